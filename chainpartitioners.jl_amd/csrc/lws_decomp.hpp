// lws_decomp.hpp -- the cells between two monotone staircases a(r) <= p <= b(r) as full rectangles and scans of partial rows: the
// off-line decomposition of dp_total_budget.hip (a, b from the weight's j0 array) and of sym_total.hip (a, b in closed form).
//
// A block [ja, jb] of candidates meets the contiguous rows with b(r) >= ja and a(r) <= jb; those with a(r) <= ja and b(r) >= jb see
// every candidate of the block -- again contiguous, one FULL rectangle -- and the rows above it (cut by b) and below it (cut by a)
// recurse into the two halves of the block, or, below stair_cols columns, are scanned whole.  Every feasible cell lies in exactly
// one rectangle or scan.
//
//     B::first_b_ge(x, y, v)            the first row of [x, y] with b(r) >= v; y + 1: none
//     B::last_a_le(x, y, v)             the last row of [x, y] with a(r) <= v; x - 1: none
//     S::rect(depth, ja, jb, ra, rb)    a full rectangle, found at this depth of the column tree (the whole block: depth 0)
//     S::stair(depth, ja, jb, ra, m, ra2, m2)      the partial rows [ra, ra + m) and [ra2, ra2 + m2) of a narrow block
#pragma once
#include <cstdint>

namespace cpk {

template <typename B, typename S>
void stair_decompose(const B &bounds, S &sink, int64_t stair_cols, int64_t ja, int64_t jb, int64_t ra, int64_t rb, int depth = 0)
{
    if (ja > jb || ra > rb) return;
    // the rows that meet the block: b(r) >= ja (a suffix of the rows) and a(r) <= jb (a prefix)
    const int64_t s = bounds.first_b_ge(ra, rb, ja), e = bounds.last_a_le(ra, rb, jb);
    if (s > e) return;
    // ... and among them those that see all of it: b(r) >= jb (a suffix) and a(r) <= ja (a prefix)
    const int64_t f1 = bounds.first_b_ge(s, e, jb), f2 = bounds.last_a_le(s, e, ja);
    int64_t t0 = s, t1 = e, u0 = e + 1, u1 = e;      // partial rows above [t0, t1] and below [u0, u1] the rectangle; none full: all in the first
    if (f1 <= f2) {
        sink.rect(depth, ja, jb, f1, f2);
        t1 = f1 - 1; u0 = f2 + 1;
    }
    if (t1 < t0 && u1 < u0) return;
    if (jb - ja < stair_cols) { sink.stair(depth, ja, jb, t0, t1 - t0 + 1, u0, u1 - u0 + 1); return; }
    const int64_t jm = (ja + jb) / 2;
    stair_decompose(bounds, sink, stair_cols, ja, jm, t0, t1, depth + 1); stair_decompose(bounds, sink, stair_cols, jm + 1, jb, t0, t1, depth + 1);
    stair_decompose(bounds, sink, stair_cols, ja, jm, u0, u1, depth + 1); stair_decompose(bounds, sink, stair_cols, jm + 1, jb, u0, u1, depth + 1);
}

}  // namespace cpk
