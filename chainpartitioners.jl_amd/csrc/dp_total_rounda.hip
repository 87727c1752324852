// dp_total_rounda.hip -- ROUND A FROM CACHED COUNTS and the WINDOWED ANCHORS of the total-cost DP layer (scheme: dp_total.hip): what
// depends on the pattern (and the window width) only and is kept across layers -- the anchors of the mirrored head tasks of the
// windowed layers (k_win_*, k_leaf_anchors; win_build) and the two round-A caches (k_ra_*; ra_build) -- and round A of a layer from
// them (launch_round_a; round_a_full, round_a_win_std, round_a_win_mir).
#include "dp_total.hpp"

namespace cpk {

// ---- anchors of the mirrored head tasks (windowed layers), once per (pattern, w)
// hist[e] = #{q : e(q) = e}, e(q) = min(next[q], col[q] + w, n): then  nets(max(0, r - w), r) = pos[r] - #{q : e(q) < r}   (an entry is counted by
// the window ending before r iff it lies in a column < r, is the LAST occurrence of its row before r, and its column is >= r - w)
// Without atomics (10^8 scattered atomic adds took 12.5 ms; this takes the time of two column passes): the entries with e = x are
//   * next[q] = x <= col[q] + w : one per entry q' of COLUMN x whose previous occurrence is within the window, prev[q'] >= max(0, x - w);
//   * col[q] + w = x < next[q]  : the entries of column x - w that do not come back by column x;
// one lane per column x < n (hist[n] is never read: E[r] sums the values below r <= n), eight loads in flight.
__global__ void __launch_bounds__(256) k_win_hist(int64_t n, int64_t w, const int32_t *__restrict__ pos, const int32_t *__restrict__ prev,
                                                  const int32_t *__restrict__ next, int32_t *__restrict__ hist)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > n) return;
    int32_t c = 0;
    if (x < n) {
        const int32_t lo = (int32_t)(x > w ? x - w : 0);
        for (int32_t q = pos[x], q1 = pos[x + 1]; q < q1; q += 8) {
            int32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? prev[q + k] : -1;
#pragma unroll
            for (int k = 0; k < 8; k++) c += (v[k] >= lo);
        }
        if (x >= w) {
            const int32_t xx = (int32_t)x;
            for (int32_t q = pos[x - w], q1 = pos[x - w + 1]; q < q1; q += 8) {
                int32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? next[q + k] : INT32_MIN;
#pragma unroll
                for (int k = 0; k < 8; k++) c += (v[k] > xx);
            }
        }
    }
    hist[x] = c;
}
// the same for whole rows (self nets): rows with first >= r - w and last < r  =  #{last < r} - #{max(last, first + w) < r}
__global__ void __launch_bounds__(256) k_win_hist_rows(int64_t m, int64_t n, int64_t w, const int32_t *__restrict__ rfirst, const int32_t *__restrict__ rlast,
                                                       int32_t *__restrict__ hist)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    int64_t f = rfirst[i];
    if (f < 0) return;                                      // empty row
    int64_t e = f + w, l = rlast[i];
    if (l > e) e = l;
    if (e > n) e = n;
    atomicAdd(&hist[e], 1);
}
// one wave per mirrored head (plane b < s, rho = idx << (b+1)): entries of the block's columns passing the test
//   tot[aoff[b] + idx] = #{q in the columns of the block : next[q] >= rho}   (GE)   /   #{rows starting in the block with last < rho}
template <bool GE>
__global__ void __launch_bounds__(256) k_win_block_totals(RoundDesc R, int64_t nitems, const int32_t *__restrict__ cpos, const int32_t *__restrict__ arr,
                                                          int32_t *__restrict__ tot)
{
    const int lane = threadIdx.x & 63;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < nitems; it += (int64_t)gridDim.x * 4) {
        int b = 0;
        while (it >= R.aoff[b + 1]) b++;
        const int64_t idx = it - R.aoff[b], rho = idx << (b + 1);
        int32_t c = 0;
        int64_t cs, ce;
        if (idx >= 1 && rho <= R.n && geo_block(R.G, rho, b, cs, ce)) {
            const int32_t thr = (int32_t)rho;
            for (int32_t q = cpos[cs] + lane, q1 = cpos[ce]; q < q1; q += 64) { const int32_t v = arr[q]; c += GE ? (v >= thr) : (v < thr); }
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) tot[it] = c;
    }
}
// anchor of (b, rho) = count of the whole window [max(0, rho - w), rho) minus the totals of the blocks b' <= b left of the block's end
__global__ void __launch_bounds__(256) k_win_anchors(RoundDesc R, int64_t nitems, const int64_t *__restrict__ base, const int64_t *__restrict__ E,
                                                     const int32_t *__restrict__ tot, int32_t *__restrict__ anch)
{
    int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= nitems) return;
    int b = 0;
    while (it >= R.aoff[b + 1]) b++;
    const int64_t idx = it - R.aoff[b], rho = idx << (b + 1);
    if (idx < 1 || rho > R.n) { anch[it] = 0; return; }
    int64_t v = base[rho] - E[rho];
    for (int bb = 0; bb <= b; bb++) v -= tot[R.aoff[bb] + (rho >> (bb + 1))];
    anch[it] = (int32_t)v;
}

// leaf pass: the part [64 g + 62 - w, 64 g) of every group (E from the histogram of width w - 62)
__global__ void __launch_bounds__(256) k_leaf_anchors(int64_t ng, int64_t n, const int64_t *__restrict__ base, const int64_t *__restrict__ E,
                                                      int32_t *__restrict__ anch)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int64_t r = g << 6;
    anch[g] = r <= n ? (int32_t)(base[r] - E[r]) : 0;
}

// ------------------------------------------------------------------ round A from cached counts
// Round A (row r against its lowest block [r - 2^b, r), b = ctz(r)) is the one round whose candidate ranges do not depend on
// the layer: nets(p, r) for all its (row, candidate) pairs -- sum_r 2^ctz(r) = n log2(n) / 2 values -- is computed ONCE per
// partition and kept (4 B each); a layer then evaluates round A by streaming counts, W and pos (16 B per candidate instead
// of the candidate's whole column).  Elements are stored level by level (b), row by row, candidate p = r - 1 - i at index i;
// every level is padded to whole tiles of LT elements.
// tiles of level b: [tbase[b], tbase[b+1]); rows of the levels >= 9: [rbase[b], rbase[b+1]).
// mir_w = 0: the unconstrained scheme's round-A rows -- level b holds the rows r = (2u+1) 2^b, candidates r - 1 - i, i < 2^b.
// mir_w = w > 0: the MIRRORED heads of the windowed geometry (geo_block) -- level b < s holds the rows r = (u+1) 2^(b+1),
// candidates ce - 1 - i with ce = r + 2^(b+1) - 1 - w (those below column 0 do not exist); the counts carry the head's anchor
// nets(ce, r), at aoff[b] + (r >> (b+1)) of the window anchors.  tlo / thi: the tiles of each level a windowed layer needs.

__device__ __forceinline__ int64_t ra_row(const RATab &T, int b, int64_t u)
{
    return T.mir_w ? (u + 1) << (b + 1) : ((u << 1) | 1) << b;
}

__device__ __forceinline__ bool ra_decode(const RATab &T, int64_t tile, int j, int &b, int64_t &r, int64_t &p, int64_t &i)
{
    b = 0;
    while (tile >= T.tbase[b + 1]) b++;                     // (uniform per tile)
    int64_t e = (tile - T.tbase[b]) * LT + j;               // element inside the level
    int64_t u = e >> b;
    i = e & (((int64_t)1 << b) - 1);
    r = ra_row(T, b, u);
    p = (T.mir_w ? r + ((int64_t)2 << b) - 1 - T.mir_w : r) - 1 - i;
    return r <= T.n && p >= 0;
}

// d[E] = #{q in column p : next[q] >= r} (d2: rows whose first column is p and whose last column is < r)
__global__ void __launch_bounds__(256) k_ra_colcount(RATab T, const int32_t *__restrict__ pos, const int32_t *__restrict__ next,
                                                     const int32_t *__restrict__ fpos, const int32_t *__restrict__ flast,
                                                     int32_t *__restrict__ d, int32_t *__restrict__ d2)
{
    int b; int64_t r, p, i;
    bool ok = ra_decode(T, blockIdx.x, threadIdx.x, b, r, p, i);
    int64_t E = (int64_t)blockIdx.x * LT + threadIdx.x;
    int32_t c = 0, c2 = 0;
    if (ok) {
        int32_t rr = (int32_t)r;
        for (int32_t q = pos[p], q1 = pos[p + 1]; q < q1; q += 8) {        // eight loads in flight (one at a time: a memory latency per entry)
            int32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? next[q + k] : INT32_MIN;
#pragma unroll
            for (int k = 0; k < 8; k++) c += (v[k] >= rr);
        }
        if (d2) for (int32_t q = fpos[p], q1 = fpos[p + 1]; q < q1; q++) c2 += (flast[q] < rr);
    }
    d[E] = c;
    if (d2) d2[E] = c2;
}

// c[E] = sum of d over the row's elements 0 .. i  (G = exclusive prefix sums of d over all elements)
__global__ void __launch_bounds__(256) k_ra_final(RATab T, const int64_t *__restrict__ G, int32_t *__restrict__ c, const int32_t *__restrict__ anch)
{
    int b; int64_t r, p, i;
    ra_decode(T, blockIdx.x, threadIdx.x, b, r, p, i);
    int64_t E = (int64_t)blockIdx.x * LT + threadIdx.x;
    int32_t v = (int32_t)(G[E + 1] - G[E - i]);
    if (anch && r <= T.n) v += anch[T.aoff[b] + (r >> (b + 1))];            // (mirrored heads: the part [ce, r) the block's columns stand on)
    c[E] = v;
}

template <typename TC, bool HYP>
__device__ __forceinline__ bool ra_takes(const Best<TC, HYP> &x, const Best<TC, HYP> &c)      // c replaces x: smaller value, or equal value and larger p
{
    return (x.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < x.v || (c.v == x.v && c.p > x.p)));
}

// one wave per tile of LT elements; a lane holds four consecutive elements.  Rows of up to LT candidates (b <= 8) lie inside
// one tile and are finished here; longer rows leave one partial per tile for k_ra_merge.
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_ra_layer(RATab T, int64_t ntile, const int32_t *__restrict__ cnt, const int32_t *__restrict__ cnt2,
                                                  const int32_t *__restrict__ pos, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                  int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt,
                                                  Best<TC, HYP> *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntile) return;
    const int64_t n1 = T.n + 1;
    const int64_t E0 = tile * LT + 4 * lane;
    const int4 c4 = *reinterpret_cast<const int4 *>(cnt + E0);
    int4 d4 = make_int4(0, 0, 0, 0);
    if (HYP) d4 = *reinterpret_cast<const int4 *>(cnt2 + E0);
    // the lane's first element is decoded; from level 2 on the other three are the next candidates of the same row
    int b = 0;
    int64_t r0, p0, i0;
    const bool ok0 = ra_decode(T, tile, 4 * lane, b, r0, p0, i0);
    if (tile < T.tlo[b] || tile >= T.thi[b]) return;        // (uniform) a windowed layer: rows far from its window
    Best<TC, HYP> cand[4];
    int64_t rk[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int64_t r = r0, p = p0 - k;
        bool ok = ok0 && p >= 0;                            // (mirrored heads: a block may be cut off at column 0)
        if (b < 2) { int bb; int64_t ii; ok = ra_decode(T, tile, 4 * lane + k, bb, r, p, ii); }      // (uniform branch)
        rk[k] = ok ? r : 0;
        best_clear(cand[k]);
        if (ok) {
            int32_t c = k == 0 ? c4.x : k == 1 ? c4.y : k == 2 ? c4.z : c4.w, c2 = k == 0 ? d4.x : k == 1 ? d4.y : k == 2 ? d4.z : d4.w;
            cand[k].v = cadd(W[p], dm_apply_affine(M, alpha, r - p, (int64_t)(pos[r] - pos[p]), (int64_t)c, (int64_t)c2));
            cand[k].p = (int32_t)p; cand[k].nn = c; best_set_nl(cand[k], c2);
        }
    }
    if (b < 2) {                                            // rows of one or two candidates: finished inside the lane
        const int per = 1 << b;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((k & (per - 1)) != 0 || rk[k] == 0) continue;
            Best<TC, HYP> x = cand[k];
            if (per == 2 && ra_takes(x, cand[k + 1 < 4 ? k + 1 : 3])) x = cand[k + 1 < 4 ? k + 1 : 3];
            int64_t rw = (int64_t)b * n1 + prow((rk[k]), n1 - 1);
            opt[rw] = x.p; nnopt[rw] = x.nn;
            if (HYP) nlopt[rw] = best_nl(x);
        }
        return;
    }
    Best<TC, HYP> x = cand[0];
#pragma unroll
    for (int k = 1; k < 4; k++) if (ra_takes(x, cand[k])) x = cand[k];
    const int lpr = b >= 8 ? 64 : (1 << (b - 2));          // lanes per row
    for (int o = 1; o < lpr; o <<= 1) {                     // butterfly inside the row's lanes: every lane ends with the winner
        Best<TC, HYP> c; best_clear(c);
        c.v = shfl64(x.v, lane ^ o); c.p = __shfl(x.p, lane ^ o); c.nn = __shfl(x.nn, lane ^ o);
        if (HYP) best_set_nl(c, __shfl(best_nl(x), lane ^ o));
        if (ra_takes(x, c)) x = c;
    }
    if ((lane & (lpr - 1)) == 0) {
        if (b <= 8) {
            if (rk[0]) {
                int64_t rw = (int64_t)b * n1 + prow((rk[0]), n1 - 1);
                opt[rw] = x.p; nnopt[rw] = x.nn;
                if (HYP) nlopt[rw] = best_nl(x);
            }
        } else {
            part[tile - T.tbase[9]] = x;
        }
    }
}

// The same round, COLUMN-major: one wave per 256 consecutive candidates p, all levels.  A candidate p belongs to the round-A row
// of every level b whose bit is clear in p (r = p with the bits below b cleared, plus 2^b), a dozen rows on average: k_ra_layer reads
// its cost W[p] and its column pointer once per row (16 B per (candidate, row)); here they are read once per candidate and
// only the 4-byte cached count is read per row -- 60 B instead of 190 B per candidate and layer.  Lane l holds the candidates
// P0 + 4 l .. + 3; the count elements of a row are stored by descending p (ra_decode), so a lane's four are one aligned vector.
// Rows of up to 256 candidates (b <= 8) lie inside the wave's columns and are finished here (butterfly over the row's lanes);
// longer rows leave one partial per 256 candidates for k_ra_merge, in the slot k_ra_layer would use.
template <typename TC, bool HYP, bool MIR>
__global__ void __launch_bounds__(256) k_ra_cols(RATab T, const int32_t *__restrict__ cnt, const int32_t *__restrict__ cnt2,
                                                 const int32_t *__restrict__ pos, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                 int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt,
                                                 Best<TC, HYP> *__restrict__ part, int64_t tile0, int64_t tile1, int bmin)
{
    // levels bmin .. nbits - 1 (the leaf pass computes the levels below LEAF_T itself: their rows are never multiples of 64).
    // tiles [tile0, tile1) of 256 consecutive values of the coordinate z (a windowed layer needs the rows near its window only).
    // MIR = false: z = p, the candidate p belongs to the level-b row of the block [r - 2^b, r) iff bit b of z is CLEAR.
    // MIR = true (table with mir_w = w): z = p + w + 1, p belongs to the mirrored head rho = z with the bits <= b cleared
    // (block [rho + 2^b - 1 - w, rho + 2^(b+1) - 1 - w)) iff bit b of z is SET.  In both maps a row's 2^b candidates are an aligned
    // block of z and its elements run by descending z: element i = (2^b - 1) - (z mod 2^b).
    const int lane = threadIdx.x & 63;
    const int64_t n = T.n, n1 = n + 1, off = MIR ? T.mir_w + 1 : 0;
    const int64_t Z0 = (tile0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * LT;
    if (Z0 - off >= n || Z0 >= tile1 * LT) return;          // (wave-uniform) candidates are the columns 0 .. n - 1
    const int64_t z0 = Z0 + 4 * lane, p0 = z0 - off;
    TC wv[4]; int32_t pv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { int64_t p = p0 + k; p = p < 0 ? 0 : p < n ? p : n; wv[k] = W[p]; pv[k] = pos[p]; }
    for (int b = bmin; b < T.nbits; b++) {
        if (b >= 8 && (bool)((Z0 >> b) & 1) != MIR) continue;       // (wave-uniform) no row of this level over the wave's columns
        // the lane's row of this level and its candidates among z0 .. z0 + 3:
        //   b = 0: two rows of one candidate each; b = 1: one row of two; b >= 2: all four
        const int64_t mask = ((int64_t)1 << b) - 1;
        const bool cov = b < 2 || (bool)((z0 >> b) & 1) == MIR;
        const int64_t zr = (z0 >> (b + 1)) << (b + 1);              // z0 with the bits <= b cleared
        const int64_t r = MIR ? zr : zr + ((int64_t)1 << b);        // (b = 0: the first of the lane's two rows)
        const int64_t u = MIR ? (z0 >> (b + 1)) - 1 : z0 >> (b + 1);
        // the lane's candidates k0, k0 + 1 (b = 1) or 0 .. 3 (b >= 2); element of the LAST one (the smallest index)
        const int k0 = (b == 1 && MIR) ? 2 : 0;
        const int64_t zlast = b == 1 ? z0 + k0 + 1 : z0 + 3;
        const int64_t E = (T.tbase[b] << 8) + ((u << b) | (mask - (zlast & mask)));
        int32_t c[4] = {0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
        if (b == 0) {
            // single candidates: z0 + k (k = 0, 2; mirrored: 1, 3) -> rows r, r + 2; their elements are neighbours
            const int kk = MIR ? 1 : 0;
            const int64_t E0 = (T.tbase[0] << 8) + u;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t rk = r + 2 * j, pk = p0 + kk + 2 * j;
                if (rk >= 1 && rk <= n && pk >= 0 && (!MIR || u + j >= 0)) {
                    const int64_t rw = prow((rk), n1 - 1);
                    opt[rw] = (int32_t)pk; nnopt[rw] = cnt[E0 + j]; if (HYP) nlopt[rw] = cnt2[E0 + j];
                }
            }
            continue;
        }
        const bool rok = cov && r >= 1 && r <= n && u >= 0;
        if (rok) {
            if (b >= 2) {
                const int4 t = *reinterpret_cast<const int4 *>(cnt + E);
                c[3] = t.x; c[2] = t.y; c[1] = t.z; c[0] = t.w;
                if (HYP) { const int4 t2 = *reinterpret_cast<const int4 *>(cnt2 + E); d[3] = t2.x; d[2] = t2.y; d[1] = t2.z; d[0] = t2.w; }
            } else {
                const int2 t = *reinterpret_cast<const int2 *>(cnt + E);
                c[k0 + 1] = t.x; c[k0] = t.y;
                if (HYP) { const int2 t2 = *reinterpret_cast<const int2 *>(cnt2 + E); d[k0 + 1] = t2.x; d[k0] = t2.y; }
            }
        }
        const int32_t posr = pos[rok ? r : 0];
        Best<TC, HYP> x; best_clear(x);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (b == 1 && (k < k0 || k > k0 + 1)) continue;
            if (!rok || p0 + k < 0) continue;               // (mirrored heads: a block may be cut off at column 0)
            Best<TC, HYP> cc; best_clear(cc);
            cc.v = cadd(wv[k], dm_apply_affine(M, alpha, r - (p0 + k), (int64_t)(posr - pv[k]), (int64_t)c[k], (int64_t)d[k]));
            cc.p = (int32_t)(p0 + k); cc.nn = c[k]; best_set_nl(cc, d[k]);
            if (ra_takes(x, cc)) x = cc;
        }
        const int lpr = b <= 2 ? 1 : b >= 8 ? 64 : (1 << (b - 2));          // lanes per row
        for (int o = 1; o < lpr; o <<= 1) {                 // butterfly inside the row's lanes: every lane ends with the winner
            Best<TC, HYP> cc; best_clear(cc);
            cc.v = shfl64(x.v, lane ^ o); cc.p = __shfl(x.p, lane ^ o); cc.nn = __shfl(x.nn, lane ^ o);
            if (HYP) best_set_nl(cc, __shfl(best_nl(x), lane ^ o));
            if (ra_takes(x, cc)) x = cc;
        }
        if ((lane & (lpr - 1)) == 0 && rok) {
            if (b <= 8) {
                if (x.p >= 0) {
                    const int64_t rw = (int64_t)b * n1 + prow((r), n1 - 1);
                    opt[rw] = x.p; nnopt[rw] = x.nn;
                    if (HYP) nlopt[rw] = best_nl(x);
                }
            } else {
                // lane 0: the wave's smallest element of the row is that of its last column
                const int64_t el = (u << b) | (mask - ((Z0 + LT - 1) & mask));
                part[T.tbase[b] + (el >> 8) - T.tbase[9]] = x;
            }
        }
    }
}

// rows of more than LT candidates (b >= 9): one wave per row merges the row's tile partials
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_ra_merge(RATab T, int64_t nrow, const Best<TC, HYP> *__restrict__ part,
                                                  int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nrow) return;
    int b = 9;
    while (w >= T.rbase[b + 1]) b++;
    const int64_t u = w - T.rbase[b], r = ra_row(T, b, u), n1 = T.n + 1;
    const int64_t t0 = T.tbase[b] + (u << (b - 8)) - T.tbase[9], cntt = (int64_t)1 << (b - 8);
    Best<TC, HYP> x; best_clear(x);
    // (the top row's block is half the matrix -- 2^15 partials at n = 10^7: eight loads per lane in flight; one at a time, that row
    //  alone made the kernel 160 us long)
    for (int64_t kb = lane; kb < cntt; kb += 512) {
        Best<TC, HYP> cc[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { best_clear(cc[u]); if (kb + 64 * u < cntt) cc[u] = part[t0 + kb + 64 * u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) if (kb + 64 * u < cntt && ra_takes(x, cc[u])) x = cc[u];
    }
    for (int o = 32; o > 0; o >>= 1) {
        Best<TC, HYP> c; best_clear(c);
        c.v = shfl64(x.v, lane ^ o); c.p = __shfl(x.p, lane ^ o); c.nn = __shfl(x.nn, lane ^ o);
        if (HYP) best_set_nl(c, __shfl(best_nl(x), lane ^ o));
        if (ra_takes(x, c)) x = c;
    }
    if (lane == 0 && r <= T.n) {
        int64_t rw = (int64_t)b * n1 + prow((r), n1 - 1);
        opt[rw] = x.p; nnopt[rw] = x.nn;
        if (HYP) nlopt[rw] = best_nl(x);
    }
}

// Builds a cached round-A table: the counts of `levels` levels of rows_of(b) rows each (they depend on the pattern only -- once per
// partition; the table of the mirrored heads of the windowed geometry, mir_w > 0, also on the window width: once per (pattern, w),
// after win_build, whose anchors `anch` / `anch2` its counts carry).  Fills the cache's table, counts (c2: second count) and
// sizes; `part` gets room for the partials of the rows of more than LT candidates.
template <typename TC, typename Rows>
static void ra_build(cp_csr_s *A, LayerWork<TC> &Wk, RaCache<TC> &Ra, int levels, Rows rows_of, int64_t mir_w, const int32_t *anch, const int32_t *anch2)
{
    hipStream_t s = A->stream;
    const bool hyp = Wk.hyp;
    RATab &T = Ra.tab;
    memset(&T, 0, sizeof(T));
    T.nbits = levels; T.n = A->n; T.mir_w = mir_w;
    for (int b = 0; b < 33; b++) { T.tlo[b] = 0; T.thi[b] = INT64_MAX; T.aoff[b] = (mir_w && b < 32) ? Wk.win.aoff[b] : 0; }
    int64_t tb = 0, rb = 0;
    for (int b = 0; b < 33; b++) {
        T.tbase[b] = tb; T.rbase[b] = rb;
        if (b >= levels) continue;
        const int64_t nrows = rows_of(b);
        tb += cdiv(nrows << b, LT);
        if (b >= 9) rb += nrows;
    }
    Ra.ntile = tb; Ra.nrow = rb;
    const size_t total = (size_t)tb * LT;
    Ra.c.ensure(total + 8);
    if (hyp) Ra.c2.ensure(total + 8);
    Ra.part.ensure((size_t)std::max<int64_t>(1, tb - T.tbase[9]));
    if (tb > 0) {
        DBuf<int64_t> &G = Wk.sc.ra_G, &scratch = Wk.sc.scratch;        // (kept with the layer scratch: 8 B per element)
        G.ensure(total + 1);
        hipLaunchKernelGGL(k_ra_colcount, dim3((unsigned)tb), dim3(LT), 0, s, T, A->pos32.p, A->next.p, hyp ? A->fpos32.p : (const int32_t *)nullptr,
                           hyp ? A->flast.p : (const int32_t *)nullptr, Ra.c.p, hyp ? Ra.c2.p : (int32_t *)nullptr);
        exclusive_scan_i32(Ra.c.p, G.p, (int64_t)total, scratch, s);
        hipLaunchKernelGGL(k_ra_final, dim3((unsigned)tb), dim3(LT), 0, s, T, G.p, Ra.c.p, anch);
        if (hyp) {
            exclusive_scan_i32(Ra.c2.p, G.p, (int64_t)total, scratch, s);
            hipLaunchKernelGGL(k_ra_final, dim3((unsigned)tb), dim3(LT), 0, s, T, G.p, Ra.c2.p, anch2);
        }
        CP_HIP(hipGetLastError());
    }
    Ra.built = true; Ra.w = mir_w;
}
// the table of the unconstrained scheme's round A (the windowed layers' standard heads are its levels below s)
template <typename TC>
static void ra_build_std(cp_csr_s *A, LayerWork<TC> &Wk)
{
    const int64_t n = A->n;
    ra_build<TC>(A, Wk, Wk.ra, Wk.nbits, [n](int b) { return ((n >> b) + 1) >> 1; }, 0, nullptr, nullptr);
}
// ... and of the mirrored heads of the current window: rows (u + 1) 2^(b+1) <= n
template <typename TC>
static void ra_build_mir(cp_csr_s *A, LayerWork<TC> &Wk)
{
    const int64_t n = A->n;
    ra_build<TC>(A, Wk, Wk.mir, Wk.G.s, [n](int b) { return n >> (b + 1); }, Wk.G.w, Wk.win.w_anch.p, Wk.win.w_anch2.p);
}

// the nets (pass 0) / self nets (pass 1) a window of width x cuts, per column into w_hist and as prefix sums into w_E
template <typename TC>
static void win_hist_scan(cp_csr_s *A, LayerWork<TC> &Wk, int64_t x, int pass)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    if (pass == 1 || A->N == 0) CP_HIP(hipMemsetAsync(Wk.win.w_hist.p, 0, sizeof(int32_t) * (size_t)(n + 1), s));
    if (pass == 0) { if (A->N > 0) hipLaunchKernelGGL(k_win_hist, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, n, x, A->pos32.p, A->prev.p, A->next.p, Wk.win.w_hist.p); }
    else if (A->m > 0) hipLaunchKernelGGL(k_win_hist_rows, dim3((unsigned)cdiv(A->m, 256)), dim3(256), 0, s, A->m, n, x, A->rfirst.p, A->rlast.p, Wk.win.w_hist.p);
    exclusive_scan_i32(Wk.win.w_hist.p, Wk.win.w_E.p, n + 1, Wk.sc.scratch, s);
}

// anchors of the mirrored head tasks of the windowed layers (k_win_*): once per (pattern, w)
template <typename TC>
void win_build(cp_csr_s *A, LayerWork<TC> &Wk)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, w = Wk.G.w;
    const int sb = Wk.G.s;
    int64_t acc = 0;
    for (int b = 0; b < 33; b++) { Wk.win.aoff[b] = acc; if (b < sb) acc += (n >> (b + 1)) + 1; }      // heads of plane b: rho = idx << (b+1), idx <= n >> (b+1)
    Wk.win.nitems = acc;
    const size_t ni = (size_t)(acc > 0 ? acc : 1);
    Wk.win.w_anch.ensure(ni); Wk.win.w_tot.ensure(ni); Wk.win.w_hist.ensure((size_t)n + 2); Wk.win.w_E.ensure((size_t)n + 2);
    if (Wk.hyp) Wk.win.w_anch2.ensure(ni);
    Wk.win.built = false;
    if (acc > 0) {
        RoundDesc R;
        make_round(R, true, 0, sb + 1, n, 0, n, Wk.G, Wk.win.aoff);
        const unsigned wg = (unsigned)std::min<int64_t>(cdiv(acc, 4), 65536);
        for (int pass = 0; pass < (Wk.hyp ? 2 : 1); pass++) {
            win_hist_scan<TC>(A, Wk, w, pass);
            if (pass == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_win_block_totals<true>), dim3(wg), dim3(256), 0, s, R, acc, A->pos32.p, A->next.p, Wk.win.w_tot.p);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_win_block_totals<false>), dim3(wg), dim3(256), 0, s, R, acc, A->fpos32.p, A->flast.p, Wk.win.w_tot.p);
            hipLaunchKernelGGL(k_win_anchors, dim3((unsigned)cdiv(acc, 256)), dim3(256), 0, s, R, acc, pass == 0 ? A->pos.p : A->lpos.p, Wk.win.w_E.p, Wk.win.w_tot.p,
                               pass == 0 ? Wk.win.w_anch.p : Wk.win.w_anch2.p);
        }
        CP_HIP(hipGetLastError());
    }
    // leaf pass (dp_total_leaf.hip): anchors of the inner mirrored blocks, nets(64 g + 62 - w, 64 g) for every group g -- the same
    // histogram with the width w - 62
    Wk.win.leaf_anch.release(); Wk.win.leaf_anch2.release();
    if (sb >= LEAF_T && w > 62) {
        const int64_t ng = (n >> LEAF_T) + 1;
        Wk.win.leaf_anch.alloc((size_t)ng);
        if (Wk.hyp) Wk.win.leaf_anch2.alloc((size_t)ng);
        for (int pass = 0; pass < (Wk.hyp ? 2 : 1); pass++) {
            win_hist_scan<TC>(A, Wk, w - 62, pass);
            hipLaunchKernelGGL(k_leaf_anchors, dim3((unsigned)cdiv(ng, 256)), dim3(256), 0, s, ng, n, pass == 0 ? A->pos.p : A->lpos.p, Wk.win.w_E.p,
                               pass == 0 ? Wk.win.leaf_anch.p : Wk.win.leaf_anch2.p);
        }
        CP_HIP(hipGetLastError());
    }
    Wk.win.built = true; Wk.win.w = w;
}

// Round A from a cache with the table T (the cache's own, or a copy cut to the levels and tiles a windowed layer needs): the
// column-major kernel over the candidate tiles [tile0, tile1) (`mirrored`: the table of the mirrored heads) or the row-major one
// over the cache's tiles, then the rows of more than LT candidates (nrow_merge of them) merge their partials.
template <typename TC, bool HYP>
static void launch_round_a(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RaCache<TC> &Ra, const RATab &T, int64_t nrow_merge, int64_t tile0, int64_t tile1,
                           int bmin, bool mirrored, bool colmajor)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    int32_t *nl = if_hyp<HYP>(Wk.pl.nlopt.p);
    if (colmajor)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mirrored ? k_ra_cols<TC, HYP, true> : k_ra_cols<TC, HYP, false>), dim3((unsigned)std::max<int64_t>(1, cdiv(tile1 - tile0, 4))), dim3(256), 0, s,
                           T, Ra.c.p, if_hyp<HYP>(Ra.c2.p), A->pos32.p, C.W, C.M, C.alpha, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, recs<HYP>(Ra.part), tile0, tile1, bmin);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ra_layer<TC, HYP>), dim3((unsigned)cdiv(Ra.ntile, 4)), dim3(256), 0, s, T, Ra.ntile, Ra.c.p, if_hyp<HYP>(Ra.c2.p), A->pos32.p, C.W, C.M,
                           C.alpha, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, recs<HYP>(Ra.part));
    if (nrow_merge > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ra_merge<TC, HYP>), dim3((unsigned)cdiv(nrow_merge, 4)), dim3(256), 0, s, T, nrow_merge, recs<HYP>(Ra.part), Wk.pl.opt.p,
                           Wk.pl.nnopt.p, nl);
    CP_HIP(hipGetLastError());
}

// A full layer: round A of the rows' lowest blocks from the cached counts; what is left of round A for the generic round is the
// last row in its upper planes
template <typename TC, bool HYP>
void round_a_full(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    if (!Wk.ra.built) { ProfScope ps(PROF_LINKS, s, 0.0); ra_build_std<TC>(C.A, Wk); }
    ProfScope ps(PROF_RA, s, 16.0 * (double)Wk.ra.ntile * LT);
    launch_round_a<TC, HYP>(C, Wk, Wk.ra, Wk.ra.tab, Wk.ra.nrow, 0, cdiv(C.n, LT), C.ra_bmin, false, !(g_opt_dbg & DBG_RA_ROWMAJOR));
}

// Windowed layer: the STANDARD heads of round A (rows with ctz == b < s, block [r - 2^b, r)) are the unconstrained scheme's
// round-A rows of the levels below s -- same blocks, same layer-independent counts: k_ra_cols computes them for all rows
// from the cache (60 B per candidate) and the generic round keeps the mirrored and common heads only.  The heads the layer
// reads are those make_round lists -- within 2^(b+1) of the row tile in plane b <= s: their blocks start at rlo - 3 * 2^s or later.
// `scope`: the stage's profile scope, opened here behind the table build and closed by the caller (the mirrored heads have always
// been enqueued inside it).
template <typename TC, bool HYP>
void round_a_win_std(const LayerCtx<TC> &C, LayerWork<TC> &Wk, std::optional<ProfScope> &scope)
{
    hipStream_t s = C.s;
    const Geo &G = C.G;
    const int64_t n = C.n, rlo = C.rlo, rhi = C.rhi;
    if (!Wk.ra.built) { ProfScope ps(PROF_LINKS, s, 0.0); ra_build_std<TC>(C.A, Wk); }
    RATab T2 = Wk.ra.tab;
    T2.nbits = std::min<int32_t>(G.s, Wk.ra.tab.nbits);
    const int64_t nrow2 = T2.nbits > 9 ? Wk.ra.tab.rbase[T2.nbits] : 0;
    const int64_t c_lo = std::max<int64_t>(0, (rlo > 0 ? rlo : 0) - ((int64_t)4 << G.s)), c_hi = std::min<int64_t>(n, rhi);
    const int64_t tile0 = c_lo / LT, tile1 = cdiv(c_hi, LT);
    scope.emplace(PROF_RA, s, 60.0 * (double)(tile1 - tile0) * LT);
    // (the standard heads below LEAF_T are rows inside a leaf group: the leaf pass computes them; the MIRRORED heads of those
    //  levels include the multiples of 64 -- every row has a task in every plane -- and stay)
    launch_round_a<TC, HYP>(C, Wk, Wk.ra, T2, nrow2, tile0, tile1, C.ra_bmin, false, true);
}

// Windowed layer: the MIRRORED heads of round A the same way, from their own table (per level the tiles of the rows near the
// window); false: the table is empty, the heads stay generic tasks
template <typename TC, bool HYP>
bool round_a_win_mir(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    const Geo &G = C.G;
    const int64_t n = C.n, rlo = C.rlo, rhi = C.rhi;
    if (!Wk.mir.built || Wk.mir.w != G.w) { ProfScope ps2(PROF_LINKS, s, 0.0); ra_build_mir<TC>(C.A, Wk); }
    if (Wk.mir.ntile <= 0) return false;
    RATab T3 = Wk.mir.tab;
    const int64_t r_lo = std::max<int64_t>(1, (rlo > 0 ? rlo : 0) - ((int64_t)4 << G.s)), r_hi = std::min<int64_t>(n, rhi);
    double elems = 0;
    for (int b = 0; b < T3.nbits; b++) {
        const int64_t u_lo = std::max<int64_t>(0, (r_lo >> (b + 1)) - 1), u_hi = r_hi >> (b + 1);        // rows u_lo .. u_hi - 1
        T3.tlo[b] = T3.tbase[b] + ((u_lo << b) / LT);
        T3.thi[b] = std::min<int64_t>(T3.tbase[b + 1], T3.tbase[b] + cdiv(std::max<int64_t>(u_hi, 0) << b, LT));
        elems += (double)std::max<int64_t>(0, T3.thi[b] - T3.tlo[b]) * LT;
    }
    // column-major like the standard heads (z = p + w + 1: the blocks of the rows r_lo .. r_hi lie in [r_lo, r_hi + 2^s)); the
    // row-major kernel reads 16 B per (candidate, level) instead of 4
    const bool mcols = !(g_opt_dbg & DBG_MIR_ROWMAJOR);
    const int64_t zt0 = r_lo / LT, zt1 = cdiv(std::min<int64_t>(n + G.w + 1, r_hi + ((int64_t)1 << G.s) + 1), LT);
    ProfScope ps2(PROF_RA, s, mcols ? 80.0 * (double)(zt1 - zt0) * LT : 16.0 * elems);
    launch_round_a<TC, HYP>(C, Wk, Wk.mir, T3, Wk.mir.nrow, zt0, zt1, 0, true, mcols);
    return true;
}

template void win_build<int64_t>(cp_csr_s *, LayerWork<int64_t> &);
template void win_build<double>(cp_csr_s *, LayerWork<double> &);
#define CP_INST(TC, HYP) \
    template void round_a_full<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &); \
    template void round_a_win_std<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, std::optional<ProfScope> &); \
    template bool round_a_win_mir<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &);
CP_INST(int64_t, false) CP_INST(int64_t, true) CP_INST(double, false) CP_INST(double, true)
#undef CP_INST

}  // namespace cpk

