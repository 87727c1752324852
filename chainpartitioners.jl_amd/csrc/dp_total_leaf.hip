// dp_total_leaf.hip -- the LEAF PASS of a total-cost DP layer (dp_total.hip), and the combine of the per-plane winners.
//
// The divide and conquer of dp_total.hip halves the row distance per round; its last six rounds (tau = 5 .. 0) hold 63 of 64
// rows, and almost every task there is ONE candidate (the winners of the two tree neighbours coincide): a task record, four
// plane gathers, a right-part count and two plane stores per (row, plane) for a value that is a handful of adds.  The leaf
// pass replaces those rounds: one WAVE takes one group of rows g*64 < r < (g+1)*64 (lane i <-> row g*64 + i) after the rounds
// tau >= 6 have given the two bounding rows rL = g*64 and rR = (g+1)*64 their per-plane winners, and finishes the 63 rows in
// one go -- including the final combine over the planes, so the leaf rows never write or re-read the plane arrays:
//
//   INNER planes b < 6 (blocks inside the group).  The Fenwick blocks of the set bits b < 6 of row r tile [g*64, r): together
//     they are the reference's own sweep  min over g*64 <= p < r of W[p] + f(p, r)  (DynamicSplitter.jl:38-44) restricted to the
//     group, walked from p = r - 1 downwards with strict < (the largest p wins ties, like the combine order "lower planes
//     first").  nets(p, r) = pins(p, r) - #{q in cols [p, r) : next[q] < r}  (an entry is the last of its row in [p, r) unless
//     the row comes back before r): only entries whose next column lies INSIDE the group ever count -- they are compacted into
//     an LDS list while the group's entries are streamed (a handful per group on SuiteSparse-shaped patterns, all of them on
//     banded ones).  Self nets: rows with first == c, last < r, from the rows bucketed by first column.
//   OUTER planes b >= 6 (set bits of g: the same for every row of the group).  Candidates [a, B], B = opt[b][rL], a = opt[b][rR]
//     (block start when rR leaves the rectangle), exactly the bounds the divide and conquer would hand down;
//        nets(p, r) = nets(B, rL) + R_B(r) + C(p, r),   R_B(r) = #{q in cols [rL, r) : prev[q] < B},
//                                                       C(p, r) = #{q in cols [p, B) : next[q] >= r}.
//     R_B(r) for all planes at once: the group's entries are streamed ONCE, 64 per step; per plane one compare into a lane mask
//     and every row-lane counts the mask bits in front of its column's end (4 VALU instructions per (step, plane)).
//     C(p, r) is the same for all 63 rows unless next[q] falls strictly inside the group ("special", cf. the gap passes):
//     without specials the rows share ONE arg-min over the candidates -- a wave reduction of the row-independent part
//     U(p) = W[p] - p b_v - pos[p] b_p + C(p) b_n -- and differ by a row-only term; with specials every row-lane walks the
//     candidates itself.  A single candidate (a == B, the common case) needs no entry at all.
//   Rows finished by a gap pass of a round tau >= 6 (fin) are read back from the planes.
//
// Ties: every comparison is strict < in walking order (diagonal, inner p descending, outer planes ascending, p descending
// inside a plane), i.e. the largest p wins, as in the reference (DynamicSplitter.jl:40 `<=` while scanning upwards).
// Arithmetic: the eligible models (fast_total_ok) are exact -- Int64 totals below 2^60 (no wrap) or Float64 with integer values
// below 2^53 -- so the affine costs may be split into a row part and a candidate part.
//
// WIDTH-WINDOWED layers (struct Geo; candidates max(0, r - w) <= p <= r with 2^6 <= 2^s <= w): the outer planes
// are ALL planes 6 .. s (standard, mirrored or common: the block is the same for the 64 rows of a group), with the same bounds
// (B, a) and anchors from the two bounding rows; the inner standard blocks tile [g*64, r) as before; and the inner MIRRORED blocks
// (clear bits b < 6 of r) tile [r - w, g*64 + 63 - w): one more pseudo-plane whose head B = g*64 + 62 - w is a real candidate
// with the layer-independent anchor nets(B, g*64) (cached per pattern and width, LeafArgs::anchM), and whose candidate count
// depends on the row: row g*64 + i takes B, B - 1, .., B - (62 - i) -- a prefix-min scan over the candidates instead of one
// arg-min.  Everything is "smaller value, then larger p", so the order of the planes does not matter.
//
// cp_set_option("block_tables", 1) makes the pass also store every per-block winner and its counts (cp_dp_block_tables: tests).

#include "dp_total.hpp"

namespace cpk {

template <typename TC, bool HYP>
struct LeafArgs {
    int64_t n, g0, ngroups, c0, c1;      // groups g0 .. g0 + ngroups - 1; rows written: c0 <= r <= c1
    int32_t nbits, planes;               // planes: also store the per-block winners (block tables)
    const int32_t *pos, *prev, *next, *col;
    const int32_t *fpos, *flast, *ffirst, *lpos, *lfirst;
    int32_t *opt, *nnopt, *nlopt; const uint8_t *fin; int32_t fin_stamp;       // fin: set iff == fin_stamp
    const TC *W; DevModel<TC> M; TC alpha;
    TC *cst; int32_t *ptr;
    Geo G;                               // G.win: width-windowed layer
    const int32_t *anchM, *anchM2;       // windowed: nets / self nets of the part [g*64 + 62 - w, g*64) per group
    int32_t lcap; int32_t *err;          // a plane with more candidates than lcap: flag the layer for a redo (*err = 1) and skip it
    int32_t *pz;                         // poison mode (tests): count plane cells read that nobody wrote
};

__device__ __forceinline__ uint64_t leaf_lowmask(int32_t w) { return w <= 0 ? 0ull : (w >= 64 ? ~0ull : ((1ull << w) - 1ull)); }
__device__ __forceinline__ int64_t rdl64u(int64_t v, int src) { return rdl64(v, src); }
__device__ __forceinline__ double rdl64u(double v, int src) { return rdl64(v, src); }

// cnt[j] += #{lanes of the step whose value passes plane j's test and lie under the lane's mask}, planes 0 .. nact - 1, three
// planes per scalar test (a counter past nact may collect garbage: it is never read).  Per plane: a compare into a lane mask, two ANDs
// and two v_bcnt with accumulate (the popcount of a 64-bit mask written in C gets a separate add).
__device__ __forceinline__ int32_t leaf_bcnt(uint32_t m, int32_t acc)
{
    int32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(m), "v"(acc));
    return r;
}
template <int NP, bool GE>
__device__ __forceinline__ void leaf_count(int32_t (&cnt)[NP], const int32_t (&thr)[NP], int nact, int32_t v, uint64_t lm)
{
    const uint32_t lo = (uint32_t)lm, hi = (uint32_t)(lm >> 32);
#pragma unroll
    for (int j0 = 0; j0 < NP; j0 += 3) {
        if (j0 < nact) {                                                 // (scalar)
#pragma unroll
            for (int j = j0; j < j0 + 3; j++) {
                if (j < NP) {
                    const uint64_t mb = __ballot(GE ? (v >= thr[j]) : (v < thr[j]));
                    cnt[j] = leaf_bcnt((uint32_t)(mb >> 32) & hi, leaf_bcnt((uint32_t)mb & lo, cnt[j]));
                }
            }
        }
    }
}

// Entries [e_lo, e_hi) of a run of candidate columns, 256 per step (four loads in flight): every candidate-lane gets the number of
// entries AT OR AFTER its own column start `mine` that every row of the group counts (LEFT = false: next >= hiG - 1; LEFT = true:
// last column <= gG), `tot` the number over the whole range, and the return value tells whether an entry is counted by SOME rows
// of the group only (strictly inside (gG, hiG - 1): "special").
template <bool LEFT>
__device__ __forceinline__ bool leaf_suffix(const int32_t *__restrict__ arr, int32_t e_lo, int32_t e_hi, int32_t mine, int32_t gG, int32_t hiG, int lane,
                                            int32_t &C, int32_t &tot)
{
    bool spec = false;
    for (int32_t base0 = e_lo; base0 < e_hi; base0 += 256) {
        int32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const int32_t q = base0 + 64 * k + lane; v[k] = q < e_hi ? arr[q] : (LEFT ? INT32_MAX : INT32_MIN); }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int32_t base = base0 + 64 * k;
            if (base < e_hi) {                                           // (wave-uniform)
                const uint64_t mb = __ballot(LEFT ? (v[k] <= gG) : (v[k] >= hiG - 1));
                if (__ballot(v[k] > gG && v[k] < hiG - 1)) spec = true;
                const int32_t t = (int32_t)__popcll(mb);
                C += t - (int32_t)__popcll(mb & leaf_lowmask(mine - base));
                tot += t;
            }
        }
    }
    return spec;
}

#ifndef CP_LEAF_SKIP
#define CP_LEAF_SKIP 0      // timing experiments (tools/leaf_parts.py): 1 no right-part counts, 2 no multi-candidate planes, 4 no one-candidate planes, 8 no inner planes
#endif
#ifndef CP_LEAF_WPB
#define CP_LEAF_WPB 2
#endif
// The specials of a run of candidate columns (see leaf_suffix): for every entry with a value strictly inside (gG, hiG - 1) the list gets
// (candidate index of its column << 8) | (value - gG).  Lane i holds candidate column B - i, whose entries start at `mine` (columns
// descend with the lane, so the candidate index of position q is the number of lanes whose column starts above q).  Entries come in
// ascending position = DEscending candidate index.  -> their number (the list keeps the first LEAF_LIST).
template <bool LEFT>
__device__ __forceinline__ int leaf_specials(const int32_t *__restrict__ arr, int32_t e_lo, int32_t e_hi, int32_t mine, bool cv, int32_t gG, int32_t hiG, int lane,
                                             uint16_t *__restrict__ list)
{
    int ns = 0;
    for (int32_t base = e_lo; base < e_hi; base += 64) {
        const int32_t q = base + lane;
        const int32_t v = q < e_hi ? arr[q] : INT32_MIN;
        uint64_t m = __ballot(v > gG && v < hiG - 1);
        while (m) {
            const int u = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int32_t iq = (int32_t)__popcll(__ballot(cv && mine > base + u));
            const int32_t val = rdl(v, u);
            if (lane == 0 && ns < LEAF_LIST) list[ns] = (uint16_t)((iq << 8) | (val - gG));
            ns++;
        }
    }
    return ns;
}

template <bool HYP> struct LeafWPB { static constexpr int v = CP_LEAF_WPB; };        // waves (groups) per workgroup

// NP: outer planes 6 .. 6 + NP - 1 (18: n < 2^24)
template <typename TC, bool HYP, int NP>
__global__ void __launch_bounds__(64 * LeafWPB<HYP>::v) k_leaf(LeafArgs<TC, HYP> A)
{
    constexpr int WPB = LeafWPB<HYP>::v;
    // (wave-uniform values go through readfirstlane: the compiler then branches on the scalar unit instead of masking lanes)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t g = A.g0 + (int64_t)blockIdx.x * WPB + wv;
    if (g >= A.g0 + A.ngroups) return;                                   // (wave-uniform)
    if ((g << LEAF_T) >= A.n || (g << LEAF_T) >= A.c1) return;           // no row of the group is wanted (n or the tile end a multiple of 64)
    __shared__ uint16_t s_list_all[WPB][HYP ? 2 : 1][LEAF_LIST];
    uint16_t(*s_list)[LEAF_LIST] = s_list_all[wv];
    const int64_t n = A.n, n1 = n + 1;
    const DevModel<TC> &M = A.M;
    const TC alpha = A.alpha;
    const int32_t gG = (int32_t)(g << LEAF_T);
    const int32_t hiG = gG + LEAF_G;                                     // first row of the next group
    const int32_t r = gG + lane;
    const int32_t rq = r <= n ? r : (int32_t)n;
    const bool rvalid = lane >= 1 && r <= n;
    const int32_t posr = A.pos[rq];
    const TC Wr = A.W[rq];
    const int32_t gE = hiG <= n ? hiG : (int32_t)n;                      // columns [gG, gE) exist
    const int32_t q0 = rdl(posr, 0), q1 = A.pos[gE];
    int32_t lposr = 0, fposr = 0, l0 = 0, l1 = 0, f0 = 0, f1 = 0;
    if (HYP) { lposr = A.lpos[rq]; fposr = A.fpos[rq]; l0 = rdl(lposr, 0); l1 = A.lpos[gE]; f0 = rdl(fposr, 0); f1 = A.fpos[gE]; }
    const int64_t slot = r >= 1 ? prow(((int64_t)rq), n1 - 1) : 0;                   // plane slot of this lane's row

    // ---- outer planes of the group.  Unconstrained: lane j holds the j-th set bit of g.  Windowed: lane j holds plane 6 + j for
    // every plane up to s, and lane s - 5 the pseudo-plane of the inner mirrored blocks.  pl_fin: 1 = finished by a gap pass,
    // 2 = no block here (skip)
    const uint32_t gbits = (uint32_t)g;
    const bool win = A.G.win != 0;
    const int nreal = __builtin_amdgcn_readfirstlane(win ? A.G.s - LEAF_T + 1 : __popc(gbits));
    const int nact = win ? nreal + 1 : nreal;
    int32_t pl_b = 0, pl_B = 0, pl_a = 0, pl_nn = 0, pl_nl = 0, pl_fin = 0;
    TC pl_U = (TC)0;                                                     // row-independent part of the head candidate's cost
    // (windowed: lane 0 <-> plane 6, lane 1 <-> the pseudo-plane, lanes 2 .. <-> planes 7 .. s: the two planes every group has to
    //  walk candidate by candidate sit at fixed counter registers)
    if (win ? (lane < nact && lane != 1) : lane < nreal) {
        int b;
        int64_t cs = 0, ce = 0;
        bool have = true;
        if (win) { b = lane == 0 ? LEAF_T : LEAF_T + lane - 1; have = gG > 0 && geo_block(A.G, (int64_t)gG, b, cs, ce); }
        else {
            uint32_t t = gbits;
            for (int k = 0; k < lane; k++) t &= t - 1;
            b = LEAF_T + (__ffs(t) - 1);
        }
        pl_b = b;
        if (!have) pl_fin = 2;
        else {
            const int64_t sL = (int64_t)b * n1 + prow(((int64_t)gG), n1 - 1);
            pl_B = A.opt[sL]; pl_nn = A.nnopt[sL];
            if (HYP) pl_nl = A.nlopt[sL];
            const int64_t rb = ((int64_t)gG >> b) << b, rR = (int64_t)hiG;
            if (win) pl_a = (rR < rb + ((int64_t)1 << b) && rR <= n) ? A.opt[(int64_t)b * n1 + prow((rR), n1 - 1)] : (int32_t)cs;
            else pl_a = (rR - rb) < ((int64_t)1 << b) ? A.opt[(int64_t)b * n1 + prow((rR <= n ? rR : n), n1 - 1)] : (int32_t)(rb - ((int64_t)1 << b));
            if (pl_a > pl_B) pl_a = pl_B;                                // (cannot happen for an inverse-Monge cost; keeps the ranges well-formed)
            pl_fin = A.fin[(int64_t)b * n1 + prow(((int64_t)gG + 1), n1 - 1)] == (uint8_t)A.fin_stamp;      // (gG + 1 <= n: the group has a row)
        }
    } else if (win && lane == 1) {
        const int64_t Bm = (int64_t)gG + 62 - A.G.w;
        pl_b = 255;
        if (Bm < 0) pl_fin = 2;
        else {
            pl_B = (int32_t)Bm; pl_nn = A.anchM[g];
            if (HYP) pl_nl = A.anchM2[g];
            const int64_t am = (int64_t)gG + 1 - A.G.w;                  // the lowest candidate any row of the group takes
            pl_a = am > 0 ? (int32_t)am : 0;
        }
    }

    if (A.pz && lane < nact && pl_fin != 2 && ((uint32_t)pl_B > (uint32_t)n || (uint32_t)pl_a > (uint32_t)n)) {
        atomicAdd(A.pz, 1);
        pl_B = pl_B < 0 ? 0 : (pl_B > n ? (int32_t)n : pl_B); pl_a = pl_a < 0 ? 0 : (pl_a > pl_B ? pl_B : pl_a);
    }
    // (the last group of the matrix has no row (g+1)*64 whose round-6 task would have vouched for its ranges -- the row is beyond the
    //  matrix, or it is the last row n itself, whose upper planes are whole-block tasks of round A: no cap there)
    // (plane 6: the rectangle IS the group -- its bounds are the head's round-A winner and the block start, at most 64 candidates)
    if (lane < nact && pl_fin != 2 && pl_b != 255 && !(pl_fin == 1) && hiG < n && pl_B - pl_a >= (pl_b == LEAF_T ? LEAF_G : A.lcap)) { *A.err = 1; pl_fin = 2; }

    // ---- stream the group's entries once: right-part counts of every outer plane, local link entries
    int32_t cnt[NP], cnt2[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) { cnt[j] = 0; if (HYP) cnt2[j] = 0; }
    int32_t nloc = 0, nloc2 = 0;
    int32_t thr[NP];                                                     // the planes' thresholds on the scalar side (the counters past nact are never read)
#pragma unroll
    for (int j = 0; j < NP; j++) thr[j] = rdl(pl_B, j);
    {
        // 256 entries per step as four coalesced loads per array, the next step's issued before this one's are counted
        int32_t pv[4], nx[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const int32_t q = q0 + 64 * k + lane; pv[k] = q < q1 ? A.prev[q] : INT32_MAX; nx[k] = q < q1 ? A.next[q] : INT32_MAX; }
        // the head candidate of every plane (lane j <-> plane j), fetched for all planes at once behind the first entries: a
        // dependent load per plane inside the plane loop would cost a memory latency each
        if (lane < nact && pl_fin != 2) pl_U = cadd(A.W[pl_B], dm_apply_affine(M, (TC)0, (int64_t)(-pl_B), (int64_t)(-A.pos[pl_B]), (int64_t)0, (int64_t)0));
        for (int32_t base0 = q0; base0 < q1; base0 += 256) {
            int32_t cpv[4], cnx[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { cpv[k] = pv[k]; cnx[k] = nx[k]; }
            if (base0 + 256 < q1) {
#pragma unroll
                for (int k = 0; k < 4; k++) { const int32_t q = base0 + 256 + 64 * k + lane; pv[k] = q < q1 ? A.prev[q] : INT32_MAX; nx[k] = q < q1 ? A.next[q] : INT32_MAX; }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int32_t base = base0 + 64 * k, q = base + lane;
                if (base < q1) {                                         // (wave-uniform)
                const uint64_t lm = leaf_lowmask(posr - base);           // the entries of the columns < r in this step
                if (!(CP_LEAF_SKIP & 1)) leaf_count<NP, false>(cnt, thr, nact, cpv[k], lm);
                const bool loc = q < q1 && cnx[k] < hiG;                 // the row comes back inside the group
                const uint64_t ml = __ballot(loc);
                if (ml) {
                    const int32_t idx = nloc + (int32_t)__popcll(ml & leaf_lowmask(lane));
                    if (loc && idx < LEAF_LIST) s_list[0][idx] = (uint16_t)(((A.col[q] - gG) << 8) | (cnx[k] - gG));
                    nloc += (int32_t)__popcll(ml);
                }
                }
            }
        }
        if (HYP) {
            // rows bucketed by LAST column: right steps of the self nets (first >= B)
            for (int32_t base = l0; base < l1; base += 64) {
                const int32_t q = base + lane;
                const int32_t lf = q < l1 ? A.lfirst[q] : INT32_MIN;
                const uint64_t lm = leaf_lowmask(lposr - base);
                leaf_count<NP, true>(cnt2, thr, nact, lf, lm);
            }
            // rows bucketed by FIRST column whose last column lies inside the group: the local self nets
            for (int32_t base = f0; base < f1; base += 64) {
                const int32_t q = base + lane;
                const int32_t fl = q < f1 ? A.flast[q] : INT32_MAX;
                const bool loc = q < f1 && fl < hiG;
                const uint64_t ml = __ballot(loc);
                if (ml) {
                    const int32_t idx = nloc2 + (int32_t)__popcll(ml & leaf_lowmask(lane));
                    if (loc && idx < LEAF_LIST) s_list[HYP ? 1 : 0][idx] = (uint16_t)(((A.ffirst[q] - gG) << 8) | (fl - gG));
                    nloc2 += (int32_t)__popcll(ml);
                }
            }
        }
    }
    __threadfence_block();                                               // (the local lists are read below)

    // ---- the diagonal and the inner planes: p = r, r - 1, .., gG
    // cost(p, r) = [W[p] - p b_v - pos[p] b_p] + [alpha + r b_v + pos[r] b_p] + the net terms: the first bracket once per column
    // (this lane's own column gG + lane), the second once per row
    TC bv = cadd(Wr, dm_apply_affine(M, alpha, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0));
    int32_t bp = r;
    const TC rowbase = dm_apply_affine(M, alpha, (int64_t)r, (int64_t)posr, (int64_t)0, (int64_t)0);
    const TC colU = cadd(Wr, dm_apply_affine(M, (TC)0, (int64_t)(-r), (int64_t)(-posr), (int64_t)0, (int64_t)0));
    // the net terms split the same way: nets(p, r) = (pos[r] - pos[p]) - (local repeats), self nets = (local)
    const TC colN = cadd(colU, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(-posr), (int64_t)0));
    const TC rowN = cadd(rowbase, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)posr, (int64_t)0));
    if (CP_LEAF_SKIP & 8) {
    } else if (nloc == 0 && nloc2 == 0 && !A.planes) {
        // no row of the group comes back inside it (the usual case away from bands): cost(p, r) = colN(p) + rowN(r), so the
        // winner of row r is the RIGHTMOST minimum of colN over the columns gG .. r - 1: one wave prefix-min scan
        TC sv = colN; int32_t si = lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const TC pvv = shfl_up64(sv, o);
            const int32_t pi = __shfl_up(si, o);
            const bool take = lane >= o && pvv < sv;                     // ties keep the later (larger) column
            sv = take ? pvv : sv; si = take ? pi : si;
        }
        const TC ev = shfl_up64(sv, 1);                                  // exclusive: the columns strictly below the row
        const int32_t ei = __shfl_up(si, 1);
        if (lane >= 1) {
            const TC v = cadd(ev, rowN);
            if (v < bv) { bv = v; bp = gG + ei; }
        }
    } else if (!A.planes && nloc + nloc2 <= LEAF_FEW) {
        // a FEW rows come back inside the group (a third of the groups of a SuiteSparse-shaped pattern, one or two entries each):
        //   cost(p, r) = colN(p) + rowN(r) - k_N #{e : c_e >= p, next_e < r} + k_L #{rows e : first_e >= p, last_e < r}
        // -- the correction is constant between two entry columns.  One SEGMENTED prefix-min scan of colN with a segment starting
        // right of every entry column, then every row combines the minima of the segments below it, each with its own correction:
        // a few dozen instructions per entry instead of a 64-step loop over the columns.
        uint64_t bmask = 0;                                              // columns holding an entry (local index 0 .. 63)
        for (int i = 0; i < nloc; i++) bmask |= 1ull << (__builtin_amdgcn_readfirstlane((int32_t)s_list[0][i]) >> 8);
        if (HYP) for (int i = 0; i < nloc2; i++) bmask |= 1ull << (__builtin_amdgcn_readfirstlane((int32_t)s_list[HYP ? 1 : 0][i]) >> 8);
        const uint64_t heads = (bmask << 1) | 1ull;                       // segment starts: lane 0 and the lane right of every entry column
        const int dist = lane - (63 - __clzll((unsigned long long)(heads & leaf_lowmask(lane + 1))));      // lanes since the segment start
        TC sv = colN; int32_t si = lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const TC pvv = shfl_up64(sv, o);
            const int32_t pi = __shfl_up(si, o);
            const bool take = o <= dist && pvv < sv;                     // (inside the segment; ties keep the later column)
            sv = take ? pvv : sv; si = take ? pi : si;
        }
        const TC ev = shfl_up64(sv, 1);                                  // the (partial) segment ending at column r - 1: no entry of it is counted by row r
        const int32_t ei = __shfl_up(si, 1);
        if (lane >= 1) {
            const TC v = cadd(ev, rowN);
            if (v < bv) { bv = v; bp = gG + ei; }
        }
        int32_t Dn = 0, Dl = 0;                                          // entries at or right of the current boundary that this row counts
        for (uint64_t m = bmask; m;) {
            const int b = 63 - __clzll((unsigned long long)m);            // entry columns from the right
            m ^= 1ull << b;
            for (int i = 0; i < nloc; i++) { const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[0][i]); if ((e >> 8) == b) Dn += ((e & 255) < lane); }
            if (HYP) for (int i = 0; i < nloc2; i++) { const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[HYP ? 1 : 0][i]); if ((e >> 8) == b) Dl += ((e & 255) < lane); }
            const TC sb = rdl64u(sv, b);                                 // minimum of the segment ending at column b
            const int32_t ib = rdl(si, b);
            if (b <= lane - 2) {
                const TC v = cadd(cadd(sb, rowN), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(-Dn), (int64_t)Dl));
                if (v < bv) { bv = v; bp = gG + ib; }
            }
        }
    } else {
        const bool listed = nloc <= LEAF_LIST, listed2 = !HYP || nloc2 <= LEAF_LIST;
        int32_t cur = nloc, cur2 = nloc2, cl = 0, cl2 = 0;
        TC kv = (TC)0; int32_t kp = -1, knn = 0, knl = 0;                 // winner of the current block (block tables only)
        const int jtop = gE - gG - 1;                                    // last existing column of the group
        for (int jc = jtop; jc >= 0; jc--) {
            // column gG + jc joins the parts ending before the rows above it
            if (listed) {
                while (cur > 0) {
                    const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[0][cur - 1]);
                    if ((e >> 8) != jc) break;
                    cl += ((e & 255) < lane);
                    cur--;
                }
            } else {
                const int32_t a0 = rdl(posr, jc), a1 = jc + 1 < 64 ? rdl(posr, jc + 1) : q1;
                for (int32_t qq = a0; qq < a1; qq++) cl += (A.next[qq] < r);
            }
            if (HYP) {
                if (listed2) {
                    while (cur2 > 0) {
                        const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[HYP ? 1 : 0][cur2 - 1]);
                        if ((e >> 8) != jc) break;
                        cl2 += ((e & 255) < lane);
                        cur2--;
                    }
                } else {
                    const int32_t a0 = rdl(fposr, jc), a1 = jc + 1 < 64 ? rdl(fposr, jc + 1) : f1;
                    for (int32_t qq = a0; qq < a1; qq++) cl2 += (A.flast[qq] < r);
                }
            }
            const TC Up = rdl64u(colN, jc);
            if (lane > jc) {
                const TC v = cadd(cadd(Up, rowN), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(-cl), (int64_t)cl2));
                if (v < bv) { bv = v; bp = gG + jc; }
                if (A.planes) {
                    const int b = 31 - __clz(lane ^ jc);                 // the block of row `lane` holding column jc
                    const int low = jc & ((1 << b) - 1);
                    if (low == (1 << b) - 1 || v < kv) { kv = v; kp = gG + jc; knn = posr - rdl(posr, jc) - cl; knl = cl2; }
                    if (low == 0 && rvalid) {
                        const int64_t sw = (int64_t)b * n1 + slot;
                        A.opt[sw] = kp; A.nnopt[sw] = knn;
                        if (HYP) A.nlopt[sw] = knl;
                    }
                }
            }
        }
    }

    // ---- the outer planes.  The planes are visited out of order (the one-candidate planes first, straight from the counter
    // registers), so ties are broken explicitly: the smaller value, then the LARGER p -- what "lower planes first, strict <" gives.
    uint32_t general = 0;                                                // planes with several candidates, or finished by a gap pass
#pragma unroll
    for (int j0 = 0; j0 < NP; j0 += 3) {
        if (j0 < nact) {                                                 // (scalar)
#pragma unroll
            for (int j = j0; j < j0 + 3; j++) {
                if (j < NP && j < nact) {
                    const int32_t B = rdl(pl_B, j), a = rdl(pl_a, j), fl = rdl(pl_fin, j);
                    if (fl == 2) continue;                               // (no block of this plane for the group)
                    if (fl || a != B || rdl(pl_b, j) == 255) { general |= 1u << j; continue; }
                    if (CP_LEAF_SKIP & 4) continue;
                    // one candidate (the winners of the two bounding rows coincide): nothing to stream, nothing to reduce
                    const int32_t nn = rdl(pl_nn, j) + cnt[j], nl = HYP ? rdl(pl_nl, j) + cnt2[j] : 0;
                    const TC v = cadd(cadd(rdl64u(pl_U, j), rowbase), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)nn, (int64_t)nl));
                    if (v < bv || (v == bv && B > bp)) { bv = v; bp = B; }
                    if (A.planes && rvalid) {
                        const int64_t sw = (int64_t)rdl(pl_b, j) * n1 + slot;
                        A.opt[sw] = B; A.nnopt[sw] = nn;
                        if (HYP) A.nlopt[sw] = nl;
                    }
                }
            }
        }
    }
    if (CP_LEAF_SKIP & 2) general = 0;
    for (; general; general &= general - 1) {
        const int j = __ffs(general) - 1;
        const int b = rdl(pl_b, j);
        const int32_t B = rdl(pl_B, j), a = rdl(pl_a, j), nn0 = rdl(pl_nn, j), nl0 = HYP ? rdl(pl_nl, j) : 0;
        const int64_t sw = (int64_t)b * n1 + slot;
        if (rdl(pl_fin, j)) {
            // finished by a gap pass of a round above: the winner is in the planes
            if (CP_LEAF_SKIP & 16) continue;
            if (rvalid) {
                int32_t p = A.opt[sw];
                const int32_t nn = A.nnopt[sw], nl = HYP ? A.nlopt[sw] : 0;
                if (A.pz && (uint32_t)p > (uint32_t)n) { atomicAdd(A.pz, 1); p = r; }
                const TC v = cadd(A.W[p], dm_apply_affine(M, alpha, (int64_t)(r - p), (int64_t)(posr - A.pos[p]), (int64_t)nn, (int64_t)nl));
                if (v < bv || (v == bv && p > bp)) { bv = v; bp = p; }
            }
            continue;
        }
        if ((CP_LEAF_SKIP & 32) && b != LEAF_T) continue;
        if ((CP_LEAF_SKIP & 64) && b == LEAF_T) continue;
        // the right-part counts of this plane again (the counter registers are indexed at compile time: one more pass over the
        // group's entries -- a few dozen cache-resident loads -- is cheaper than parking every plane's counts in LDS for all groups)
        // (the planes 0 and 1 -- in a windowed layer plane 6 and the pseudo-plane, which every group walks -- keep theirs)
        int32_t R = 0, R2 = 0;
        if (j == 0) { R = cnt[0]; R2 = HYP ? cnt2[0] : 0; }
        else if (j == 1 && NP > 1) { R = cnt[1]; R2 = HYP ? cnt2[1] : 0; }
        else {
            for (int32_t base = q0; base < q1; base += 64) {
                const int32_t q = base + lane;
                const int32_t v = q < q1 ? A.prev[q] : INT32_MAX;
                R += (int32_t)__popcll(__ballot(v < B) & leaf_lowmask(posr - base));
            }
            if (HYP) {
                for (int32_t base = l0; base < l1; base += 64) {
                    const int32_t q = base + lane;
                    const int32_t v = q < l1 ? A.lfirst[q] : INT32_MIN;
                    R2 += (int32_t)__popcll(__ballot(v >= B) & leaf_lowmask(lposr - base));
                }
            }
        }
        if (b == 255) {
            // ---- the inner mirrored blocks: candidates i = 0 .. Lm - 1 <-> p = B - i, the head a real candidate; row `lane` takes
            // i <= 62 - lane
            const int32_t Lm = B + 1 < 62 ? B + 1 : 62;
            const bool cv = lane < Lm;
            const int32_t p = cv ? B - lane : B - (Lm - 1);
            const TC Wp = A.W[p];
            const int32_t pp = A.pos[p], pp1 = A.pos[p + 1];
            int32_t fp = 0, fp1 = 0;
            if (HYP) { fp = A.fpos[p]; fp1 = A.fpos[p + 1]; }
            int32_t C = 0, C2 = 0;
            bool specm = false;
            {
                int32_t tot = 0;
                specm = leaf_suffix<false>(A.next, rdl(pp, Lm - 1), rdl(pp, 0), pp, gG, hiG, lane, C, tot);
                if (HYP) specm |= leaf_suffix<true>(A.flast, rdl(fp, Lm - 1), rdl(fp, 0), fp, gG, hiG, lane, C2, tot);
            }
            const int32_t klim = 62 - lane < Lm - 1 ? 62 - lane : Lm - 1;          // last candidate index of this lane's row
            if (!specm) {
                // inclusive prefix-min over the candidates (ties keep the earlier = larger p), then every row reads its own prefix
                TC U = cadd(Wp, dm_apply_affine(M, (TC)0, (int64_t)(-p), (int64_t)(-pp), (int64_t)C, (int64_t)C2));
                int32_t iu = lane;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const TC Uo = shfl_up64(U, o);
                    const int32_t io = __shfl_up(iu, o), Co = __shfl_up(C, o), C2o = HYP ? __shfl_up(C2, o) : 0;
                    const bool take = lane >= o && Uo <= U;
                    U = take ? Uo : U; iu = take ? io : iu; C = take ? Co : C; C2 = take ? C2o : C2;
                }
                const int src = klim >= 0 ? klim : 0;
                const TC Um = shfl64(U, src);
                const int32_t im = __shfl(iu, src), Cm = __shfl(C, src), C2m = HYP ? __shfl(C2, src) : 0;
                if (lane >= 1 && klim >= 0) {
                    const int32_t nn = nn0 + R + Cm, nl = nl0 + R2 + C2m;
                    const TC v = cadd(cadd(Um, rowbase), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(nn0 + R), (int64_t)(nl0 + R2)));
                    const int32_t pw = B - im;
                    (void)nn; (void)nl;
                    if (v < bv || (v == bv && pw > bp)) { bv = v; bp = pw; }
                }
            } else {
                int32_t cr = 0, cr2 = 0;
                for (int t = 0; t < Lm; t++) {
                    const int32_t pc = B - t;
                    if (t >= 1) {
                        const int32_t a0 = rdl(pp, t), a1 = rdl(pp1, t);
                        for (int32_t base = a0; base < a1; base += 64) {
                            const int32_t x = base + lane < a1 ? A.next[base + lane] : 0;
                            const int m = a1 - base < 64 ? a1 - base : 64;
                            for (int u = 0; u < m; u++) cr += (rdl(x, u) >= r);
                        }
                        if (HYP) {
                            const int32_t b0 = rdl(fp, t), b1 = rdl(fp1, t);
                            for (int32_t base = b0; base < b1; base += 64) {
                                const int32_t x = base + lane < b1 ? A.flast[base + lane] : 0;
                                const int m = b1 - base < 64 ? b1 - base : 64;
                                for (int u = 0; u < m; u++) cr2 += (rdl(x, u) < r);
                            }
                        }
                    }
                    const TC Wc = rdl64u(Wp, t);
                    const int32_t posc = rdl(pp, t);
                    const TC v = cadd(Wc, dm_apply_affine(M, alpha, (int64_t)(r - pc), (int64_t)(posr - posc), (int64_t)(nn0 + R + cr), (int64_t)(nl0 + R2 + cr2)));
                    if (lane >= 1 && t <= klim && (v < bv || (v == bv && pc > bp))) { bv = v; bp = pc; }
                }
            }
            continue;
        }
        const int32_t L = B - a + 1;
        TC pv_v = (TC)0; int32_t pv_p = -1, pv_nn = 0, pv_nl = 0;          // this row's winner in the plane
        bool spec = false, few_done = false;
        {
            // candidates 64 at a time (lane <-> candidate p = B - i); the part of the cost that does not depend on the row
            TC Ub = (TC)0; int32_t ib = -1, Cb = 0, Cb2 = 0;
            int32_t carry = 0, carry2 = 0;
            for (int32_t c0 = 0; c0 < L && !spec; c0 += 64) {
                const int32_t i = c0 + lane;
                const bool cv = i < L;
                const int32_t p = cv ? B - i : a;
                const TC Wp = A.W[p];
                const int32_t pp = A.pos[p];
                int32_t C = 0, C2 = 0;
                if (L > 1) {
                    // entries of the stepped columns of this chunk: [pos[last candidate], pos[first stepped column + 1])
                    const int nl_ = L - c0 < 64 ? L - c0 : 64;
                    const int32_t e_lo = rdl(pp, nl_ - 1), e_hi = c0 == 0 ? rdl(pp, 0) : A.pos[B - c0 + 1];
                    int32_t tot = 0;
                    spec |= leaf_suffix<false>(A.next, e_lo, e_hi, pp, gG, hiG, lane, C, tot);
                    C += carry; carry += tot;
                    int32_t fp = 0, g_lo = 0, g_hi = 0;
                    if (HYP) {
                        fp = A.fpos[p];
                        g_lo = rdl(fp, nl_ - 1); g_hi = c0 == 0 ? rdl(fp, 0) : A.fpos[B - c0 + 1];
                        int32_t tot2 = 0;
                        spec |= leaf_suffix<true>(A.flast, g_lo, g_hi, fp, gG, hiG, lane, C2, tot2);
                        C2 += carry2; carry2 += tot2;
                    }
                    if (spec && c0 == 0 && L <= 64 && !(CP_LEAF_SKIP & 128)) {
                        // A FEW specials among at most 64 candidates -- plane 6 of every second group walks the 64 columns in front of
                        // the group, and one group in four meets an entry that comes back inside it (half of this kernel's time went
                        // into their row-by-row walks).  The rows' counts differ only by the specials they have passed:
                        //   cost(p_i, r) = U(i) + rowpart(r) + k_N #{e : i_e <= i, next_e >= r} + k_L #{e' : i_e' <= i, last_e' < r}
                        // -- constant between two special columns.  One segmented prefix-min scan of U over the candidates (a segment
                        // starts at candidate 0 and at every special's column), then every row combines the segment minima in walking
                        // order, each with the specials passed so far: a few dozen instructions per special instead of a walk.
                        const int ns = leaf_specials<false>(A.next, e_lo, e_hi, pp, cv, gG, hiG, lane, s_list[0]);
                        const int ns2 = HYP ? leaf_specials<true>(A.flast, g_lo, g_hi, fp, cv, gG, hiG, lane, s_list[HYP ? 1 : 0]) : 0;
                        __threadfence_block();
                        if (ns + ns2 <= LEAF_FEW) {
                            uint64_t heads = 1ull;
                            for (int k = 0; k < ns; k++) heads |= 1ull << (__builtin_amdgcn_readfirstlane((int32_t)s_list[0][k]) >> 8);
                            if (HYP) for (int k = 0; k < ns2; k++) heads |= 1ull << (__builtin_amdgcn_readfirstlane((int32_t)s_list[HYP ? 1 : 0][k]) >> 8);
                            const int dist = lane - (63 - __clzll((unsigned long long)(heads & leaf_lowmask(lane + 1))));      // lanes since the segment start
                            TC sv = cadd(Wp, dm_apply_affine(M, (TC)0, (int64_t)(-p), (int64_t)(-pp), (int64_t)C, (int64_t)C2));
                            int32_t si = lane, sC = C, sC2 = C2;
#pragma unroll
                            for (int o = 1; o < 64; o <<= 1) {
                                const TC pvv = shfl_up64(sv, o);
                                const int32_t pi = __shfl_up(si, o), pc = __shfl_up(sC, o), pc2 = HYP ? __shfl_up(sC2, o) : 0;
                                const bool take = o <= dist && pvv <= sv;                // (inside the segment; ties keep the earlier candidate = larger p)
                                sv = take ? pvv : sv; si = take ? pi : si; sC = take ? pc : sC; sC2 = take ? pc2 : sC2;
                            }
                            int32_t cn = 0, cl = 0;                                      // specials passed so far that this row counts
                            for (uint64_t m = heads; m;) {
                                const int h = __ffsll((unsigned long long)m) - 1;
                                m &= m - 1;
                                int send = m ? __ffsll((unsigned long long)m) - 1 : L;
                                if (send > L) send = L;
                                send -= 1;                                               // last candidate of the segment
                                if (h > 0) {
                                    for (int k = 0; k < ns; k++) { const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[0][k]); if ((e >> 8) == h) cn += (gG + (e & 255) >= r); }
                                    if (HYP) for (int k = 0; k < ns2; k++) { const int32_t e = __builtin_amdgcn_readfirstlane((int32_t)s_list[HYP ? 1 : 0][k]); if ((e >> 8) == h) cl += (gG + (e & 255) < r); }
                                }
                                if (h >= L) break;                                       // (cannot happen: a special's column is a candidate)
                                const TC Us = rdl64u(sv, send);
                                const int32_t is_ = rdl(si, send), Cs = rdl(sC, send), C2s = HYP ? rdl(sC2, send) : 0;
                                const TC v = cadd(cadd(Us, rowbase), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(nn0 + R + cn), (int64_t)(nl0 + R2 + cl)));
                                if (pv_p < 0 || v < pv_v) { pv_v = v; pv_p = B - is_; pv_nn = nn0 + R + Cs + cn; pv_nl = nl0 + R2 + C2s + cl; }
                            }
                            spec = false; few_done = true;
                        }
                    }
                    if (spec || few_done) break;
                }
                TC U = cadd(Wp, dm_apply_affine(M, (TC)0, (int64_t)(-p), (int64_t)(-pp), (int64_t)C, (int64_t)C2));
                int32_t iu = cv ? i : INT32_MAX;
                if (L - c0 > 1) {
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {                    // wave arg-min; ties -> the smaller i (larger p)
                        const TC Uo = shfl64(U, lane ^ o);
                        const int32_t io = __shfl(iu, lane ^ o), Co = __shfl(C, lane ^ o), C2o = HYP ? __shfl(C2, lane ^ o) : 0;
                        const bool take = io != INT32_MAX && (iu == INT32_MAX || Uo < U || (Uo == U && io < iu));
                        U = take ? Uo : U; iu = take ? io : iu; C = take ? Co : C; C2 = take ? C2o : C2;
                    }
                } else {
                    U = rdl64u(U, 0); iu = c0; C = rdl(C, 0); C2 = HYP ? rdl(C2, 0) : 0;
                }
                if (ib < 0 || U < Ub) { Ub = U; ib = iu; Cb = C; Cb2 = C2; }
            }
            if (!spec && !few_done) {
                pv_nn = nn0 + R + Cb; pv_nl = nl0 + R2 + Cb2; pv_p = B - ib;
                pv_v = cadd(cadd(Ub, rowbase), dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(nn0 + R), (int64_t)(nl0 + R2)));
            }
        }
        if (spec) {
            // some link entries of the candidate columns end inside the group: every row-lane walks the candidates itself
            int32_t cr = 0, cr2 = 0;
            for (int32_t c0 = 0; c0 < L; c0 += 64) {
                const int32_t i = c0 + lane;
                const int32_t p = i < L ? B - i : a;
                const TC Wp = A.W[p];
                const int32_t pp = A.pos[p], pp1 = A.pos[p + 1];
                int32_t fp = 0, fp1 = 0;
                if (HYP) { fp = A.fpos[p]; fp1 = A.fpos[p + 1]; }
                const int nl_ = L - c0 < 64 ? L - c0 : 64;
                for (int t = 0; t < nl_; t++) {
                    const int32_t pc = B - c0 - t;
                    if (c0 + t >= 1) {                                   // step over column pc
                        const int32_t a0 = rdl(pp, t), a1 = rdl(pp1, t);
                        for (int32_t base = a0; base < a1; base += 64) {
                            const int32_t x = base + lane < a1 ? A.next[base + lane] : 0;
                            const int m = a1 - base < 64 ? a1 - base : 64;
                            for (int u = 0; u < m; u++) cr += (rdl(x, u) >= r);
                        }
                        if (HYP) {
                            const int32_t b0 = rdl(fp, t), b1 = rdl(fp1, t);
                            for (int32_t base = b0; base < b1; base += 64) {
                                const int32_t x = base + lane < b1 ? A.flast[base + lane] : 0;
                                const int m = b1 - base < 64 ? b1 - base : 64;
                                for (int u = 0; u < m; u++) cr2 += (rdl(x, u) < r);
                            }
                        }
                    }
                    const TC Wc = rdl64u(Wp, t);
                    const int32_t posc = rdl(pp, t);
                    const int32_t nn = nn0 + R + cr, nl = nl0 + R2 + cr2;
                    const TC v = cadd(Wc, dm_apply_affine(M, alpha, (int64_t)(r - pc), (int64_t)(posr - posc), (int64_t)nn, (int64_t)nl));
                    if (pv_p < 0 || v < pv_v) { pv_v = v; pv_p = pc; pv_nn = nn; pv_nl = nl; }
                }
            }
        }
        if (pv_v < bv || (pv_v == bv && pv_p > bp)) { bv = pv_v; bp = pv_p; }
        if (A.planes && rvalid) {
            A.opt[sw] = pv_p; A.nnopt[sw] = pv_nn;
            if (HYP) A.nlopt[sw] = pv_nl;
        }
    }
    if (rvalid && r >= A.c0 && r <= A.c1) { A.cst[r] = bv; A.ptr[r] = bp; }
}


// ------------------------------------------------------------------ combine the per-bit winners of every row
// Which row a thread of the combine kernels takes.  lvl = 0: row rlo + i.  lvl = 1 (an experiment kept behind a debug option, see
// run_layer): the row of plane slot i -- the order the planes are stored in (prow); row 0 is thread n.  Returns -1 for a thread
// without a row.
__device__ __forceinline__ int64_t combine_row(int64_t i, int64_t n, int64_t rlo, int64_t rhi, int lvl)
{
    int64_t r;
    if (!lvl) r = rlo + i;
    else if (i == n) r = 0;
    else if (i > n) return -1;
    else {
        int t = 0;
        while (t < 62 && n - (n >> (t + 1)) <= i) t++;             // level of slot i: base(t) <= i < base(t + 1), base(t) = n - (n >> t)
        r = (((i - (n - (n >> t))) << 1) | 1) << t;
    }
    return (r < rlo || r > rhi) ? -1 : r;
}

template <typename TC>
__global__ void __launch_bounds__(256) k_combine(int lvl, int64_t n, int64_t rlo, int64_t rhi, int nbits, const int32_t *__restrict__ pos,
                                                 const int32_t *__restrict__ opt, const int32_t *__restrict__ nnopt,
                                                 const int32_t *__restrict__ nlopt,
                                                 const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                 TC *__restrict__ cst, int32_t *__restrict__ ptr, int sh, int32_t *__restrict__ pz)
{
    // sh > 0 (after a leaf pass): the rows (rlo + i) << sh only -- the leaf rows were combined where they were computed
    int64_t r = combine_row((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n, rlo, rhi, lvl);
    if (r < 0) return;
    r <<= sh;
    int64_t n1 = n + 1;
    TC bv = cadd(W[r], dm_apply_affine(M, alpha, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0));   // j = j' (empty part)
    int64_t bp = r;
    for (int b = 0; b < nbits; b++) {
        if (!((r >> b) & 1)) continue;
        int64_t p = opt[(int64_t)b * n1 + prow((r), n1 - 1)];
        if (pz && (uint64_t)p > (uint64_t)n) { atomicAdd(pz, 1); p = r; }      // (poison mode: a cell nobody wrote)
        int64_t nn = nnopt[(int64_t)b * n1 + prow((r), n1 - 1)];
        int64_t nl = nlopt ? nlopt[(int64_t)b * n1 + prow((r), n1 - 1)] : 0;
        TC v = cadd(W[p], dm_apply_affine(M, alpha, r - p, (int64_t)(pos[r] - pos[p]), nn, nl));
        if (v < bv) { bv = v; bp = p; }            // lower bits hold larger p: strict < keeps the largest p on ties
    }
    cst[r] = bv;
    ptr[r] = (int32_t)bp;
}

// windowed layers: the candidates of row r from the right: the diagonal, the standard planes by ascending bit, the common plane,
// the mirrored planes by descending bit -- strict < while moving left keeps the largest p on ties
template <typename TC>
__global__ void __launch_bounds__(256) k_combine_win(int lvl, Geo G, int64_t n, int64_t rlo, int64_t rhi, const int32_t *__restrict__ pos,
                                                     const int32_t *__restrict__ opt, const int32_t *__restrict__ nnopt,
                                                     const int32_t *__restrict__ nlopt,
                                                     const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                     TC *__restrict__ cst, int32_t *__restrict__ ptr, int sh, int32_t *__restrict__ pz)
{
    int64_t r = combine_row((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n, rlo, rhi, lvl);
    if (r < 0) return;
    r <<= sh;                                                   // (after a leaf pass: the multiples of 64 only)
    const int64_t n1 = n + 1;
    TC bv = cadd(W[r], dm_apply_affine(M, alpha, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0));   // j = j' (empty part)
    int64_t bp = r;
    if (r >= 1) {
        const int64_t slot = prow((r), n1 - 1);
        for (int i = 0; i <= 2 * G.s; i++) {
            const int b = i <= G.s ? i : 2 * G.s - i;                       // 0 .. s, then s-1 .. 0
            if (b < G.s && (((r >> b) & 1) != (i <= G.s))) continue;      // first pass: set bits (standard); second pass: clear bits (mirrored)
            if (b == G.s && i != G.s) continue;
            int64_t cs, ce;
            if (!geo_block(G, r, b, cs, ce)) continue;
            int64_t p = opt[(int64_t)b * n1 + slot];
            if (pz && (uint64_t)p > (uint64_t)n) { atomicAdd(pz, 1); p = r; }
            const int64_t nn = nnopt[(int64_t)b * n1 + slot];
            const int64_t nl = nlopt ? nlopt[(int64_t)b * n1 + slot] : 0;
            const TC v = cadd(W[p], dm_apply_affine(M, alpha, r - p, (int64_t)(pos[r] - pos[p]), nn, nl));
            if (v < bv) { bv = v; bp = p; }
        }
    }
    cst[r] = bv;
    ptr[r] = (int32_t)bp;
}

// ------------------------------------------------------------------ host side
// every row that is not a multiple of 64: inner planes, outer planes and the combine in one pass
template <typename TC, bool HYP>
void leaf_pass(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    const int64_t n = C.n;
    const Geo &G = C.G;
    const int64_t c0 = C.rlo > 1 ? C.rlo : 1, c1 = C.rhi < n ? C.rhi : n;
    if (c1 < c0) return;
    const int64_t g0 = c0 >> LEAF_T, g1 = c1 >> LEAF_T;
    // bytes: the group's link entries twice (prev, next), column pointers, previous-layer costs, the two output rows
    ProfScope ps(PROF_LEAF, s, (8.0 * (C.avg_deg + C.self_deg) + 4.0 + 8.0 + 12.0) * (double)((g1 - g0 + 1) << LEAF_T));
    const int need = G.win ? G.s - LEAF_T + 2 : C.nbits - LEAF_T;           // outer planes a group can have (+ the pseudo-plane)
    CP_REQUIRE(need <= 25, CP_EINTERNAL, "leaf pass: more outer planes than counters");
    // With a gap pass in round 6 every task of that round with gap_min candidates or more has finished its rows (and the
    // ranges of a leaf group in a plane b > 6 lie inside the range of the round-6 task of one of its two bounding rows): a longer
    // range in a leaf group can only come from plane cells a mispredicted speculative layer never wrote (zeros after
    // allocation: a range of millions of candidates per group, seconds of work for a layer that is redone anyway).  Such a
    // group flags the layer (err) and skips the plane.
    const int32_t lcap = (C.gaps && g_opt_gap_tau >= LEAF_T) ? (int32_t)std::max<int64_t>(g_opt_gap_min, 2) : INT32_MAX;
    LeafArgs<TC, HYP> L{};
    L.n = n; L.g0 = g0; L.ngroups = g1 - g0 + 1; L.c0 = c0; L.c1 = c1; L.nbits = C.nbits; L.planes = (int32_t)(g_opt_block_tables != 0);
    L.pos = A->pos32.p; L.prev = A->prev.p; L.next = A->next.p; L.col = A->col.p;
    L.fpos = if_hyp<HYP>(A->fpos32.p); L.flast = if_hyp<HYP>(A->flast.p); L.ffirst = if_hyp<HYP>(A->ffirst.p);
    L.lpos = if_hyp<HYP>(A->lpos32.p); L.lfirst = if_hyp<HYP>(A->lfirst.p);
    L.opt = Wk.pl.opt.p; L.nnopt = Wk.pl.nnopt.p; L.nlopt = if_hyp<HYP>(Wk.pl.nlopt.p); L.fin = Wk.pl.fin.p; L.fin_stamp = Wk.pl.fin_stamp;
    L.W = C.W; L.M = C.M; L.alpha = C.alpha; L.cst = C.cst_out; L.ptr = C.ptr_out; L.G = G;
    L.anchM = Wk.win.leaf_anch.p; L.anchM2 = if_hyp<HYP>(Wk.win.leaf_anch2.p); L.lcap = lcap; L.err = &Wk.sp.rc.p->err; L.pz = C.pzp;
    constexpr int WPB = LeafWPB<HYP>::v;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(need <= 18 ? k_leaf<TC, HYP, 18> : k_leaf<TC, HYP, 25>), dim3((unsigned)cdiv(L.ngroups, WPB)), dim3(64 * WPB), 0, s, L);
    CP_HIP(hipGetLastError());
}

// The rows left: with the leaf pass the multiples of 64 (their planes from LEAF_T up), without it every row.  Threads in row
// order.  (lvl = 1, DBG_COMBINE_BY_SLOT: in plane-slot order, so that the dozen plane reads of a row are contiguous across a
// wave -- measured 867 us against 650 us at config 3: the 2 x 12 gathers W[p], pos[p] of a row are what counts, and they are
// neighbours only for neighbouring rows.)
template <typename TC, bool HYP>
void combine_rows(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    const int64_t n = C.n;
    const bool leaf = C.leaf;
    ProfScope ps(PROF_COMBINE, s, 24.0 * (double)(leaf ? (n >> LEAF_T) + 1 : n + 1));
    const int64_t c0 = C.rlo > 0 ? C.rlo : 0, c1 = C.rhi < n ? C.rhi : n;
    const int64_t r0 = leaf ? (c0 + LEAF_G - 1) >> LEAF_T : c0, r1 = leaf ? c1 >> LEAF_T : c1;       // leaf: the multiples of 64 in [c0, c1]
    const int lvl = (!leaf && (g_opt_dbg & DBG_COMBINE_BY_SLOT)) ? (2 * (c1 - c0 + 1) >= n + 1) : 0;
    const int sh = leaf ? LEAF_T : 0;
    const int32_t *nl = if_hyp<HYP>(Wk.pl.nlopt.p);
    if (c1 >= c0 && r1 >= r0) {
        const unsigned cgrid = (unsigned)cdiv(lvl ? n + 1 : r1 - r0 + 1, 256);
        if (C.G.win) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_combine_win<TC>), dim3(cgrid), dim3(256), 0, s, lvl, C.G, n, r0, r1, A->pos32.p, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, C.W, C.M,
                                        C.alpha, C.cst_out, C.ptr_out, sh, C.pzp);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_combine<TC>), dim3(cgrid), dim3(256), 0, s, lvl, n, r0, r1, C.nbits, A->pos32.p, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, C.W, C.M, C.alpha,
                                C.cst_out, C.ptr_out, sh, C.pzp);
    }
}

#define CP_INST(TC, HYP) \
    template void leaf_pass<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &); \
    template void combine_rows<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &);
CP_INST(int64_t, false) CP_INST(int64_t, true) CP_INST(double, false) CP_INST(double, true)
#undef CP_INST

}  // namespace cpk
