// dp_total_gap.hip -- the GAP PASSES of a round of the total-cost DP layer (scheme: dp_total.hip): behind k_lpass_own<GAP>
// (dp_total_own.hip) every row of a task's gap gets its winner in one pass over the gap's tiles (k_gap_finish; tasks of more than
// GAPSEG tiles: k_gap_seg, k_gap_merge).
#include "dp_total.hpp"

namespace cpk {

// ------------------------------------------------------------------ gap passes
// The arg-min staircase of a rectangle jumps: between two neighbouring rows rL < rR of a round the winners B = opt[rL] and
// a = opt[rR] can lie thousands of columns apart, and the divide and conquer re-scans that gap [a, B] once per level below.
// In the rounds tau <= gap_tau a task with such a gap instead finishes EVERY row r' of (rL, hi), hi = min(rR, rectangle end,
// n + 1), in one pass over the gap: each of them has its (rightmost) winner inside [a, B].
//   nets(p, r') = nets(B, rL) + #{q in cols [rL, r') : prev[q] < B} + #{q in cols [p, B) : next[q] >= r'}
// and the last term is the same for all these rows except for the entries with rL < next[q] < hi - 1 ("special": counted by
// some rows only).  k_lpass_own<GAP> streams the gap once with the common threshold and flags the tiles holding specials; here
// one wave per (task, 64 rows) gives every lane a row and walks the task's tiles in candidate order: a plain tile contributes
// its winner (the same for all rows: their values differ by a row-only term plus cum(r') = the specials passed so far that
// the row counts); a flagged tile is re-walked entry by entry with every lane counting for its own row.  Ties: strict <
// in walking order = the larger p wins, as everywhere.  The rows are marked final (fin): later rounds skip them.
template <bool GE>
__device__ __forceinline__ int32_t gap_right_counts(const int32_t *__restrict__ cpos, const int32_t *__restrict__ arr, int32_t rL, int ck, int32_t thr,
                                                    int32_t n, int lane)
{
    // #{entries of columns [rL, r') passing the test}, r' = rL + 1 + 64 ck + lane.  Coalesced: the columns of the earlier row
    // chunks are summed by the whole wave; the wave's own 64 columns are one contiguous run of entries, flagged 64 at a time,
    // and every lane counts the flags in front of the end of its column.
    int32_t cfirst = rL + 64 * ck;
    if (cfirst > n) cfirst = n;
    int32_t c = 0;
    for (int32_t q = cpos[rL] + lane, q1 = cpos[cfirst]; q < q1; q += 64) { int32_t v = arr[q]; c += GE ? (v >= thr) : (v < thr); }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    int32_t jn = cfirst + lane + 1, cl = cfirst + 64;
    if (jn > n) jn = n;
    if (cl > n) cl = n;
    const int32_t myend = cpos[jn], e0 = cpos[cfirst], e1 = cpos[cl];
    int32_t mine = 0;
    for (int32_t base = e0; base < e1; base += 256) {       // four loads in flight
        bool fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int32_t q = base + 64 * j + lane;
            fl[j] = false;
            if (q < e1) { int32_t v = arr[q]; fl[j] = GE ? (v >= thr) : (v < thr); }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned long long m = __ballot(fl[j]);
            int32_t w = myend - (base + 64 * j);
            if (w > 0) mine += __popcll(w >= 64 ? m : (m & ((1ull << w) - 1ull)));
        }
    }
    return c + mine;
}

template <typename TC, bool HYP>
struct GapCtx {
    const Best<TC, HYP> *part, *sub; const int32_t *spv; const uint8_t *spec;
    const int64_t *tilePS, *tilePS2;
    const int32_t *pos, *next, *fpos, *flast;
    const TC *W;
    int blk;                    // the tile geometry (own_tile_geo)
};

// the tiles [ka, kz) of a task (first tile k0, head B, L steps, row r) walked for NR x 64 rows of the wave (lane l holds the rows
// rr[0 .. NR-1], one per 64-row chunk: the tile records are fetched once for all of them): the winners so far (bv, bp, bl, bl2)
// and the specials the rows count so far (cum, cum2) are carried in and out
// SLOW = false: the entry-by-entry walk of a tile with more than SMAX specials is compiled out (its column-pointer and cost
// registers cost the kernels two waves per SIMD, and they wait on memory three quarters of their time): such an item returns false
// and is redone by the SLOW variant of its kernel.
template <typename TC, bool HYP, int NR, bool SLOW>
__device__ __forceinline__ bool gap_walk(const GapCtx<TC, HYP> &C, const DevModel<TC> &M, TC alpha, int64_t ka, int64_t kz, int64_t k0,
                                         int32_t B, int32_t L, int32_t r, int32_t posr, const int32_t (&rr)[NR], const int32_t (&rcmp)[NR],
                                         const bool (&valid)[NR], int lane,
                                         TC (&bv)[NR], int32_t (&bp)[NR], int32_t (&bl)[NR], int32_t (&bl2)[NR], int32_t (&cum)[NR], int32_t (&cum2)[NR])
{
    const int64_t ps0 = C.tilePS[k0], ps20 = HYP ? C.tilePS2[k0] : 0;
    for (int64_t kb = ka; kb < kz; kb += 64) {
    const int64_t km = kb + lane < kz ? kb + lane : kz - 1;
    const int32_t m_base = (int32_t)(C.tilePS[km] - ps0), m_base2 = HYP ? (int32_t)(C.tilePS2[km] - ps20) : 0;
    const int m_ns = C.spec[km];
    Best<TC, HYP> m_part; best_clear(m_part);
    if (m_ns == 0) m_part = C.part[km];
    const int nb = (int)(kz - kb < 64 ? kz - kb : 64);
    // the segment records of the NEXT tile are fetched while the current tile is walked (the walk is a chain of dependent loads)
    Best<TC, HYP> nx_c; best_clear(nx_c);
    int32_t nx_sv = 0;
    {
        const int ns0 = rdl(m_ns, 0);
        if (ns0 > 0 && ns0 <= SMAX) { if (lane <= ns0) nx_c = C.sub[kb * (SMAX + 1) + lane]; if (lane < ns0) nx_sv = C.spv[kb * (SMAX + 1) + lane]; }
    }
    for (int i = 0; i < nb; i++) {
        const int64_t k = kb + i;
        const int32_t base = rdl(m_base, i), base2 = HYP ? rdl(m_base2, i) : 0;
        const int ns = rdl(m_ns, i);
        const Best<TC, HYP> cur_c = nx_c;
        const int32_t cur_sv = nx_sv;
        if (i + 1 < nb) {
            const int ns1 = rdl(m_ns, i + 1);
            if (ns1 > 0 && ns1 <= SMAX) { if (lane <= ns1) nx_c = C.sub[(k + 1) * (SMAX + 1) + lane]; if (lane < ns1) nx_sv = C.spv[(k + 1) * (SMAX + 1) + lane]; }
        }
        if (ns <= SMAX) {
            // plain tile: one winner; tile with ns specials: ns + 1 segment winners, a special between two segments
            Best<TC, HYP> c = cur_c;
            int32_t sv = cur_sv;
            if (ns == 0) {
                best_clear(c);
                c.v = rdl64(m_part.v, i); c.p = rdl(m_part.p, i); c.nn = rdl(m_part.nn, i);
                if (HYP) best_set_nl(c, rdl(best_nl(m_part), i));
            }
            for (int sg = 0; sg <= ns; sg++) {
                Best<TC, HYP> d = c;
                if (ns) { d.v = rdl64(c.v, sg); d.p = rdl(c.p, sg); d.nn = rdl(c.nn, sg); if (HYP) best_set_nl(d, rdl(best_nl(c), sg)); }
                if (d.p >= 0) {
#pragma unroll
                    for (int u = 0; u < NR; u++) {
                        int32_t lc = d.nn + base + cum[u], lc2 = HYP ? best_nl(d) + base2 + cum2[u] : 0;
                        TC v = cadd(d.v, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)(base + cum[u]), (int64_t)(base2 + cum2[u])));
                        if (bp[u] < 0 || v < bv[u]) { bv[u] = v; bp[u] = d.p; bl[u] = lc; bl2[u] = lc2; }
                    }
                }
                if (sg < ns) {                          // the candidates from here on have this special on their right
                    const int32_t s1 = rdl(sv, sg), val = s1 & 0x7fffffff;
                    const bool first_list = s1 >= 0;        // (two unconditional adds: an if / else here becomes ONE add through a selected address, i.e. scratch)
#pragma unroll
                    for (int u = 0; u < NR; u++) {
                        cum[u] += (first_list && val >= rcmp[u]);
                        cum2[u] += (!first_list && valid[u] && val < rr[u]);
                    }
                }
            }
            continue;
        }
        // too many specials: every lane counts for its own rows, entry by entry
        if (!SLOW) return false;
        if (SLOW) {
        const int head = k == k0 ? 1 : 0;
        int32_t pf, tlk;
        own_tile_geo(C.blk, B, L, (int32_t)(k - k0), pf, tlk);
        // C.pos[pf + 1 - j] and C.W[pf - j] of the tile's columns are fetched lane-strided; the entries come through 64-entry
        // windows (one coalesced load each) and are handed to all lanes one at a time
#define CP_SEL5(a_, i_) ((i_) < 64 ? a_[0] : (i_) < 128 ? a_[1] : (i_) < 192 ? a_[2] : (i_) < 256 ? a_[3] : a_[4])
        int32_t pk[5], pk2[5] = {0, 0, 0, 0, 0}; TC wk[4];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            int32_t e = lane + 64 * j;
            pk[j] = e <= tlk + 1 ? C.pos[pf + 1 - e] : 0;
            if (HYP) pk2[j] = e <= tlk + 1 ? C.fpos[pf + 1 - e] : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) { int32_t e = lane + 64 * j; wk[j] = e <= tlk ? C.W[pf - e] : (TC)0; }
        int32_t run[NR], run2[NR];
#pragma unroll
        for (int u = 0; u < NR; u++) { run[u] = 0; run2[u] = 0; }
        int32_t wb = INT32_MAX, reg = 0, wb2 = INT32_MAX, reg2 = 0;
        for (int32_t e = 0; e <= tlk; e++) {
            const int32_t p = pf - e, e1 = e + 1;
            const int32_t en = __shfl(CP_SEL5(pk, e), e & 63), st = __shfl(CP_SEL5(pk, e1), e1 & 63);      // C.pos[p + 1], C.pos[p]
            if (!(head && e == 0)) {                    // step over column p (the head element steps over nothing)
                for (int32_t q = en - 1; q >= st; q--) {
                    if (q < wb || q - wb > 63) { wb = q - 63; reg = wb + lane >= 0 ? C.next[wb + lane] : 0; }
                    const int32_t x = __shfl(reg, q - wb);           // (every lane takes part: no short-circuit around a shuffle)
#pragma unroll
                    for (int u = 0; u < NR; u++) run[u] += (x >= rcmp[u]);
                }
                if (HYP) {
                    const int32_t en2 = __shfl(CP_SEL5(pk2, e), e & 63), st2 = __shfl(CP_SEL5(pk2, e1), e1 & 63);
                    for (int32_t q = en2 - 1; q >= st2; q--) {
                        if (q < wb2 || q - wb2 > 63) { wb2 = q - 63; reg2 = wb2 + lane >= 0 ? C.flast[wb2 + lane] : 0; }
                        const int32_t x = __shfl(reg2, q - wb2);
#pragma unroll
                        for (int u = 0; u < NR; u++) run2[u] += (valid[u] && x < rr[u]);
                    }
                }
            }
            const TC wp = shfl64(e < 64 ? wk[0] : e < 128 ? wk[1] : e < 192 ? wk[2] : wk[3], e & 63);
#pragma unroll
            for (int u = 0; u < NR; u++) {
                int32_t lc = base + cum[u] + run[u], lc2 = base2 + cum2[u] + run2[u];
                TC v = cadd(wp, dm_apply_affine(M, alpha, (int64_t)(r - p), (int64_t)(posr - st), (int64_t)lc, (int64_t)lc2));      // (the task's row: the rows' values differ by a row-only term)
                if (bp[u] < 0 || v < bv[u]) { bv[u] = v; bp[u] = p; bl[u] = lc; bl2[u] = lc2; }
            }
        }
#undef CP_SEL5
        // from here on the rows also count the specials of this tile they passed
#pragma unroll
        for (int u = 0; u < NR; u++) {
            cum[u] += run[u] - (int32_t)(C.tilePS[k + 1] - C.tilePS[k]);
            if (HYP) cum2[u] += run2[u] - (int32_t)(C.tilePS2[k + 1] - C.tilePS2[k]);
        }
        }
    }
    }
    return true;
}

// rows of the wave, right parts and anchors of a gap task: shared by the kernels below
struct GapRows { int32_t rL, hi, rr, rcmp; bool valid, none; };
__device__ __forceinline__ GapRows gap_rows(int tau, int ck, int32_t r, int b, int64_t n, int lane)
{
    GapRows g;
    g.rL = r - (1 << tau);
    int64_t hi64 = (int64_t)r + ((int64_t)1 << tau), re = ((((int64_t)r >> b) + 1) << b);
    if (hi64 > re) hi64 = re;
    if (hi64 > n + 1) hi64 = n + 1;
    g.hi = (int32_t)hi64;
    g.rr = g.rL + 1 + 64 * ck + lane;                       // this lane's row
    g.none = g.rL + 1 + 64 * ck >= g.hi;                    // (wave-uniform: the chunk lies beyond the gap's rows)
    g.valid = g.rr < g.hi;
    g.rcmp = g.valid ? g.rr : INT32_MAX;                    // an invalid lane counts nothing
    return g;
}

template <typename TC, bool HYP>
struct GapSegRec { TC v; int32_t p, l, l2, cum, cum2, _pad; };

// NR: 64-row chunks per wave (a lane holds one row of each): the task's records -- descriptor, tile winners, segment lists -- are
// fetched once for NR x 64 rows.  The kernel waits on memory three quarters of its time at four waves per SIMD (profiles/
// r03_pmc_gap_finish.txt), i.e. it is bound by the number of (task, rows) items times the dependent loads of one item.
template <typename TC, bool HYP, int NR, bool SLOW>
__global__ void __launch_bounds__(256, 4) k_gap_finish(int tau, int nchunk, RoundCounts *__restrict__ rc, int64_t n,
                                                    const int64_t *__restrict__ toffs, GapCtx<TC, HYP> C,
                                                    const int4 *__restrict__ tdesc, const uint8_t *__restrict__ tb, const int32_t *__restrict__ rlen,
                                                    const int32_t *__restrict__ prev, const int32_t *__restrict__ lpos, const int32_t *__restrict__ lfirst,
                                                    DevModel<TC> M, TC alpha,
                                                    int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt, uint8_t *__restrict__ fin,
                                                    int2 *__restrict__ glist, int2 *__restrict__ gslot, int fin_stamp, int32_t *__restrict__ slow)
{
    // SLOW: the items the fast variant listed in `slow` (rc->n_gslow of them)
    const int lane = threadIdx.x & 63;
    const int nitem = (nchunk + NR - 1) / NR;
    const int64_t nwork = SLOW ? (int64_t)rc->n_gslow : (int64_t)rc->nown * nitem, n1 = n + 1;
    for (int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wi < nwork; wi += (int64_t)gridDim.x * 4) {
        const int64_t w = SLOW ? (int64_t)slow[wi] : wi;
        const int64_t t = w / nitem;
        const int ck0 = (int)(w - t * nitem) * NR;
        const int64_t k0 = toffs[t], k1 = toffs[t + 1];
        if (k1 - k0 > GAPSEG) {                             // (wave-uniform) a long task: listed for k_gap_seg / k_gap_merge
            if (!SLOW && ck0 == 0 && lane == 0) {
                int nseg = (int)((k1 - k0 + GAPSEG - 1) / GAPSEG);
                int idx = atomicAdd(&rc->n_glong, 1), slot0 = atomicAdd(&rc->n_gslots, nseg);
                glist[idx] = make_int2((int)t, slot0);
                for (int j = 0; j < nseg; j++) gslot[slot0 + j] = make_int2((int)t, j);       // slot -> (task, segment) for k_gap_seg
            }
            continue;
        }
        const int4 td = tdesc[t];                           // {B, anchor + right part of the task's own row, row r, pos[r]}
        const int b = tb[t];
        const int32_t B = td.x, r = td.z, posr = td.w, L = rlen[t];
        GapRows g[NR];
        int32_t rr[NR], rcmp[NR]; bool valid[NR];
#pragma unroll
        for (int u = 0; u < NR; u++) { g[u] = gap_rows(tau, ck0 + u, r, b, n, lane); rr[u] = g[u].rr; rcmp[u] = g[u].rcmp; valid[u] = g[u].valid; }
        if (g[0].none) continue;
        // right parts of the rows and the anchor (counts at (B, rL))
        int32_t Rr[NR], Rr2[NR];
#pragma unroll
        for (int u = 0; u < NR; u++) {
            Rr[u] = 0; Rr2[u] = 0;
            if (u == 0 || !g[u].none) {                     // (wave-uniform)
                Rr[u] = gap_right_counts<false>(C.pos, prev, g[0].rL, ck0 + u, B, (int32_t)n, lane);
                if (HYP) Rr2[u] = gap_right_counts<true>(lpos, lfirst, g[0].rL, ck0 + u, B, (int32_t)n, lane);
            }
        }
        const int64_t rwL = (int64_t)b * n1 + prow(((int64_t)g[0].rL), n1 - 1);
        const int32_t anchor = nnopt[rwL], anchor2 = HYP ? nlopt[rwL] : 0;
        TC bv[NR]; int32_t bp[NR], bl[NR], bl2[NR], cum[NR], cum2[NR];
#pragma unroll
        for (int u = 0; u < NR; u++) { bv[u] = (TC)0; bp[u] = -1; bl[u] = 0; bl2[u] = 0; cum[u] = 0; cum2[u] = 0; }
        if (!gap_walk<TC, HYP, NR, SLOW>(C, M, alpha, k0, k1, k0, B, L, r, posr, rr, rcmp, valid, lane, bv, bp, bl, bl2, cum, cum2)) {
            if (lane == 0) slow[atomicAdd(&rc->n_gslow, 1)] = (int32_t)w;
            continue;
        }
#pragma unroll
        for (int u = 0; u < NR; u++) {
            if (valid[u]) {
                int64_t rw = (int64_t)b * n1 + prow(((int64_t)rr[u]), n1 - 1);
                opt[rw] = bp[u]; nnopt[rw] = anchor + Rr[u] + bl[u];
                if (HYP) nlopt[rw] = anchor2 + Rr2[u] + bl2[u];
                fin[rw] = (uint8_t)fin_stamp;
            }
        }
    }
}

// long gap tasks, phase 1: one wave per (segment slot = GAPSEG tiles of a listed task, 64 rows) walks its tiles as if nothing lay
// in front of them
template <typename TC, bool HYP, bool SLOW>
__global__ void __launch_bounds__(256) k_gap_seg(int tau, int nchunk, RoundCounts *__restrict__ rc, int64_t n, const int64_t *__restrict__ toffs,
                                                 GapCtx<TC, HYP> C, const int4 *__restrict__ tdesc, const uint8_t *__restrict__ tb,
                                                 const int32_t *__restrict__ rlen, DevModel<TC> M, TC alpha, const int2 *__restrict__ gslot,
                                                 GapSegRec<TC, HYP> *__restrict__ gseg, int32_t *__restrict__ slow)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwork = SLOW ? (int64_t)rc->n_sslow : (int64_t)rc->n_gslots * nchunk;
    for (int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wi < nwork; wi += (int64_t)gridDim.x * 4) {
        const int64_t w = SLOW ? (int64_t)slow[wi] : wi;
        const int64_t slot = w / nchunk;
        const int ck = (int)(w - slot * nchunk);
        const int2 se = gslot[slot];
        const int64_t t = se.x, k0 = toffs[t], k1 = toffs[t + 1];
        const int sg = se.y;
        const int4 td = tdesc[t];
        const GapRows g = gap_rows(tau, ck, td.z, tb[t], n, lane);
        if (g.none) continue;
        TC bv[1] = {(TC)0}; int32_t bp[1] = {-1}, bl[1] = {0}, bl2[1] = {0}, cum[1] = {0}, cum2[1] = {0};
        const int32_t rr1[1] = {g.rr}, rcmp1[1] = {g.rcmp}; const bool valid1[1] = {g.valid};
        const int64_t ka = k0 + (int64_t)sg * GAPSEG, kz = ka + GAPSEG < k1 ? ka + GAPSEG : k1;
        if (!gap_walk<TC, HYP, 1, SLOW>(C, M, alpha, ka, kz, k0, td.x, rlen[t], td.z, td.w, rr1, rcmp1, valid1, lane, bv, bp, bl, bl2, cum, cum2)) {
            if (lane == 0) slow[atomicAdd(&rc->n_sslow, 1)] = (int32_t)w;
            continue;
        }
        GapSegRec<TC, HYP> rec; rec.v = bv[0]; rec.p = bp[0]; rec.l = bl[0]; rec.l2 = bl2[0]; rec.cum = cum[0]; rec.cum2 = cum2[0]; rec._pad = 0;
        gseg[(slot * nchunk + ck) * 64 + lane] = rec;
    }
}

// phase 2: one wave per (listed task, 64 rows) merges the segment winners in walking order, adding the specials of the
// segments in front
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_gap_merge(int tau, int nchunk, const RoundCounts *__restrict__ rc, int64_t n, const int64_t *__restrict__ toffs,
                                                   const int4 *__restrict__ tdesc, const uint8_t *__restrict__ tb,
                                                   const int32_t *__restrict__ pos, const int32_t *__restrict__ prev, const int32_t *__restrict__ lpos,
                                                   const int32_t *__restrict__ lfirst, DevModel<TC> M, const int2 *__restrict__ glist,
                                                   const GapSegRec<TC, HYP> *__restrict__ gseg,
                                                   int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt, uint8_t *__restrict__ fin, int fin_stamp)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwork = (int64_t)rc->n_glong * nchunk, n1 = n + 1;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwork; w += (int64_t)gridDim.x * 4) {
        const int i = (int)(w / nchunk), ck = (int)(w - (int64_t)i * nchunk);
        const int2 le = glist[i];
        const int64_t t = le.x, k0 = toffs[t], k1 = toffs[t + 1];
        const int nseg = (int)((k1 - k0 + GAPSEG - 1) / GAPSEG);
        const int4 td = tdesc[t];
        const int b = tb[t];
        const GapRows g = gap_rows(tau, ck, td.z, b, n, lane);
        if (g.none) continue;
        const int32_t Rr = gap_right_counts<false>(pos, prev, g.rL, ck, td.x, (int32_t)n, lane);
        const int32_t Rr2 = HYP ? gap_right_counts<true>(lpos, lfirst, g.rL, ck, td.x, (int32_t)n, lane) : 0;
        const int64_t rwL = (int64_t)b * n1 + prow(((int64_t)g.rL), n1 - 1);
        const int32_t anchor = nnopt[rwL], anchor2 = HYP ? nlopt[rwL] : 0;
        TC bv = (TC)0; int32_t bp = -1, bl = 0, bl2 = 0, cum = 0, cum2 = 0;
        // (the task over the top rectangle's whole block has thousands of segments: eight records per lane in flight -- the running
        //  counts make the merge sequential, the loads need not be)
        for (int s0 = 0; s0 < nseg; s0 += 8) {
            GapSegRec<TC, HYP> rr[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (s0 + u < nseg) rr[u] = gseg[((int64_t)(le.y + s0 + u) * nchunk + ck) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (s0 + u >= nseg) break;
                const GapSegRec<TC, HYP> rec = rr[u];
                if (rec.p >= 0) {
                    TC v = cadd(rec.v, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, (int64_t)cum, (int64_t)cum2));
                    if (bp < 0 || v < bv) { bv = v; bp = rec.p; bl = rec.l + cum; bl2 = rec.l2 + cum2; }
                }
                cum += rec.cum; cum2 += rec.cum2;
            }
        }
        if (g.valid) {
            int64_t rw = (int64_t)b * n1 + prow(((int64_t)g.rr), n1 - 1);
            opt[rw] = bp; nnopt[rw] = anchor + Rr + bl;
            if (HYP) nlopt[rw] = anchor2 + Rr2 + bl2;
            fin[rw] = (uint8_t)fin_stamp;
        }
    }
}

// the gap round's finishing kernels: fast variants first, then the SLOW ones over what they listed
template <typename TC, bool HYP>
static void launch_gap(hipStream_t s, cp_csr_s *A, LayerWork<TC> &Wk, int tau, int nchunk, int gnr, RoundCounts *rc, int64_t n, const TC *W,
                       const DevModel<TC> &M, TC alpha, unsigned gg, unsigned gs_grid, unsigned gm, unsigned gslow_grid, int blk)
{
    GapCtx<TC, HYP> C{recs<HYP>(Wk.ow.o_part), recs<HYP>(Wk.ow.o_sub), Wk.ow.o_spv.p, Wk.ow.o_spec.p, Wk.ow.o_tilePS.p, if_hyp<HYP>(Wk.ow.o_tilePS2.p), A->pos32.p, A->next.p,
                      if_hyp<HYP>(A->fpos32.p), if_hyp<HYP>(A->flast.p), W, blk};
    auto *gs = reinterpret_cast<GapSegRec<TC, HYP> *>(Wk.gp.g_seg.p);      // (sized for the larger record, like the Best buffers)
    const int32_t *lp = if_hyp<HYP>(A->lpos32.p), *lf = if_hyp<HYP>(A->lfirst.p);
    int32_t *nl = if_hyp<HYP>(Wk.pl.nlopt.p);
#define GF_ARGS tau, nchunk, rc, n, Wk.ow.o_toffs.p, C, Wk.ow.o_tdesc.p, Wk.ow.o_tb.p, Wk.ow.o_rlen.p, A->prev.p, lp, lf, M, alpha, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, Wk.pl.fin.p, \
                Wk.gp.g_list.p, Wk.gp.g_slot.p, Wk.pl.fin_stamp, Wk.gp.g_slow.p
    if (gnr == 2) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_finish<TC, HYP, 2, false>), dim3(gg), dim3(256), 0, s, GF_ARGS);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_finish<TC, HYP, 2, true>), dim3(gslow_grid), dim3(256), 0, s, GF_ARGS);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_finish<TC, HYP, 1, false>), dim3(gg), dim3(256), 0, s, GF_ARGS);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_finish<TC, HYP, 1, true>), dim3(gslow_grid), dim3(256), 0, s, GF_ARGS);
    }
#undef GF_ARGS
#define GS_ARGS tau, nchunk, rc, n, Wk.ow.o_toffs.p, C, Wk.ow.o_tdesc.p, Wk.ow.o_tb.p, Wk.ow.o_rlen.p, M, alpha, Wk.gp.g_slot.p, gs, Wk.gp.g_sslow.p
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_seg<TC, HYP, false>), dim3(gs_grid), dim3(256), 0, s, GS_ARGS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_seg<TC, HYP, true>), dim3(gslow_grid), dim3(256), 0, s, GS_ARGS);
#undef GS_ARGS
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gap_merge<TC, HYP>), dim3(gm), dim3(256), 0, s, tau, nchunk, rc, n, Wk.ow.o_toffs.p, Wk.ow.o_tdesc.p, Wk.ow.o_tb.p, A->pos32.p, A->prev.p,
                       lp, lf, M, Wk.gp.g_list.p, gs, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, Wk.pl.fin.p, Wk.pl.fin_stamp);
}

// The tail of the own-tile chain in a gap round: the tiles' prefix, then every row of the gaps gets its winner
template <typename TC, bool HYP>
void gap_finish(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P)
{
    hipStream_t s = C.s;
    const int64_t gown = C.spec ? grow_pred(P.nown) : P.nown;
    {
        // the gap kernels look a tile's prefix up at random: a device-wide scan of the tile counts.  (The other rounds need
        // sums inside one task only: k_fix_own makes them from o_tileS.)
        ProfScope ps(PROF_CARRY, s, 12.0 * (double)P.NT);
        const int32_t *ntp = reinterpret_cast<const int32_t *>(&rc->NT);       // (NT < 2^31: the low word)
        exclusive_scan_i32_lb(Wk.ow.o_tileS.p, Wk.ow.o_tilePS.p, ntp, (int64_t)Wk.ow.o_tileS.n, nullptr, Wk.sc.scanws, s);
        if (HYP) exclusive_scan_i32_lb(Wk.ow.o_tileS2.p, Wk.ow.o_tilePS2.p, ntp, (int64_t)Wk.ow.o_tileS.n, nullptr, Wk.sc.scanws, s);
    }
    // every row of the gaps gets its winner: one wave per (task, 64 rows); tasks of more than GAPSEG tiles in two steps
    ProfScope ps(PROF_GAP, s, 24.0 * (double)P.NT);
    const int nchunk = (int)std::max<int64_t>(1, ((int64_t)2 << R.tau) / 64);
    const size_t ncap = Wk.ow.o_rec.n / GAPSEG + 2;
    Wk.gp.g_list.ensure(ncap); Wk.gp.g_slot.ensure(2 * ncap);
    Wk.gp.g_seg.ensure((2 * ncap) * (size_t)nchunk * 64 * sizeof(GapSegRec<TC, true>));
    // items that meet a tile with more than SMAX specials are listed by the fast kernels and redone by the SLOW ones
    Wk.gp.g_slow.ensure((size_t)gown * (size_t)nchunk + 64); Wk.gp.g_sslow.ensure((2 * ncap) * (size_t)nchunk + 64);
    CP_REQUIRE((int64_t)gown * nchunk < INT32_MAX && (int64_t)(2 * ncap) * nchunk < INT32_MAX, CP_EINTERNAL, "gap work index beyond 32 bits");
    const int gnr = (g_opt_gap_nr >= 2 && nchunk >= 2) ? 2 : 1;       // 64-row chunks per wave of k_gap_finish
    unsigned gg = (unsigned)std::min<int64_t>(cdiv(gown * cdiv((int64_t)nchunk, gnr), 4), 16384);
    unsigned gs_grid = (unsigned)std::min<int64_t>(cdiv((int64_t)(2 * ncap) * nchunk, 4), 8192);
    unsigned gm = (unsigned)std::min<int64_t>(cdiv((int64_t)ncap * nchunk, 4), 4096);
    const unsigned gslow_grid = 2048;                               // (grid-stride over the device-side counts n_gslow / n_sslow: usually none)
    launch_gap<TC, HYP>(s, C.A, Wk, R.tau, nchunk, gnr, rc, C.n, C.W, C.M, C.alpha, gg, gs_grid, gm, gslow_grid, C.oblk);
}

#define CP_INST(TC, HYP) \
    template void gap_finish<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, const RoundDesc &, RoundCounts *, const RoundCounts &);
CP_INST(int64_t, false) CP_INST(int64_t, true) CP_INST(double, false) CP_INST(double, true)
#undef CP_INST

}  // namespace cpk
