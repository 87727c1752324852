// lws_rect.hpp -- row minima of W[p] + f(p, r) over rectangles and staircases of (row, candidate) cells, the cells coming from the
// device counters (wavelet rank queries).  The engine of chunk_lws.hip (pack_stripe, DynamicTotalChunker) and of dp_total_budget.hip
// (one layer of the K-part total-cost DP under a work budget); what differs between the two is a policy P:
//
//     P::TC, P::Args                    cost type; the kernel argument block, derived from LwsCounts<TC>
//     P::base(G, p)                     the cost the candidate p starts from (the finished C[p] / the previous layer's W[p])
//     P::cell(G, p, r)                  f(p, r): lws_f over the counters of LwsCounts, or a family's own evaluation (sym_total.hip)
//     P::better(c, p, bc, bp)           does the pair (c, p) replace (bc, bp)?  p < 0: no pair.  Fixes the tie direction
//     P::stair_lo / stair_hi(G, r, j)   the first / last feasible candidate of row r inside a block that starts / ends at column j
//
// Inside a FULL rectangle (every row sees every candidate, jb <= ra) the cost is inverse-Monge for the fast_total_ok models: for
// p1 < p2 <= r1 < r2, submodularity of the net count gives f(p1, r2) + f(p2, r1) <= f(p1, r1) + f(p2, r2).  A smaller column that
// wins or ties at r1 keeps doing so at r2, and one that loses strictly to a smaller column keeps losing: the leftmost and the
// rightmost argmin are both non-INCREASING in r.  So under either tie direction row i of a level searches [opt(i + h), opt(i - h)]
// (k_lws_level, cut into chunks of LWS_CH columns, one wave each; k_lws_fin reduces the chunks).  Small rectangles are scanned
// whole (k_lws_brute), and so are the partial rows of a narrow block (k_lws_stair).
//
// The level kernels take their rows from a level description LV: LwsLevel, one rectangle, or LwsBatch, the rectangles of one depth
// of a column tree together -- pairwise disjoint in rows and in columns, so one launch sequence serves them all (sym_total.hip).
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include "wavelet.hpp"
#include <algorithm>

namespace cpk {

static constexpr int LWS_CH = 256;              // columns per wave in a rectangle level
static constexpr int LWS_LDS_ROWS = 4096;       // levels with at most this many rows find their chunks in LDS
static constexpr int64_t LWS_BRUTE_CELLS = (int64_t)1 << 20, LWS_BRUTE_COLS = 1024, LWS_STAIR_COLS = 1024;

// what every policy's argument block holds
template <typename TC>
struct LwsCounts {
    DevModel<TC> M;
    TC alpha;
    int64_t n;
    int32_t nets, self;
    const int64_t *pos;
    const int64_t *lpos;
    WaveletDev wnet, wself;                      // rank queries
    TC *bc; int32_t *bp;                         // n + 1 : best pair of each row so far
    int32_t *opt;                                // n + 1 : argmin of a row inside the current rectangle
};

template <typename P>
__device__ __forceinline__ void wave_best(typename P::TC &c, int32_t &p)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const typename P::TC oc = __shfl_xor(c, o);
        const int32_t op = __shfl_xor(p, o);
        if (P::better(oc, op, c, p)) { c = oc; p = op; }
    }
}

// f(p, r), columns [p, r): the counts of ocl (seq.hip) for a stateless model
template <typename TC>
__device__ __forceinline__ TC lws_f(const LwsCounts<TC> &G, int64_t p, int64_t r)
{
    const int64_t np = G.pos[r] - G.pos[p];
    int64_t nn = 0, nl = 0;
    if (G.nets) nn = np - wt_count_le(G.wnet, G.n - p, G.pos[r]);
    if (G.self) nl = wt_count_le(G.wself, G.n - p, G.lpos[r]);
    return dm_apply(G.M, G.alpha, r - p, np, nn, nl);
}

// the best pair of row r among the candidates c0 + lane, c0 + lane + 64, ... <= c1 (one wave; every lane returns it)
template <typename P>
__device__ __forceinline__ void lws_scan_row(const typename P::Args &G, int64_t r, int64_t c0, int64_t c1, int lane, typename P::TC &bc, int32_t &bp)
{
    using TC = typename P::TC;
    bc = (TC)0;
    bp = -1;
    for (int64_t p = c0 + lane; p <= c1; p += 64) {
        const TC v = cadd(P::base(G, p), P::cell(G, p, r));
        if (P::better(v, (int32_t)p, bc, bp)) { bc = v; bp = (int32_t)p; }
    }
    wave_best<P>(bc, bp);
}

// ------------------------------------------------------------------ small full rectangle: rows ra + blockIdx.x, columns [ja, jb]
template <typename P>
__global__ void __launch_bounds__(64) k_lws_brute(typename P::Args G, int64_t ja, int64_t jb, int64_t ra)
{
    const int64_t r = ra + blockIdx.x;
    typename P::TC bc;
    int32_t bp;
    lws_scan_row<P>(G, r, ja, jb, threadIdx.x, bc, bp);
    if (threadIdx.x == 0 && P::better(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ partial rows of a narrow block [ja, jb]: block x < m is row ra + x,
// the later blocks are the rows from ra2 on; each row scans its feasible candidates inside the block
// (along a moving bound the full rectangles of the decomposition shrink to single cells: below a column threshold the partial rows
// are scanned whole in one launch instead)
template <typename P>
__global__ void __launch_bounds__(64) k_lws_stair(typename P::Args G, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2)
{
    const int64_t r = (int64_t)blockIdx.x < m ? ra + blockIdx.x : ra2 + ((int64_t)blockIdx.x - m);
    typename P::TC bc;
    int32_t bp;
    lws_scan_row<P>(G, r, P::stair_lo(G, r, ja), P::stair_hi(G, r, jb), threadIdx.x, bc, bp);
    if (threadIdx.x == 0 && P::better(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ large full rectangle: one level of the monotone D&C
// level h (a power of two): rows i = h - 1 + 2 h u < m of the rectangle (row ra + i); rows i - h and i + h were done on coarser levels
struct LwsLevel { int64_t ra, m, ja, jb, h, cnt, cap; };

__device__ __forceinline__ void lws_range(const int32_t *__restrict__ opt, const LwsLevel &L, int64_t u, int64_t &r, int64_t &lo, int64_t &hi)
{
    const int64_t i = L.h - 1 + 2 * L.h * u;
    r = L.ra + i;
    lo = i + L.h < L.m ? (int64_t)opt[r + L.h] : L.ja;
    hi = i >= L.h ? (int64_t)opt[r - L.h] : L.jb;
    if (hi < lo) hi = lo;                        // (cannot happen for an inverse-Monge cost)
}
__device__ __forceinline__ int64_t lws_row(const LwsLevel &L, int64_t u) { return L.ra + L.h - 1 + 2 * L.h * u; }

// the same level of several rectangles: rd[0 .. nr), pre[0 .. nr] the prefix of their row counts on this level (a rectangle with
// m < h has none); level row u belongs to the last rectangle with pre <= u and its opt neighbours stay inside that rectangle
struct LwsRectD { int32_t ra, m, ja, jb; };      // rows ra .. ra + m - 1, candidates [ja, jb]
struct LwsBatch { const LwsRectD *rd; const int32_t *pre; int64_t nr, h, cnt, cap; };

__device__ __forceinline__ int64_t lws_batch_find(const int32_t *__restrict__ pre, int64_t nr, int64_t u)
{
    int64_t a = 0, b = nr - 1;
    while (a < b) { const int64_t mid = (a + b + 1) >> 1; if ((int64_t)pre[mid] <= u) a = mid; else b = mid - 1; }
    return a;
}

__device__ __forceinline__ void lws_range(const int32_t *opt, const LwsBatch &L, int64_t u, int64_t &r, int64_t &lo, int64_t &hi)
{
    const int64_t a = lws_batch_find(L.pre, L.nr, u);
    const LwsRectD R = L.rd[a];
    const int64_t i = L.h - 1 + 2 * L.h * (u - L.pre[a]);
    r = R.ra + i;
    lo = i + L.h < R.m ? (int64_t)opt[r + L.h] : (int64_t)R.ja;
    hi = i >= L.h ? (int64_t)opt[r - L.h] : (int64_t)R.jb;
    if (hi < lo) hi = lo;
}
__device__ __forceinline__ int64_t lws_row(const LwsBatch &L, int64_t u)
{
    const int64_t a = lws_batch_find(L.pre, L.nr, u);
    return L.rd[a].ra + L.h - 1 + 2 * L.h * (u - L.pre[a]);
}

// ... and the small rectangles, or the partial rows, of one depth in one launch: block x is row x of the concatenated descriptors
// (pre[0 .. nr]: the prefix of their m).  A row of a full rectangle sees all of [ja, jb], so stair_lo / stair_hi return ja / jb there
template <typename P>
__global__ void __launch_bounds__(64) k_lws_rows(typename P::Args G, const LwsRectD *__restrict__ rd, const int32_t *__restrict__ pre, int64_t nr)
{
    const int64_t a = lws_batch_find(pre, nr, (int64_t)blockIdx.x);
    const LwsRectD R = rd[a];
    const int64_t r = R.ra + ((int64_t)blockIdx.x - pre[a]);
    typename P::TC bc;
    int32_t bp;
    lws_scan_row<P>(G, r, P::stair_lo(G, r, R.ja), P::stair_hi(G, r, R.jb), threadIdx.x, bc, bp);
    if (threadIdx.x == 0 && P::better(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

template <typename P, typename LV>
__global__ void __launch_bounds__(256) k_lws_count(typename P::Args G, LV L, int32_t *__restrict__ cnt)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= L.cnt) return;
    int64_t r, lo, hi;
    lws_range(G.opt, L, u, r, lo, hi);
    cnt[u] = (int32_t)((hi - lo + LWS_CH) / LWS_CH);
}

// chunk g of the level: binary search of the row in the chunk offsets off[0..cnt] (in LDS for small levels, else from the scan)
template <typename P, typename LV>
__global__ void __launch_bounds__(256) k_lws_level(typename P::Args G, LV L, int64_t *__restrict__ goff, int32_t lds,
                                                   typename P::TC *__restrict__ pc, int32_t *__restrict__ pq)
{
    __shared__ int64_t off[LWS_LDS_ROWS + 1];
    __shared__ int64_t wsum[256];
    const int t = threadIdx.x;
    if (lds) {
        const int64_t per = (L.cnt + 255) / 256, u0 = t * per;
        int64_t sum = 0;
        for (int64_t u = u0; u < u0 + per && u < L.cnt; u++) {
            int64_t r, lo, hi;
            lws_range(G.opt, L, u, r, lo, hi);
            off[u] = sum;
            sum += (hi - lo + LWS_CH) / LWS_CH;
        }
        wsum[t] = sum;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {      // inclusive scan of the thread sums
            const int64_t v = t >= o ? wsum[t - o] : 0;
            __syncthreads();
            wsum[t] += v;
            __syncthreads();
        }
        const int64_t base = t > 0 ? wsum[t - 1] : 0;
        for (int64_t u = u0; u < u0 + per && u < L.cnt; u++) off[u] += base;
        if (t == 255) off[L.cnt] = wsum[255];
        __syncthreads();
        if (blockIdx.x == 0) for (int64_t u = t; u <= L.cnt; u += 256) goff[u] = off[u];
    }
    const int64_t *O = lds ? off : goff;
    const int64_t g = (int64_t)blockIdx.x * 4 + (t >> 6);
    const int64_t total = O[L.cnt];
    if (g >= total || g >= L.cap) return;
    int64_t a = 0, b = L.cnt - 1;                // the last u with off[u] <= g
    while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (O[mid] <= g) a = mid; else b = mid - 1; }
    int64_t r, lo, hi;
    lws_range(G.opt, L, a, r, lo, hi);
    const int64_t c0 = lo + (g - O[a]) * LWS_CH, c1 = std::min<int64_t>(hi, c0 + LWS_CH - 1);
    typename P::TC bc;
    int32_t bp;
    lws_scan_row<P>(G, r, c0, c1, t & 63, bc, bp);
    if ((t & 63) == 0) { pc[g] = bc; pq[g] = bp; }
}

// one thread per level row: its chunks -> opt of the row, merged into its best pair
template <typename P, typename LV>
__global__ void __launch_bounds__(256) k_lws_fin(typename P::Args G, LV L, const int64_t *__restrict__ off, const typename P::TC *__restrict__ pc,
                                                 const int32_t *__restrict__ pq)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= L.cnt) return;
    const int64_t r = lws_row(L, u);
    typename P::TC bc = (typename P::TC)0;
    int32_t bp = -1;
    const int64_t e = std::min<int64_t>(off[u + 1], L.cap);
    for (int64_t g = off[u]; g < e; g++) if (P::better(pc[g], pq[g], bc, bp)) { bc = pc[g]; bp = pq[g]; }
    if (bp < 0) return;
    G.opt[r] = bp;
    if (P::better(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ host: the launches of one rectangle / one set of partial rows
// rows of an m-row rectangle on level h, and a bound on the chunks of cnt level rows over cols columns: the search ranges of
// neighbouring rows share at most their end points
inline int64_t lws_level_rows(int64_t m, int64_t h) { return m < h ? 0 : (m - h + 1 + 2 * h - 1) / (2 * h); }
inline int64_t lws_level_chunks(int64_t cols, int64_t cnt) { return (cols + cnt + LWS_CH - 1) / LWS_CH + cnt; }

template <typename P>
struct LwsRect {
    using TC = typename P::TC;
    hipStream_t s = nullptr;
    typename P::Args G;
    int prof = PROF_LWS;                         // the profile slot every launch is timed in
    int64_t brute_cells = LWS_BRUTE_CELLS, brute_cols = LWS_BRUTE_COLS;      // a rectangle within both is scanned whole
    DBuf<int64_t> off, scratch;
    DBuf<int32_t> cnt32, pq;
    DBuf<TC> pc;
    int64_t cap = 0;

    // scratch for rectangles inside rows / candidates 0 .. n1 - 1
    void reserve(int64_t n1)
    {
        cap = (2 * n1 + LWS_CH - 1) / LWS_CH + n1 + 1;
        pc.ensure((size_t)cap); pq.ensure((size_t)cap);
        off.ensure((size_t)n1 + 1); cnt32.ensure((size_t)n1);
    }

    template <typename F> void launch(F &&f) { ProfScope ps(prof, s, 0.0); f(); }

    void rect(int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        const int64_t m = rb - ra + 1, cols = jb - ja + 1;
        if (cols <= brute_cols && m * cols <= brute_cells) {
            launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_brute<P>), dim3((unsigned)m), dim3(64), 0, s, G, ja, jb, ra); });
            return;
        }
        int64_t h = 1;
        while (2 * h <= m) h *= 2;               // rows h - 1 (+ 2h u) first
        for (; h >= 1; h /= 2) {
            LwsLevel Lv;
            Lv.ra = ra; Lv.m = m; Lv.ja = ja; Lv.jb = jb; Lv.h = h;
            Lv.cnt = lws_level_rows(m, h);
            Lv.cap = std::min<int64_t>(cap, lws_level_chunks(cols, Lv.cnt));
            level(Lv);
        }
    }

    // one level, of one rectangle or of a depth's rectangles: Lv.cnt rows in at most Lv.cap <= cap chunks
    template <typename LV> void level(const LV &Lv)
    {
        const bool lds = Lv.cnt <= LWS_LDS_ROWS;
        if (!lds) {
            launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_count<P, LV>), dim3((unsigned)cdiv(Lv.cnt, 256)), dim3(256), 0, s, G, Lv, cnt32.p); });
            launch([&] { exclusive_scan_i32(cnt32.p, off.p, Lv.cnt, scratch, s); });          // (three kernels, one timed step)
        }
        launch([&] {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_level<P, LV>), dim3((unsigned)cdiv(Lv.cap, 4)), dim3(256), 0, s, G, Lv, off.p, (int32_t)lds,
                               pc.p, pq.p);
        });
        launch([&] {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_fin<P, LV>), dim3((unsigned)cdiv(Lv.cnt, 256)), dim3(256), 0, s, G, Lv, (const int64_t *)off.p,
                               (const TC *)pc.p, (const int32_t *)pq.p);
        });
    }

    // the rows of the descriptors rd[0 .. nr) scanned whole, one launch (pre: the prefix of their row counts, `rows` in all)
    void rows(const LwsRectD *rd, const int32_t *pre, int64_t nr, int64_t rows)
    {
        if (nr <= 0 || rows <= 0) return;
        launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_rows<P>), dim3((unsigned)rows), dim3(64), 0, s, G, rd, pre, nr); });
    }

    // the partial rows [ra, ra + m) and [ra2, ra2 + m2) of the block [ja, jb], one launch
    void stair(int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2 = 0, int64_t m2 = 0)
    {
        if (m + m2 <= 0) return;
        launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_stair<P>), dim3((unsigned)(m + m2)), dim3(64), 0, s, G, ja, jb, ra, m, ra2); });
    }
};

}  // namespace cpk
