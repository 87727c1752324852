// chunk_lws.hip -- pack_stripe(A, DynamicTotalChunker(f | ConstrainedCost(f, w, w_max))) for any width or monotone work budget
// (DynamicChunker.jl:20-56) as an on-line divide and conquer over the columns (the least-weight-subsequence problem).
//
// 0-based rows r = j' - 1 and candidates p = j - 1: C[0] = 0, C[r] = min over p in [lo(r), r - 1] of C[p] + f(p, r), where
// f(p, r) is the cost of columns [p, r) and lo(r) = j0(j') - 1 never decreases.  Every row keeps its best pair (cost, p), reduced
// by LEXICOGRAPHIC minimum: the smallest minimising p whatever order the candidates arrive in -- the reference's strict < while
// scanning j upwards.  solve(x, y): solve(x, mid); push the finished candidates [x, mid] into the rows (mid, y]; solve(mid + 1, y).
//
// A push covers the staircase {(r, p) : p >= lo(r)}, which does NOT keep the monotone argmin, so it is split into full rectangles
// (push): the rows with lo(r) <= ja see all of [ja, jb] -- a prefix of the rows, lo being non-decreasing -- and the rest recurse
// into the two halves of the columns.  Every feasible cell lies in exactly one rectangle.  Inside a full rectangle the cost is
// inverse-Monge for the fast_total_ok models (for p1 < p2 <= jb < r1 < r2, submodularity of the net count gives
// f(p1, r2) + f(p2, r1) <= f(p1, r1) + f(p2, r2)), so a column that wins or ties at r1 keeps doing so at r2: the leftmost argmin
// is non-INCREASING in r and the row minima come from the monotone divide and conquer, run level by level (k_lws_level: row i of
// the level searches [opt(i + h), opt(i - h)], cut into chunks of LWS_CH columns, one wave each; k_lws_fin reduces the chunks).
// Small rectangles are scanned whole (k_lws_brute), and so is the staircase left of a push below LWS_STAIR_COLS columns
// (k_lws_stair).  Rectangle cells come from the device counters (wavelet rank queries).
//
// A leaf of at most 64 * CPT rows runs on one wave, row after row (k_lws_leaf): lane l owns the candidates x + l + 64 k and keeps
// their counts in registers, updated per new column from the link arrays -- nets grow by #{q in column : prev[q] < p}, self nets by
// the rows whose last column is the new one and whose first column is >= p -- so a leaf row costs no rank query.
#include "csr.hpp"
#include "model.hpp"
#include "wavelet.hpp"
#include "weight.hpp"
#include "dp.hpp"
#include <algorithm>

namespace cpk {

int64_t g_opt_lws = 1, g_opt_lws_leaf = 512;

static constexpr int LWS_CH = 256;              // columns per wave in a rectangle level
static constexpr int LWS_LDS_ROWS = 4096;       // levels with at most this many rows find their chunks in LDS
static constexpr int64_t LWS_BRUTE_CELLS = (int64_t)1 << 20, LWS_BRUTE_COLS = 1024, LWS_STAIR_COLS = 1024;

template <typename TC>
struct LwsArgs {
    DevModel<TC> M;
    TC alpha;
    int64_t n;
    int32_t nets, self;
    const int64_t *pos;
    const int32_t *prev;                         // link arrays (leaf rows)
    const int64_t *lpos;
    const int32_t *lfirst;
    WaveletDev wnet, wself;                      // rank queries (rectangles)
    const int32_t *lo;                           // n + 1 : first candidate of each row
    TC *bc; int32_t *bp;                         // n + 1 : best pair pushed into each row so far (bp < 0: none)
    int32_t *opt;                                // n + 1 : leftmost argmin of a row inside the current rectangle
    TC *cst1; int64_t *spl1;                     // the 1-based tables of k_pack_dynamic: cst1[r] = C[r], spl1[r] = p + 1
};

template <typename TC>
__device__ __forceinline__ bool lex_less(TC c, int32_t p, TC bc, int32_t bp)
{
    return p >= 0 && (bp < 0 || c < bc || (c == bc && p < bp));
}

template <typename TC>
__device__ __forceinline__ void wave_lexmin(TC &c, int32_t &p)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const TC oc = __shfl_xor(c, o);
        const int32_t op = __shfl_xor(p, o);
        if (lex_less(oc, op, c, p)) { c = oc; p = op; }
    }
}

// f(p, r), columns [p, r): the counts of ocl (seq.hip) for a stateless model without per-part alpha
template <typename TC>
__device__ __forceinline__ TC lws_f(const LwsArgs<TC> &G, int64_t p, int64_t r)
{
    const int64_t np = G.pos[r] - G.pos[p];
    int64_t nn = 0, nl = 0;
    if (G.nets) nn = np - wt_count_le(G.wnet, G.n - p, G.pos[r]);
    if (G.self) nl = wt_count_le(G.wself, G.n - p, G.lpos[r]);
    return dm_apply(G.M, G.alpha, r - p, np, nn, nl);
}

// ------------------------------------------------------------------ leaf: rows [x, y], candidates inside the leaf, one wave
// Nothing a leaf row reads but the costs of its own candidates depends on the rows before it, so the leaf's column pointers, lower
// bounds, pushed best pairs and (up to the LDS left) link entries are staged in LDS first: the row chain then waits on no HBM load.
template <typename TC, int CPT>
__global__ void __launch_bounds__(64) k_lws_leaf(LwsArgs<TC> G, int64_t x, int64_t y)
{
    constexpr int LR = 64 * CPT;
    constexpr int64_t STAGE = (65536 - (int64_t)LR * (8 + 4 + 4 + 8) - 64) / 4;
    __shared__ int64_t s_pos[LR + 1];
    __shared__ TC s_bc[LR];
    __shared__ int32_t s_lo[LR], s_bp[LR], s_prev[STAGE];
    const int lane = threadIdx.x;
    for (int64_t t = lane; t <= y - x + 1 && x + t <= G.n; t += 64) s_pos[t] = G.pos[x + t];
    for (int64_t t = lane; t <= y - x; t += 64) { s_lo[t] = G.lo[x + t]; s_bc[t] = G.bc[x + t]; s_bp[t] = G.bp[x + t]; }
    const int64_t q0 = G.pos[x], qs = std::min<int64_t>(G.pos[y], q0 + STAGE);
    if (G.nets) for (int64_t q = q0 + lane; q < qs; q += 64) s_prev[q - q0] = G.prev[q];
    __syncthreads();
    int32_t nn[CPT], nl[CPT], pk[CPT];            // (columns < 2^30: the compares of the row loop in 32 bits)
    int64_t pp[CPT];
    TC cc[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const int64_t p = x + lane + 64 * k;
        nn[k] = 0; nl[k] = 0; cc[k] = (TC)0; pk[k] = (int32_t)p;
        pp[k] = s_pos[(p <= y ? p : y) - x];
    }
    {
        const TC c0 = x == 0 ? (TC)0 : s_bc[0];
        const int32_t p0 = x == 0 ? -1 : s_bp[0];
        if (lane == 0) { G.cst1[x] = c0; if (x > 0) G.spl1[x] = (int64_t)p0 + 1; cc[0] = c0; }
    }
    for (int64_t r = x + 1; r <= y; r++) {
        const int64_t c = r - 1;                 // the column that joins every part [p, r)
        if (G.nets) {
            const int64_t q1 = s_pos[c + 1 - x];
            const int32_t c32 = (int32_t)c;
            for (int64_t q = s_pos[c - x]; q < q1; q++) {
                const int32_t pv = q < qs ? s_prev[q - q0] : G.prev[q];
#pragma unroll
                for (int k = 0; k < CPT; k++) nn[k] += (pv < pk[k]) & (pk[k] <= c32);
            }
        }
        if (G.self) {
            const int64_t t1 = G.lpos[c + 1];
            for (int64_t t = G.lpos[c]; t < t1; t++) {
                const int32_t fc = G.lfirst[t];
#pragma unroll
                for (int k = 0; k < CPT; k++) nl[k] += (pk[k] <= fc);
            }
        }
        const int64_t lor = s_lo[r - x], pr = s_pos[r - x];
        TC bc = s_bc[r - x];
        int32_t bp = s_bp[r - x];
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int64_t p = x + lane + 64 * k;
            if (p <= c && p >= lor) {
                const TC v = cadd(cc[k], dm_apply(G.M, G.alpha, r - p, pr - pp[k], (int64_t)nn[k], (int64_t)nl[k]));
                if (lex_less(v, (int32_t)p, bc, bp)) { bc = v; bp = (int32_t)p; }
            }
        }
        wave_lexmin(bc, bp);
        if (lane == 0) { G.cst1[r] = bc; G.spl1[r] = (int64_t)bp + 1; }
        const int64_t d = r - x;
#pragma unroll
        for (int k = 0; k < CPT; k++) if (d == (int64_t)lane + 64 * k) cc[k] = bc;
    }
}

// ------------------------------------------------------------------ small full rectangle: rows ra + blockIdx.x, columns [ja, jb]
template <typename TC>
__global__ void __launch_bounds__(64) k_lws_brute(LwsArgs<TC> G, int64_t ja, int64_t jb, int64_t ra)
{
    const int64_t r = ra + blockIdx.x;
    TC bc = (TC)0;
    int32_t bp = -1;
    for (int64_t p = ja + threadIdx.x; p <= jb; p += 64) {
        const TC v = cadd(G.cst1[p], lws_f(G, p, r));
        if (lex_less(v, (int32_t)p, bc, bp)) { bc = v; bp = (int32_t)p; }
    }
    wave_lexmin(bc, bp);
    if (threadIdx.x == 0 && lex_less(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ small staircase: rows ra + blockIdx.x, columns [max(lo(r), ja), jb]
// (along a moving lower bound the full rectangles of the decomposition shrink to single cells: below LWS_STAIR_COLS columns the
// staircase is scanned whole in one launch instead)
template <typename TC>
__global__ void __launch_bounds__(64) k_lws_stair(LwsArgs<TC> G, int64_t ja, int64_t jb, int64_t ra)
{
    const int64_t r = ra + blockIdx.x;
    const int64_t a = G.lo[r] > ja ? (int64_t)G.lo[r] : ja;
    TC bc = (TC)0;
    int32_t bp = -1;
    for (int64_t p = a + threadIdx.x; p <= jb; p += 64) {
        const TC v = cadd(G.cst1[p], lws_f(G, p, r));
        if (lex_less(v, (int32_t)p, bc, bp)) { bc = v; bp = (int32_t)p; }
    }
    wave_lexmin(bc, bp);
    if (threadIdx.x == 0 && lex_less(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ large full rectangle: one level of the monotone D&C
// level h (a power of two): rows i = h - 1 + 2 h u < m of the rectangle (row ra + i); rows i - h and i + h were done on coarser levels
struct LwsLevel { int64_t ra, m, ja, jb, h, cnt, cap; };

template <typename TC>
__device__ __forceinline__ void lws_range(const LwsArgs<TC> &G, const LwsLevel &L, int64_t u, int64_t &r, int64_t &lo, int64_t &hi)
{
    const int64_t i = L.h - 1 + 2 * L.h * u;
    r = L.ra + i;
    lo = i + L.h < L.m ? (int64_t)G.opt[r + L.h] : L.ja;
    hi = i >= L.h ? (int64_t)G.opt[r - L.h] : L.jb;
    if (hi < lo) hi = lo;                        // (cannot happen for an inverse-Monge cost)
}

template <typename TC>
__global__ void __launch_bounds__(256) k_lws_count(LwsArgs<TC> G, LwsLevel L, int32_t *__restrict__ cnt)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= L.cnt) return;
    int64_t r, lo, hi;
    lws_range(G, L, u, r, lo, hi);
    cnt[u] = (int32_t)((hi - lo + LWS_CH) / LWS_CH);
}

// chunk g of the level: binary search of the row in the chunk offsets off[0..cnt] (in LDS for small levels, else from the scan)
template <typename TC>
__global__ void __launch_bounds__(256) k_lws_level(LwsArgs<TC> G, LwsLevel L, int64_t *__restrict__ goff, int32_t lds,
                                                   TC *__restrict__ pc, int32_t *__restrict__ pq)
{
    __shared__ int64_t off[LWS_LDS_ROWS + 1];
    __shared__ int64_t wsum[256];
    const int t = threadIdx.x;
    if (lds) {
        const int64_t per = (L.cnt + 255) / 256, u0 = t * per;
        int64_t sum = 0;
        for (int64_t u = u0; u < u0 + per && u < L.cnt; u++) {
            int64_t r, lo, hi;
            lws_range(G, L, u, r, lo, hi);
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
    lws_range(G, L, a, r, lo, hi);
    const int64_t c0 = lo + (g - O[a]) * LWS_CH, c1 = std::min<int64_t>(hi, c0 + LWS_CH - 1);
    TC bc = (TC)0;
    int32_t bp = -1;
    for (int64_t p = c0 + (t & 63); p <= c1; p += 64) {
        const TC v = cadd(G.cst1[p], lws_f(G, p, r));
        if (lex_less(v, (int32_t)p, bc, bp)) { bc = v; bp = (int32_t)p; }
    }
    wave_lexmin(bc, bp);
    if ((t & 63) == 0) { pc[g] = bc; pq[g] = bp; }
}

// one thread per level row: the chunks in order -> opt of the row, merged into its best pair
template <typename TC>
__global__ void __launch_bounds__(256) k_lws_fin(LwsArgs<TC> G, LwsLevel L, const int64_t *__restrict__ off, const TC *__restrict__ pc,
                                                 const int32_t *__restrict__ pq)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= L.cnt) return;
    const int64_t r = L.ra + L.h - 1 + 2 * L.h * u;
    TC bc = (TC)0;
    int32_t bp = -1;
    const int64_t e = std::min<int64_t>(off[u + 1], L.cap);
    for (int64_t g = off[u]; g < e; g++) if (lex_less(pc[g], pq[g], bc, bp)) { bc = pc[g]; bp = pq[g]; }
    if (bp < 0) return;
    G.opt[r] = bp;
    if (lex_less(bc, bp, G.bc[r], G.bp[r])) { G.bc[r] = bc; G.bp[r] = bp; }
}

// ------------------------------------------------------------------ host
template <typename TC>
struct LwsRun {
    cp_csr_s *A;
    hipStream_t s;
    LwsArgs<TC> G;
    const std::vector<int32_t> *lo;
    int64_t L;
    DBuf<int64_t> off, scratch;
    DBuf<int32_t> cnt32, pq;
    DBuf<TC> pc;
    int64_t cap;

    template <typename F> void launch(F &&f) { ProfScope ps(PROF_LWS, s, 0.0); f(); }

    void rect(int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        const int64_t m = rb - ra + 1, cols = jb - ja + 1;
        if (cols <= LWS_BRUTE_COLS && m * cols <= LWS_BRUTE_CELLS) {
            launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_brute<TC>), dim3((unsigned)m), dim3(64), 0, s, G, ja, jb, ra); });
            return;
        }
        int64_t h = 1;
        while (2 * h <= m) h *= 2;               // rows h - 1 (+ 2h u) first
        for (; h >= 1; h /= 2) {
            LwsLevel Lv;
            Lv.ra = ra; Lv.m = m; Lv.ja = ja; Lv.jb = jb; Lv.h = h;
            Lv.cnt = (m - h + 1 + 2 * h - 1) / (2 * h);
            Lv.cap = std::min<int64_t>(cap, (cols + Lv.cnt + LWS_CH - 1) / LWS_CH + Lv.cnt);
            const bool lds = Lv.cnt <= LWS_LDS_ROWS;
            if (!lds) {
                launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_count<TC>), dim3((unsigned)cdiv(Lv.cnt, 256)), dim3(256), 0, s, G, Lv, cnt32.p); });
                launch([&] { exclusive_scan_i32(cnt32.p, off.p, Lv.cnt, scratch, s); });          // (three kernels, one timed step)
            }
            launch([&] {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_level<TC>), dim3((unsigned)cdiv(Lv.cap, 4)), dim3(256), 0, s, G, Lv, off.p, (int32_t)lds,
                                   pc.p, pq.p);
            });
            launch([&] {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_fin<TC>), dim3((unsigned)cdiv(Lv.cnt, 256)), dim3(256), 0, s, G, Lv, (const int64_t *)off.p,
                                   (const TC *)pc.p, (const int32_t *)pq.p);
            });
        }
    }

    // the feasible cells of columns [ja, jb] x rows [ra, rb] as full rectangles (rows with lo(r) <= ja see every column)
    void push(int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        if (ja > jb || ra > rb) return;
        const int32_t *l = lo->data();
        const int64_t r1 = (int64_t)(std::upper_bound(l + ra, l + rb + 1, (int32_t)ja) - l) - 1;     // last row with lo <= ja
        const int64_t r2 = (int64_t)(std::upper_bound(l + ra, l + rb + 1, (int32_t)jb) - l) - 1;     // last row with lo <= jb
        if (r1 >= ra) rect(ja, jb, ra, r1);
        if (r2 > r1 && jb - ja < LWS_STAIR_COLS) {
            launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_stair<TC>), dim3((unsigned)(r2 - r1)), dim3(64), 0, s, G, ja, jb, r1 + 1); });
        } else if (r2 > r1) {
            const int64_t jm = (ja + jb) / 2;
            push(jm + 1, jb, r1 + 1, r2);
            push(ja, jm, r1 + 1, r2);
        }
    }

    void leaf(int64_t x, int64_t y)
    {
        launch([&] {
            if (L == 256) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_leaf<TC, 4>), dim3(1), dim3(64), 0, s, G, x, y);
            else if (L == 512) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_leaf<TC, 8>), dim3(1), dim3(64), 0, s, G, x, y);
            else if (L == 1024) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_leaf<TC, 16>), dim3(1), dim3(64), 0, s, G, x, y);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lws_leaf<TC, 32>), dim3(1), dim3(64), 0, s, G, x, y);
        });
    }

    // rows [x, y]; the left part is a whole number of leaves
    void solve(int64_t x, int64_t y)
    {
        const int64_t len = y - x + 1;
        if (len <= L) { leaf(x, y); return; }
        const int64_t nb = cdiv(len, L), mid = x + L * ((nb + 1) / 2) - 1;
        solve(x, mid);
        push(x, mid, mid + 1, y);
        solve(mid + 1, y);
    }
};

// the weights lo(r) is known for: none / Feasible (0), a width (VertexCount past 16, width_of_weight) or a monotone AffineWorkModel budget
// (k_weight_j0); Int64 budgets only while alpha + n b_v + N b_p cannot wrap.  -> 0: none, 1: width (*wv), 2: budget, -1: other
static int lws_weight_kind(const cp_csr_s *A, const cp_model_t *w, int64_t wi, double wf, int64_t *wv)
{
    if (!w || w->kind == CP_MODEL_FEASIBLE) return 0;
    if (w->kind == CP_MODEL_VERTEX_COUNT) { *wv = wi; return wi <= 16 ? -1 : 1; }      // (w <= 16: the (min,+) scan / one-wave kernel)
    if (w->kind != CP_MODEL_WORK || w->alpha_k) return -1;
    if (w->dtype == CP_I64) {
        typedef unsigned __int128 u128;
        auto mag = [](int64_t v) { return v < 0 ? (u128)0 - (u128)(__int128)v : (u128)v; };
        const u128 b = mag(w->p_i64[CP_P_ALPHA]) + mag(w->p_i64[CP_P_VERTEX]) * (u128)(A->n + 1) + mag(w->p_i64[CP_P_PIN]) * (u128)(A->N + 1) + mag(wi);
        if (b >= ((u128)1 << 62)) return -1;
    }
    const int64_t v = width_of_weight(w, A->n, wi, wf);
    if (v >= -1) { *wv = v; return 1; }
    return monotone_work_weight(w) ? 2 : -1;
}

bool lws_ok(const cp_csr_s *A, const cp_model_t *mdl, const cp_model_t *w, int64_t wi, double wf)
{
    int64_t wv = 0;
    return g_opt_lws && !g_opt_force_brute && A->n >= 1 && A->n < ((int64_t)1 << 30) && A->N < ((int64_t)1 << 31) - 1 && !mdl->alpha_k &&
           (mdl->kind == CP_MODEL_WORK || mdl->kind == CP_MODEL_CONNECTIVITY || mdl->kind == CP_MODEL_HYPEREDGE_CUT) &&
           fast_total_ok(mdl, A->n, A->N, A->n + 1) && lws_weight_kind(A, w, wi, wf, &wv) >= 0;
}

template <typename TC>
int32_t run_pack_lws(cp_csr_s *A, const DevModel<TC> &M, const WaveletDev &wnet, const WaveletDev &wself, const cp_model_t *w, int64_t wi,
                     double wf, TC *cst1, int64_t *spl1)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    const bool nets = M.kind == CP_MODEL_CONNECTIVITY || M.kind == CP_MODEL_HYPEREDGE_CUT, self = M.kind == CP_MODEL_HYPEREDGE_CUT;
    ensure_links(A);
    if (self) ensure_self(A);
    int64_t wv = 0;
    const int wk = lws_weight_kind(A, w, wi, wf, &wv);
    CP_REQUIRE(wk >= 0, CP_EINTERNAL, "run_pack_lws: unsupported weight");
    std::vector<int32_t> lo((size_t)n1, 0);
    DBuf<int32_t> dlo((size_t)n1);
    if (wk == 2) {
        const unsigned gw = (unsigned)cdiv(n1, 256);
        if (w->dtype == CP_I64)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_weight_j0<int64_t>), dim3(gw), dim3(256), 0, s, n, A->pos.p, w->p_i64[CP_P_ALPHA],
                               w->p_i64[CP_P_VERTEX], w->p_i64[CP_P_PIN], wi, dlo.p);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_weight_j0<double>), dim3(gw), dim3(256), 0, s, n, A->pos.p, w->p_f64[CP_P_ALPHA],
                               w->p_f64[CP_P_VERTEX], w->p_f64[CP_P_PIN], wf, dlo.p);
        CP_HIP(hipGetLastError());
        CP_HIP(hipMemcpyAsync(lo.data(), dlo.p, sizeof(int32_t) * (size_t)n1, hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
    } else if (wk == 1) {
        for (int64_t r = 0; r <= n; r++) lo[(size_t)r] = (int32_t)(wv >= 0 ? std::max<int64_t>(0, r - std::min<int64_t>(wv, r)) : r + 1);
    }
    for (int64_t r = 1; r <= n; r++)             // @assert j0 < j' (DynamicChunker.jl:31): every row needs a candidate
        if (lo[(size_t)r] >= r) { set_error("pack_stripe: a single column exceeds w_max (@assert j0 < j')"); return CP_EINVAL; }
    if (wk != 2) CP_HIP(hipMemcpyAsync(dlo.p, lo.data(), sizeof(int32_t) * (size_t)n1, hipMemcpyHostToDevice, s));

    LwsRun<TC> R;
    R.A = A; R.s = s; R.lo = &lo;
    R.L = g_opt_lws_leaf;
    DBuf<TC> bc((size_t)n1);
    DBuf<int32_t> bp((size_t)n1), opt((size_t)n1);
    CP_HIP(hipMemsetAsync(bp.p, 0xff, bp.bytes(), s));
    R.cap = (2 * n1 + LWS_CH - 1) / LWS_CH + n1 + 1;
    R.pc.alloc((size_t)R.cap); R.pq.alloc((size_t)R.cap);
    R.off.alloc((size_t)n1 + 1); R.cnt32.alloc((size_t)n1);
    LwsArgs<TC> &G = R.G;
    memset(&G, 0, sizeof(G));
    G.M = M; G.alpha = M.p[CP_P_ALPHA]; G.n = n; G.nets = nets; G.self = self;
    G.pos = A->pos.p; G.prev = A->prev.p; G.lpos = self ? A->lpos.p : nullptr; G.lfirst = self ? A->lfirst.p : nullptr;
    G.wnet = wnet; G.wself = wself;
    G.lo = dlo.p; G.bc = bc.p; G.bp = bp.p; G.opt = opt.p; G.cst1 = cst1; G.spl1 = spl1;
    R.solve(0, n);
    CP_HIP(hipGetLastError());
    CP_HIP(hipStreamSynchronize(s));              // (the buffers above are released on return)
    return CP_OK;
}

template int32_t run_pack_lws<int64_t>(cp_csr_s *, const DevModel<int64_t> &, const WaveletDev &, const WaveletDev &, const cp_model_t *, int64_t, double,
                                       int64_t *, int64_t *);
template int32_t run_pack_lws<double>(cp_csr_s *, const DevModel<double> &, const WaveletDev &, const WaveletDev &, const cp_model_t *, int64_t, double,
                                      double *, int64_t *);

}  // namespace cpk
