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
// into the two halves of the columns.  Every feasible cell lies in exactly one rectangle.  Inside a full rectangle the leftmost
// argmin is non-INCREASING in r and the row minima come from the monotone divide and conquer of lws_rect.hpp, which this unit
// shares with dp_total_budget.hip: the rectangle, level and staircase kernels live there, this unit's policy is LwsFirst.  Small
// rectangles are scanned whole, and so is the staircase left of a push below LWS_STAIR_COLS columns.
//
// A leaf of at most 64 * CPT rows runs on one wave, row after row (k_lws_leaf): lane l owns the candidates x + l + 64 k and keeps
// their counts in registers, updated per new column from the link arrays -- nets grow by #{q in column : prev[q] < p}, self nets by
// the rows whose last column is the new one and whose first column is >= p -- so a leaf row costs no rank query.
#include "csr.hpp"
#include "model.hpp"
#include "wavelet.hpp"
#include "weight.hpp"
#include "dp.hpp"
#include "lws_rect.hpp"

namespace cpk {

int64_t g_opt_lws = 1, g_opt_lws_leaf = 512;

template <typename TC>
struct LwsArgs : LwsCounts<TC> {
    const int32_t *prev;                         // link arrays (leaf rows)
    const int32_t *lfirst;
    const int32_t *lo;                           // n + 1 : first candidate of each row
    TC *cst1; int64_t *spl1;                     // the 1-based tables of k_pack_dynamic: cst1[r] = C[r], spl1[r] = p + 1
};

template <typename TC>
__device__ __forceinline__ bool lex_less(TC c, int32_t p, TC bc, int32_t bp)
{
    return p >= 0 && (bp < 0 || c < bc || (c == bc && p < bp));
}

// the policy of lws_rect.hpp: candidates start from the finished C[p], ties go to the smallest p, a block is bounded by lo(r) on the left only
template <typename TC_>
struct LwsFirst {
    using TC = TC_;
    using Args = LwsArgs<TC>;
    static __device__ __forceinline__ TC base(const Args &G, int64_t p) { return G.cst1[p]; }
    static __device__ __forceinline__ TC cell(const Args &G, int64_t p, int64_t r) { return lws_f<TC>(G, p, r); }
    static __device__ __forceinline__ bool better(TC c, int32_t p, TC bc, int32_t bp) { return lex_less(c, p, bc, bp); }
    static __device__ __forceinline__ int64_t stair_lo(const Args &G, int64_t r, int64_t ja) { return G.lo[r] > ja ? (int64_t)G.lo[r] : ja; }
    static __device__ __forceinline__ int64_t stair_hi(const Args &, int64_t, int64_t jb) { return jb; }
};

template <typename TC>
__device__ __forceinline__ void wave_lexmin(TC &c, int32_t &p) { wave_best<LwsFirst<TC>>(c, p); }

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

// ------------------------------------------------------------------ host
template <typename TC>
struct LwsRun : LwsRect<LwsFirst<TC>> {
    using LwsRect<LwsFirst<TC>>::s;
    using LwsRect<LwsFirst<TC>>::G;
    using LwsRect<LwsFirst<TC>>::rect;
    using LwsRect<LwsFirst<TC>>::stair;
    using LwsRect<LwsFirst<TC>>::launch;
    cp_csr_s *A;
    const std::vector<int32_t> *lo;
    int64_t L;

    // the feasible cells of columns [ja, jb] x rows [ra, rb] as full rectangles (rows with lo(r) <= ja see every column)
    void push(int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        if (ja > jb || ra > rb) return;
        const int32_t *l = lo->data();
        const int64_t r1 = (int64_t)(std::upper_bound(l + ra, l + rb + 1, (int32_t)ja) - l) - 1;     // last row with lo <= ja
        const int64_t r2 = (int64_t)(std::upper_bound(l + ra, l + rb + 1, (int32_t)jb) - l) - 1;     // last row with lo <= jb
        if (r1 >= ra) rect(ja, jb, ra, r1);
        if (r2 > r1 && jb - ja < LWS_STAIR_COLS) {
            stair(ja, jb, r1 + 1, r2 - r1);
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
    if (!work_weight_no_wrap(w, A->n, A->N, wi)) return -1;
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
    R.reserve(n1);
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
