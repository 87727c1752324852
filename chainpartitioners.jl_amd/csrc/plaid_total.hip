// plaid_total.hip -- the K-part total-cost DP of the plaid connectivity pair under a row partition Pi, exact at any n:
// partition_stripe(A, K, DynamicTotalSplitter(f), Pi) with f an AffinePrimaryConnectivityModel inside plaid_total_ok or an
// AffineSecondaryConnectivityModel inside plaid_scan_exact (model.hpp).  DESIGN 5d.
//
// 0-based rows r = j' - 1 and candidates p = j - 1:   cst[r] = min over 0 <= p <= r of W[p] + f(p, r, k), the LARGEST p among equal
// values (DynamicSplitter.jl:37-43).
//
// Primary.  Inside the gate the cost is inverse-Monge on a full rectangle, so a layer is the triangle decomposition of lws_plan.hpp on
// the rectangle engine of lws_rect.hpp, as sym_total.hip runs it, a cell being the random-access evaluation of oracle_eval_dev
// (bisect.hip) in the same expression and operand order: pins from pos, nets from A's net counter, the local nets l from the net
// counter of the partwise matrix, dm_apply(M, alpha_k, r - p, pins, l, nets - l), combined as W[p] + f.  The gate admits exact totals
// only, so the tables are the sweep's (k_plaid_layer) bit for bit in both cost types.  The two binary searches of pw_rank per cell are
// replaced by a per-layer array Lk[0 .. n], the number of columns < c that hold a row of part k: the partwise column of c is
// pios[k] - 1 + Lk[c].  Lk is a flag scattered for each of part k's entries of prm and one exclusive scan -- O(n'_k + n), a heavy column
// costs nothing extra.  Per layer >= 2: the two preparation steps (scatter, scan), the init launch and the plan's launches; nothing is
// copied back, the whole layer is enqueued without a host synchronisation (the first layer of a geometry uploads its plan).
//
// Secondary.  f(i, i', k) = const_k + S_k[i'] - S_k[i] with S_k[c] = Lk[c]*(b_local_net - b_remote_net) and const_k = alpha_k +
// nv_k*b_vertex + w_k*b_pin + d_k*b_remote_net: the secondary edge-cut form over the prefix count Lk, so a layer is the prefix-min
// scan of plaid_cut.hip (cut_scan_layer) with b_self_pin := b_local_net and b_cut_pin := b_remote_net.  nv_k and w_k come from Pi's split
// vector and A's row pointer, d_k = pios[k + 1] - pios[k], all on the host before the first layer.
#include "plaid_total.hpp"
#include "partwise.hpp"
#include "cut.hpp"
#include "lws_plan.hpp"

namespace cpk {

int64_t g_opt_plaid_total = 1;
int64_t g_opt_plaid_total_min_n = 1024, g_opt_plaid_scan_min_n = 1024;      // the first measured n at which each beats the sweep (4.2 ms against 33.5 ms, 1.1 ms against 7.4 ms)
int64_t g_opt_plaid_total_scan_cells = LWS_BRUTE_CELLS, g_opt_plaid_total_scan_cols = LWS_BRUTE_COLS, g_opt_plaid_total_stair_cols = LWS_STAIR_COLS;
int64_t g_plaid_total_layers = 0, g_plaid_scan_layers = 0;

// ------------------------------------------------------------------ the one decision
PlaidPath plaid_path(const cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl)
{
    const int64_t n = A->n;
    const bool past = n > g_opt_brute_max_n;                          // the sweep would refuse
    if (g_opt_plaid_total && !g_opt_force_brute) {
        if (mdl->kind == CP_MODEL_PRIMARY && plaid_total_ok(mdl, n, A->N, K, combine, order) &&
            (n >= g_opt_plaid_total_min_n || (past && n >= PLAID_TOTAL_FLOOR)))
            return PlaidPath::Total;
        if (mdl->kind == CP_MODEL_SECONDARY && plaid_scan_exact(mdl, A->m, A->N, K, combine, order) && (n >= g_opt_plaid_scan_min_n || past))
            return PlaidPath::Scan;
    }
    CP_REQUIRE(!past, CP_EUNSUPPORTED, "plaid cost models run the O(n^2) device sweep: n too large");
    return PlaidPath::Sweep;
}

// ------------------------------------------------------------------ primary: the policy of lws_rect.hpp
template <typename TC>
struct PlaidArgs {
    DevModel<TC> M;
    TC alpha;                                    // alpha_k
    int64_t n;
    const int64_t *pos;
    WaveletDev net;                              // A's net counter
    const int32_t *Lk;                           // n + 1 : columns < c that hold a row of part k
    int64_t pbase;                               // pios[k] - 1: the partwise column of c is pbase + Lk[c] (0-based)
    const int64_t *ppos;                         // the partwise matrix: column pointer (0-based), columns, net counter
    int64_t np;
    WaveletDev lcn;
    TC *bc; int32_t *bp;                         // n + 1 : best pair of each row so far
    int32_t *opt;                                // n + 1 : argmin of a row inside the current rectangle
    const TC *W;                                 // n + 1 : the previous layer's cost row
};

// f(p, r, k): oracle_eval_dev's plaid == 1 branch (bisect.hip) with the ranks read from Lk
template <typename TC>
__device__ __forceinline__ TC plaid_cell(const PlaidArgs<TC> &G, int64_t p, int64_t r)
{
    const int64_t np = G.pos[r] - G.pos[p];
    const int64_t nn = np - wt_count_le(G.net, G.n - p, G.pos[r]);
    const int64_t pj = G.pbase + G.Lk[p], pr = G.pbase + G.Lk[r];
    const int64_t l = (G.ppos[pr] - G.ppos[pj]) - wt_count_le(G.lcn, G.np - pj, G.ppos[pr]);
    return dm_apply(G.M, G.alpha, r - p, np, l, nn - l);
}

// candidates start from W[p], ties go to the largest p (DynamicSplitter.jl:40); the staircases are a = 0, b(r) = r
template <typename TC_>
struct PlaidLast {
    using TC = TC_;
    using Args = PlaidArgs<TC>;
    static __device__ __forceinline__ TC base(const Args &G, int64_t p) { return G.W[p]; }
    static __device__ __forceinline__ TC cell(const Args &G, int64_t p, int64_t r) { return plaid_cell<TC>(G, p, r); }
    static __device__ __forceinline__ bool better(TC c, int32_t p, TC bc, int32_t bp) { return p >= 0 && (bp < 0 || c < bc || (c == bc && p > bp)); }
    static __device__ __forceinline__ int64_t stair_lo(const Args &, int64_t, int64_t ja) { return ja; }
    static __device__ __forceinline__ int64_t stair_hi(const Args &, int64_t r, int64_t jb) { return r < jb ? r : jb; }
};

template <typename TC> struct PlaidBig;
template <> struct PlaidBig<int64_t> { static __device__ int64_t v() { return (int64_t)1 << 61; } };
template <> struct PlaidBig<double> { static __device__ double v() { return 1152921504606846976.0; } };      // 2^60

// rows [rlo, rhi] start from (a value no real total reaches, candidate 0): every real candidate replaces it
template <typename TC>
__global__ void __launch_bounds__(256) k_plaid_total_init(PlaidArgs<TC> G, int64_t rlo, int64_t rhi)
{
    const int64_t r = rlo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rhi) return;
    G.bc[r] = PlaidBig<TC>::v();
    G.bp[r] = 0;
}

// layer 1: cst[j', 1] = f(1, j', 1)  (DynamicSplitter.jl:26-31)
template <typename TC>
__global__ void __launch_bounds__(256) k_plaid_total_first(PlaidArgs<TC> G, int64_t rlo, int64_t rhi)
{
    const int64_t r = rlo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rhi) return;
    G.bc[r] = plaid_cell<TC>(G, 0, r);
    G.bp[r] = 0;
}

// ------------------------------------------------------------------ Lk: one flag per column of part k in partwise order, then a scan
__global__ void __launch_bounds__(256) k_plaid_colflags(int64_t i0, int64_t i1, int64_t n, const int64_t *__restrict__ prm, int32_t *__restrict__ flag)
{
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1) return;
    const int64_t c = prm[i] - 1;                // (prm holds 1-based columns of A; distinct inside a part)
    if (c >= 0 && c < n) flag[c] = 1;
}

// ------------------------------------------------------------------ secondary, layer 1: f(1, i', 1) from the prefix counts, as the sweep writes it
template <typename TC>
__global__ void __launch_bounds__(256) k_plaid_scan_first(int64_t n, DevModel<TC> M, TC alpha, int64_t nvk, int64_t wk, int64_t dk,
                                                          const int32_t *__restrict__ Lk, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const int64_t l = (int64_t)Lk[r] - Lk[0];
    cst[r] = dm_apply(M, alpha, nvk, wk, l, dk - l);
    ptr[r] = 0;
}

// ------------------------------------------------------------------ host
template <typename TC>
struct PlaidTotalState : PlaidTotalRun {
    cp_csr_s *A = nullptr;
    PlaidPath path = PlaidPath::Sweep;
    DevModel<TC> M;
    TC prm5[5];
    PartwiseStage PW;
    DBuf<int32_t> flag, Lk, opt;
    DBuf<int64_t> scratch;
    // primary
    WaveletHost net;
    LwsRect<PlaidLast<TC>> E;
    LwsPlanCache plans;
    // secondary
    std::vector<int64_t> hspl, htpos;
    CutScanWork<TC> ws;
};

template <typename TC>
std::unique_ptr<PlaidTotalRun> plaid_total_begin(cp_csr_s *A, PlaidPath path, const cp_model_t *mdl, const DevModel<TC> &M, const cp_rowpart_t *Pi,
                                                 const PlaidPart &R)
{
    CP_REQUIRE(path == PlaidPath::Total || path == PlaidPath::Scan, CP_EINTERNAL, "plaid_total_begin: not a path of this unit");
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    std::unique_ptr<PlaidTotalState<TC>> T(new PlaidTotalState<TC>());
    T->A = A; T->path = path; T->M = M;
    for (int i = 0; i < 5; i++) T->prm5[i] = model_param<TC>(mdl, i);
    const bool sec = path == PlaidPath::Scan;
    const int32_t rc = partwise_stage(A, Pi, sec ? PW_RANK : PW_NETS, T->PW);      // once per call
    if (rc != CP_OK) throw HipFail{rc};
    T->flag.alloc((size_t)(n > 0 ? n : 1)); T->Lk.alloc((size_t)n + 2);
    if (sec) {
        T->hspl = R.hspl;
        T->htpos.resize((size_t)A->m + 1);                            // pins of every part of Pi: tpos = row pointer of A
        CP_HIP(hipMemcpyAsync(T->htpos.data(), A->tpos.p, sizeof(int64_t) * (size_t)(A->m + 1), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
    } else {
        ensure_net_counter(A, T->net);
        T->opt.alloc((size_t)n + 1);             // (zeroed once: whatever a level reads there is a candidate index)
        CP_HIP(hipMemsetAsync(T->opt.p, 0, T->opt.bytes(), s));
    }
    return std::unique_ptr<PlaidTotalRun>(T.release());
}

template <typename TC>
void plaid_total_layer(PlaidTotalRun *run, int64_t k, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi)
{
    PlaidTotalState<TC> *T = static_cast<PlaidTotalState<TC> *>(run);
    cp_csr_s *A = T->A;
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    if (rhi < rlo) return;
    CP_REQUIRE(rlo >= 0 && rhi <= n && n < ((int64_t)1 << 30) && k >= 1, CP_EINTERNAL, "plaid_total_layer: bad rows or part");
    // part k's columns of the partwise matrix; a part number past Pi's owns no row (the sweep's owner[row] == k is never true)
    const int64_t i0 = k <= T->PW.Kp ? T->PW.hpios[(size_t)k - 1] - 1 : T->PW.npr, i1 = k <= T->PW.Kp ? T->PW.hpios[(size_t)k] - 1 : T->PW.npr;
    CP_REQUIRE(i0 >= 0 && i0 <= i1 && i1 <= T->PW.npr, CP_EINTERNAL, "plaid_total_layer: partwise offsets out of range");
    {   // preparation, two timed steps: the flags of part k's columns, their exclusive scan Lk[0 .. n]
        ProfScope ps(PROF_PLAID_TOTAL, s, 0.0);
        if (n > 0) CP_HIP(hipMemsetAsync(T->flag.p, 0, sizeof(int32_t) * (size_t)n, s));
        if (i1 > i0) hipLaunchKernelGGL(k_plaid_colflags, dim3((unsigned)cdiv(i1 - i0, 256)), dim3(256), 0, s, i0, i1, n, T->PW.prm.p, T->flag.p);
    }
    {
        ProfScope ps(PROF_PLAID_TOTAL, s, 0.0);
        exclusive_scan_i32_i32(T->flag.p, T->Lk.p, n, T->scratch, s);
    }
    if (T->path == PlaidPath::Scan) {
        const int64_t s0 = T->hspl[(size_t)k - 1] - 1, s1 = T->hspl[(size_t)k] - 1;
        const int64_t nvk = s1 - s0, wk = T->htpos[(size_t)s1] - T->htpos[(size_t)s0], dk = i1 - i0;
        ProfScope ps(PROF_PLAID_TOTAL, s, 0.0);
        if (k == 1) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_plaid_scan_first<TC>), dim3((unsigned)cdiv(n1, 256)), dim3(256), 0, s, n, T->M, alpha, nvk, wk, dk,
                               (const int32_t *)T->Lk.p, cst_out, ptr_out);
        } else {
            CutLayer<TC> Y;
            memset(&Y, 0, sizeof(Y));
            Y.secondary = 1; Y.alpha = alpha; Y.nvk = nvk; Y.wk = wk;
            Y.p[CP_P_SELF_PIN] = T->prm5[CP_P_LOCAL_NET]; Y.p[CP_P_CUT_PIN] = T->prm5[CP_P_REMOTE_NET];
            const TC constk = cadd(cadd(cadd(alpha, cmulc(nvk, T->prm5[CP_P_VERTEX])), cmulc(wk, T->prm5[CP_P_PIN])), cmulc(dk, T->prm5[CP_P_REMOTE_NET]));
            cut_scan_layer<TC>(s, n1, Y, constk, A->pos.p, T->Lk.p, W, T->ws, cst_out, ptr_out);      // (the whole layer in its one pass)
            g_plaid_scan_layers++;
        }
        CP_HIP(hipGetLastError());
        return;
    }

    LwsRect<PlaidLast<TC>> &E = T->E;
    E.s = s; E.prof = PROF_PLAID_TOTAL;
    E.brute_cells = g_opt_plaid_total_scan_cells; E.brute_cols = g_opt_plaid_total_scan_cols;
    E.reserve(2 * n1 + 2);                       // (a depth's rectangles together: up to n + 1 level rows and one more chunk per rectangle)
    PlaidArgs<TC> &G = E.G;
    memset(&G, 0, sizeof(G));
    G.M = T->M; G.alpha = alpha; G.n = n; G.pos = A->pos.p; G.net = T->net.d;
    G.Lk = T->Lk.p; G.pbase = i0; G.ppos = T->PW.Ap->pos.p; G.np = T->PW.npr; G.lcn = T->PW.lcn.d;
    G.bc = cst_out; G.bp = ptr_out; G.opt = T->opt.p; G.W = W;
    const int64_t m = rhi - rlo + 1;
    if (k == 1) {
        E.launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_plaid_total_first<TC>), dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, G, rlo, rhi); });
        CP_HIP(hipGetLastError());
        return;
    }
    E.launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_plaid_total_init<TC>), dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, G, rlo, rhi); });
    const int64_t key[LwsPlan::NKEY] = {rlo, rhi, 0, n, g_opt_plaid_total_stair_cols, E.brute_cells, E.brute_cols};
    T->plans.run(E, T->plans.get(key, E.cap, s));
    CP_HIP(hipGetLastError());
    g_plaid_total_layers++;
}

template std::unique_ptr<PlaidTotalRun> plaid_total_begin<int64_t>(cp_csr_s *, PlaidPath, const cp_model_t *, const DevModel<int64_t> &, const cp_rowpart_t *, const PlaidPart &);
template std::unique_ptr<PlaidTotalRun> plaid_total_begin<double>(cp_csr_s *, PlaidPath, const cp_model_t *, const DevModel<double> &, const cp_rowpart_t *, const PlaidPart &);
template void plaid_total_layer<int64_t>(PlaidTotalRun *, int64_t, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void plaid_total_layer<double>(PlaidTotalRun *, int64_t, double, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk
