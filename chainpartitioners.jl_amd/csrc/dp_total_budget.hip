// dp_total_budget.hip -- one layer of the K-part total-cost DP under a monotone work budget:
// partition_stripe(A, K, DynamicTotal{Splitter,Chunker}(ConstrainedCost(f, AffineWorkModel(alpha, b_v, b_p), w_max)))
// (DynamicSplitter.jl:206-314 with g = +), for the inverse-Monge cost models, at any n.  DESIGN 4g.
//
// 0-based rows r = j' - 1 and candidates p = j - 1.  Layer k >= 2 lives on the rows [rlo, rhi] of its window and
//     cst[r] = min over p in [a(r), b(r)] of W[p] + f(p, r, k),   a(r) = max(j0[r], p_lo0),   b(r) = min(r, p_hi0),
// the LARGEST p among equal values (:233-246: the first candidate unconditionally, later ones with <=).  W is the previous layer's
// cost row and [p_lo0, p_hi0] its window, so only real totals are read; j0[r] is the first column whose part up to r fits the budget
// (k_weight_j0).  p = r, the empty part, is a candidate.
//
// a and b never decrease, so the feasible cells lie between two monotone staircases.  Nothing in a layer depends on the layer's own
// rows, so the decomposition is off-line (push): a block [ja, jb] of candidates meets the contiguous rows with b(r) >= ja and
// a(r) <= jb; those with a(r) <= ja and b(r) >= jb see every candidate of the block -- again contiguous, one FULL rectangle -- and
// the rows above it (cut by b) and below it (cut by a) recurse into the two halves of the block, or, below budget_stair_cols
// columns, are scanned whole in one launch.  Every feasible cell lies in exactly one rectangle or scan.  b(r) >= jb means r >= jb,
// so a full rectangle has jb <= ra and the rightmost argmin does not increase with r (lws_rect.hpp; p2 = r1, the empty part, is
// covered by the same inequality): its row minima come from the rectangle engine this unit shares with chunk_lws.hip.
//
// Every cell is W[p] + dm_apply(...) in that order, the literal kernel's expression, and the gate admits exact totals only, so the
// tables are the reference's bit for bit in both cost types.  The whole layer is enqueued without a host synchronisation.
#include "dp.hpp"
#include "weight.hpp"
#include "lws_rect.hpp"
#include "lws_decomp.hpp"

namespace cpk {

int64_t g_opt_budget_total = 1;
int64_t g_opt_budget_scan_cells = LWS_BRUTE_CELLS, g_opt_budget_scan_cols = LWS_BRUTE_COLS, g_opt_budget_stair_cols = LWS_STAIR_COLS;
int64_t g_budget_layers = 0;

template <typename TC>
struct BudgetArgs : LwsCounts<TC> {
    const TC *W;                                 // n + 1 : the previous layer's cost row
    const int32_t *j0;                           // n + 1 : first column whose part up to the row fits the budget
    int64_t p_lo0, p_hi0;                        // the previous layer's window
};

// the policy of lws_rect.hpp: candidates start from W[p], ties go to the largest p, a block is bounded by a(r) and b(r)
template <typename TC_>
struct BudgetLast {
    using TC = TC_;
    using Args = BudgetArgs<TC>;
    static __device__ __forceinline__ TC base(const Args &G, int64_t p) { return G.W[p]; }
    static __device__ __forceinline__ TC cell(const Args &G, int64_t p, int64_t r) { return lws_f<TC>(G, p, r); }
    static __device__ __forceinline__ bool better(TC c, int32_t p, TC bc, int32_t bp) { return p >= 0 && (bp < 0 || c < bc || (c == bc && p > bp)); }
    static __device__ __forceinline__ int64_t stair_lo(const Args &G, int64_t r, int64_t ja)
    {
        const int64_t a = std::max<int64_t>(G.j0[r], G.p_lo0);
        return a > ja ? a : ja;
    }
    static __device__ __forceinline__ int64_t stair_hi(const Args &G, int64_t r, int64_t jb)
    {
        const int64_t b = std::min<int64_t>(r, G.p_hi0);
        return b < jb ? b : jb;
    }
};

template <typename TC> struct BudgetBig;
template <> struct BudgetBig<int64_t> { static __device__ int64_t v() { return (int64_t)1 << 61; } };
template <> struct BudgetBig<double> { static __device__ double v() { return 1152921504606846976.0; } };      // 2^60

// rows [rlo, rhi] start from (a value no real total reaches, the row's first candidate): every real candidate replaces it
template <typename TC>
__global__ void __launch_bounds__(256) k_budget_init(BudgetArgs<TC> G, int64_t rlo, int64_t rhi)
{
    const int64_t r = rlo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rhi) return;
    const int64_t a = std::max<int64_t>(G.j0[r], G.p_lo0);
    G.bc[r] = BudgetBig<TC>::v();
    G.bp[r] = (int32_t)(a < r ? a : r);
}

// ------------------------------------------------------------------ per-matrix state: the counters and the engine's scratch
struct BudgetWork {
    bool have_net = false, have_self = false;
    WaveletHost net, self;
    DBuf<int32_t> opt;
    LwsRect<BudgetLast<int64_t>> Ri;
    LwsRect<BudgetLast<double>> Rf;
    template <typename TC> LwsRect<BudgetLast<TC>> &engine();
};
template <> LwsRect<BudgetLast<int64_t>> &BudgetWork::engine<int64_t>() { return Ri; }
template <> LwsRect<BudgetLast<double>> &BudgetWork::engine<double>() { return Rf; }

static BudgetWork *budget_work_get(cp_csr_s *A)
{
    if (!A->budget_work) {
        A->budget_work = new BudgetWork();
        A->budget_work_free_fn = [](void *w) { delete reinterpret_cast<BudgetWork *>(w); };
        A->budget_work_reset_fn = [](void *w) { auto *B = reinterpret_cast<BudgetWork *>(w); B->have_net = false; B->have_self = false; };   // (cp_csr_reset_cache)
    }
    return reinterpret_cast<BudgetWork *>(A->budget_work);
}

// ------------------------------------------------------------------ host: the decomposition of one layer
template <typename TC>
struct BudgetRun {
    LwsRect<BudgetLast<TC>> &E;
    std::vector<int32_t> a, b;                   // a(r), b(r) for the rows rlo .. rhi
    int64_t rlo = 0, stair_cols = 1;

    explicit BudgetRun(LwsRect<BudgetLast<TC>> &E_) : E(E_) {}

    // the two staircases, read from the arrays
    int64_t first_b_ge(int64_t x, int64_t y, int64_t v) const
    {
        return rlo + (int64_t)(std::lower_bound(b.begin() + (x - rlo), b.begin() + (y - rlo) + 1, (int32_t)v) - b.begin());
    }
    int64_t last_a_le(int64_t x, int64_t y, int64_t v) const
    {
        return rlo + (int64_t)(std::upper_bound(a.begin() + (x - rlo), a.begin() + (y - rlo) + 1, (int32_t)v) - a.begin()) - 1;
    }
    // every rectangle and every set of partial rows is launched as it is found
    void rect(int, int64_t ja, int64_t jb, int64_t ra, int64_t rb) { E.rect(ja, jb, ra, rb); }
    void stair(int, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2, int64_t m2) { E.stair(ja, jb, ra, m, ra2, m2); }

    // the feasible cells of the candidates [ja, jb] in the rows [ra, rb]
    void push(int64_t ja, int64_t jb, int64_t ra, int64_t rb) { stair_decompose(*this, *this, stair_cols, ja, jb, ra, rb); }
};

template <typename TC>
void dp_total_budget_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi,
                           int64_t p_lo0, int64_t p_hi0, const int32_t *j0_dev, const int32_t *j0_host)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    if (rhi < rlo) return;
    CP_REQUIRE(j0_dev && j0_host && rlo >= 0 && rhi <= n && p_lo0 >= 0 && p_hi0 <= n, CP_EINTERNAL, "dp_total_budget_layer: bad window");
    BudgetWork *B = budget_work_get(A);
    const bool nets = M.kind == CP_MODEL_CONNECTIVITY || M.kind == CP_MODEL_HYPEREDGE_CUT, self = M.kind == CP_MODEL_HYPEREDGE_CUT;
    ensure_links(A);
    if (self) ensure_self(A);
    if (nets && !B->have_net) { ProfScope ps(PROF_WAVELET, s, 0.0); ensure_net_counter(A, B->net); B->have_net = true; }
    if (self && !B->have_self) { ProfScope ps(PROF_WAVELET, s, 0.0); ensure_selfnet_counter(A, B->self); B->have_self = true; }
    B->opt.ensure((size_t)n1);

    LwsRect<BudgetLast<TC>> &E = B->template engine<TC>();
    E.s = s; E.prof = PROF_BUDGET;
    E.brute_cells = g_opt_budget_scan_cells; E.brute_cols = g_opt_budget_scan_cols;
    E.reserve(n1);
    BudgetArgs<TC> &G = E.G;
    memset(&G, 0, sizeof(G));
    G.M = M; G.alpha = alpha; G.n = n; G.nets = nets; G.self = self;
    G.pos = A->pos.p; G.lpos = self ? A->lpos.p : nullptr;
    if (nets) G.wnet = B->net.d;
    if (self) G.wself = B->self.d;
    G.bc = cst_out; G.bp = ptr_out; G.opt = B->opt.p;
    G.W = W; G.j0 = j0_dev; G.p_lo0 = p_lo0; G.p_hi0 = p_hi0;

    BudgetRun<TC> R(E);
    R.rlo = rlo; R.stair_cols = g_opt_budget_stair_cols;
    const int64_t m = rhi - rlo + 1;
    R.a.resize((size_t)m); R.b.resize((size_t)m);
    for (int64_t r = rlo; r <= rhi; r++) {
        R.a[(size_t)(r - rlo)] = (int32_t)std::max<int64_t>(j0_host[r], p_lo0);
        R.b[(size_t)(r - rlo)] = (int32_t)std::min<int64_t>(r, p_hi0);
    }
    E.launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_budget_init<TC>), dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, G, rlo, rhi); });
    R.push(p_lo0, p_hi0, rlo, rhi);
    CP_HIP(hipGetLastError());
    g_budget_layers++;
}

template void dp_total_budget_layer<int64_t>(cp_csr_s *, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t, int64_t,
                                             int64_t, const int32_t *, const int32_t *);
template void dp_total_budget_layer<double>(cp_csr_s *, const DevModel<double> &, double, const double *, double *, int32_t *, int64_t, int64_t, int64_t,
                                            int64_t, const int32_t *, const int32_t *);

// ------------------------------------------------------------------ the gate
bool budget_total_ok(const cp_csr_s *A, int64_t K, const cp_model_t *model, const cp_model_t *weight, int64_t wi, double wf)
{
    if (!g_opt_budget_total || g_opt_force_brute || !weight) return false;
    if (!dp_takes_kind(model->kind, DP_KINDS_AFFINE)) return false;
    if (A->n >= ((int64_t)1 << 30) || A->N >= ((int64_t)1 << 31) - 1) return false;
    if (!fast_total_ok(model, A->n, A->N, K)) return false;
    // a monotone AffineWorkModel without per-part alpha that is no width (those take the windowed geometry of dp_total.hip)
    if (!monotone_work_weight(weight) || width_of_weight(weight, A->n, wi, wf) != -2) return false;
    return work_weight_no_wrap(weight, A->n, A->N, wi);
}

}  // namespace cpk
