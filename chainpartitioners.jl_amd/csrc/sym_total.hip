// sym_total.hip -- one layer of the K-part total-cost DP of the symmetric cost family (sym.hpp), unconstrained, at any n:
// partition_stripe(A, K, DynamicTotal{Splitter,Chunker}(f)) with f an AffineSymmetricConnectivityModel, its monotonized form or an
// AffineSymmetricEdgeCutModel inside sym_total_ok (model.hpp).  DESIGN 5b.
//
// 0-based rows r = j' - 1 and candidates p = j - 1:
//     cst[r] = min over 0 <= p <= r of W[p] + f(p, r, k),
// the LARGEST p among equal values (DynamicSplitter.jl:37-43).  This is the two-staircase layer of dp_total_budget.hip with the
// closed-form staircases a(r) = lo, b(r) = min(r, hi), lo = 0, hi = n: the same decomposition (lws_decomp.hpp) into full rectangles
// and scans of partial rows, the same rectangle engine (lws_rect.hpp), a cell being one sym_eval call.  Inside the gate the cost is
// inverse-Monge on a full rectangle, so the rightmost argmin does not increase with r there.
//
// In the triangle every block [ja, jb] of the column tree owns at most one rectangle, the rows [jb, the parent's jb - 1]: the
// rectangles found at one depth of the tree have pairwise disjoint rows and pairwise disjoint columns, and so have the partial rows
// of its leaves.  With "sym_total_batch" (default) a depth is therefore ONE launch sequence -- the levels of its large rectangles
// together (LwsBatch), one scan launch for its small rectangles, one for its partial rows -- instead of one sequence per rectangle:
// at most D (4 L + 2) + 1 launches per layer for D depths and L = ceil(log2(n + 1)) levels.  The descriptors of a layer geometry are
// computed once on the host and kept on the device (LwsPlan, lws_plan.hpp, shared with plaid_total.hip).  A rectangle's rows and a leaf's partial rows of the same depth may
// coincide, which is why those two are separate launches.
//
// Every cell is W[p] + sym_eval(...) in that order, the sweep's expression (k_sym_brute_layer), and the gate admits exact totals
// only, so the tables are the sweep's bit for bit in both cost types.  The whole layer is enqueued without a host synchronisation
// (the first layer of a new geometry uploads its plan from pageable memory).
#include "dp.hpp"
#include "sym.hpp"
#include "lws_plan.hpp"

namespace cpk {

int64_t g_opt_sym_total = 1, g_opt_sym_total_batch = 1;
int64_t g_opt_sym_total_min_n = 10240;         // the first measured n at which this path beats the sweep (16.0 ms against 20.1 ms)
int64_t g_opt_sym_total_scan_cells = LWS_BRUTE_CELLS, g_opt_sym_total_scan_cols = LWS_BRUTE_COLS, g_opt_sym_total_stair_cols = LWS_STAIR_COLS;
int64_t g_sym_total_layers = 0;

template <typename TC>
struct SymArgs {
    SymDev S;
    DevModel<TC> M;
    TC alpha;
    TC *bc; int32_t *bp;                         // n + 1 : best pair of each row so far
    int32_t *opt;                                // n + 1 : argmin of a row inside the current rectangle
    const TC *W;                                 // n + 1 : the previous layer's cost row
    int64_t p_lo0, p_hi0;                        // the previous layer's limits: a(r) = p_lo0, b(r) = min(r, p_hi0)
};

// the policy of lws_rect.hpp: candidates start from W[p], a cell is the symmetric cost, ties go to the largest p
template <typename TC_>
struct SymLast {
    using TC = TC_;
    using Args = SymArgs<TC>;
    static __device__ __forceinline__ TC base(const Args &G, int64_t p) { return G.W[p]; }
    static __device__ __forceinline__ TC cell(const Args &G, int64_t p, int64_t r) { return sym_eval<TC>(G.S, G.M, G.alpha, p, r); }
    static __device__ __forceinline__ bool better(TC c, int32_t p, TC bc, int32_t bp) { return p >= 0 && (bp < 0 || c < bc || (c == bc && p > bp)); }
    static __device__ __forceinline__ int64_t stair_lo(const Args &G, int64_t, int64_t ja) { return G.p_lo0 > ja ? G.p_lo0 : ja; }
    static __device__ __forceinline__ int64_t stair_hi(const Args &G, int64_t r, int64_t jb)
    {
        const int64_t b = std::min<int64_t>(r, G.p_hi0);
        return b < jb ? b : jb;
    }
};

template <typename TC> struct SymBig;
template <> struct SymBig<int64_t> { static __device__ int64_t v() { return (int64_t)1 << 61; } };
template <> struct SymBig<double> { static __device__ double v() { return 1152921504606846976.0; } };      // 2^60

// rows [rlo, rhi] start from (a value no real total reaches, the row's first candidate): every real candidate replaces it
template <typename TC>
__global__ void __launch_bounds__(256) k_sym_total_init(SymArgs<TC> G, int64_t rlo, int64_t rhi)
{
    const int64_t r = rlo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rhi) return;
    G.bc[r] = SymBig<TC>::v();
    G.bp[r] = (int32_t)(G.p_lo0 < r ? G.p_lo0 : r);
}

// "sym_total_batch" 0: every rectangle and every set of partial rows is launched as it is found, as dp_total_budget.hip does
template <typename TC>
struct SymEach {
    LwsRect<SymLast<TC>> &E;
    void rect(int, int64_t ja, int64_t jb, int64_t ra, int64_t rb) { E.rect(ja, jb, ra, rb); }
    void stair(int, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2, int64_t m2) { E.stair(ja, jb, ra, m, ra2, m2); }
};

// ------------------------------------------------------------------ per-matrix state: the engine's scratch and the plans
struct SymTotalWork {
    DBuf<int32_t> opt;
    LwsRect<SymLast<int64_t>> Ri;
    LwsRect<SymLast<double>> Rf;
    LwsPlanCache plans;                          // a K-layer run has two geometries: the full layers and the last row
    template <typename TC> LwsRect<SymLast<TC>> &engine();
};
template <> LwsRect<SymLast<int64_t>> &SymTotalWork::engine<int64_t>() { return Ri; }
template <> LwsRect<SymLast<double>> &SymTotalWork::engine<double>() { return Rf; }

static SymTotalWork *sym_total_work_get(cp_csr_s *A)
{
    SymWork *S = sym_work_get(A);
    if (!S->total) {
        S->total = new SymTotalWork();
        S->total_free_fn = [](void *w) { delete reinterpret_cast<SymTotalWork *>(w); };
    }
    return reinterpret_cast<SymTotalWork *>(S->total);
}

template <typename TC>
void sym_total_layer(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    if (rhi < rlo) return;
    CP_REQUIRE(rlo >= 0 && rhi <= n && n < ((int64_t)1 << 30), CP_EINTERNAL, "sym_total_layer: bad rows");
    SymTotalWork *T = sym_total_work_get(A);
    if (T->opt.n < (size_t)n1) {                 // (zeroed once: whatever a level reads there is a candidate index, also outside the gate's promise)
        T->opt.alloc((size_t)n1);
        CP_HIP(hipMemsetAsync(T->opt.p, 0, T->opt.bytes(), s));
    }

    LwsRect<SymLast<TC>> &E = T->template engine<TC>();
    E.s = s; E.prof = PROF_SYM_TOTAL;
    E.brute_cells = g_opt_sym_total_scan_cells; E.brute_cols = g_opt_sym_total_scan_cols;
    E.reserve(2 * n1 + 2);                       // (a depth's rectangles together: up to n + 1 level rows and one more chunk per rectangle)
    SymArgs<TC> &G = E.G;
    memset(&G, 0, sizeof(G));
    G.S = S; G.M = M; G.alpha = alpha;
    G.bc = cst_out; G.bp = ptr_out; G.opt = T->opt.p;
    G.W = W; G.p_lo0 = 0; G.p_hi0 = n;

    const int64_t m = rhi - rlo + 1;
    E.launch([&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sym_total_init<TC>), dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, G, rlo, rhi); });
    if (g_opt_sym_total_batch) {
        const int64_t key[LwsPlan::NKEY] = {rlo, rhi, G.p_lo0, G.p_hi0, g_opt_sym_total_stair_cols, E.brute_cells, E.brute_cols};
        T->plans.run(E, T->plans.get(key, E.cap, s));
    } else {
        SymEach<TC> each{E};
        const LwsTriStairs st{G.p_lo0, G.p_hi0};
        stair_decompose(st, each, g_opt_sym_total_stair_cols, G.p_lo0, G.p_hi0, rlo, rhi);
    }
    CP_HIP(hipGetLastError());
    g_sym_total_layers++;
}

template void sym_total_layer<int64_t>(cp_csr_s *, const SymDev &, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void sym_total_layer<double>(cp_csr_s *, const SymDev &, const DevModel<double> &, double, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk
