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
// computed once on the host and kept on the device (SymPlan).  A rectangle's rows and a leaf's partial rows of the same depth may
// coincide, which is why those two are separate launches.
//
// Every cell is W[p] + sym_eval(...) in that order, the sweep's expression (k_sym_brute_layer), and the gate admits exact totals
// only, so the tables are the sweep's bit for bit in both cost types.  The whole layer is enqueued without a host synchronisation
// (the first layer of a new geometry uploads its plan from pageable memory).
#include "dp.hpp"
#include "sym.hpp"
#include "lws_rect.hpp"
#include "lws_decomp.hpp"
#include <memory>

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

// ------------------------------------------------------------------ host: the two staircases in closed form
struct SymStairs {
    int64_t lo, hi;                              // a(r) = lo, b(r) = min(r, hi)
    int64_t first_b_ge(int64_t x, int64_t y, int64_t v) const
    {
        if (v > hi) return y + 1;
        const int64_t r = std::max(x, v);
        return r > y ? y + 1 : r;
    }
    int64_t last_a_le(int64_t x, int64_t y, int64_t v) const { return lo <= v ? y : x - 1; }
};

// "sym_total_batch" 0: every rectangle and every set of partial rows is launched as it is found, as dp_total_budget.hip does
template <typename TC>
struct SymEach {
    LwsRect<SymLast<TC>> &E;
    void rect(int, int64_t ja, int64_t jb, int64_t ra, int64_t rb) { E.rect(ja, jb, ra, rb); }
    void stair(int, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2, int64_t m2) { E.stair(ja, jb, ra, m, ra2, m2); }
};

// ------------------------------------------------------------------ host: the launch plan of one layer geometry
// per depth of the column tree: the large rectangles with the prefixes of their row counts level by level, the small rectangles and
// the partial rows with the prefixes of their rows; all descriptors in one device array, all prefixes in another
struct SymPlan {
    static constexpr int NKEY = 7;
    int64_t key[NKEY];                           // rlo, rhi, lo, hi, stair_cols, scan_cells, scan_cols
    struct Rows { int64_t rd, pre, nr, rows; };
    struct Level { int64_t h, pre, cnt, cap; };
    struct Depth { int64_t rd, nr; std::vector<Level> levels; Rows small, stair; };
    std::vector<Depth> depths;
    std::vector<LwsRectD> hrd;                   // (the host copies live as long as the plan: the upload reads them)
    std::vector<int32_t> hpre;
    DBuf<LwsRectD> rd;
    DBuf<int32_t> pre;
};

struct SymPlanSink {
    struct Lists { std::vector<LwsRectD> big, small, stair; };
    std::vector<Lists> d;
    int64_t scan_cells, scan_cols;
    Lists &at(int depth)
    {
        if ((size_t)depth >= d.size()) d.resize((size_t)depth + 1);
        return d[(size_t)depth];
    }
    void rect(int depth, int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        const int64_t m = rb - ra + 1, cols = jb - ja + 1;
        const bool whole = cols <= scan_cols && m * cols <= scan_cells;      // (LwsRect::rect's rule)
        (whole ? at(depth).small : at(depth).big).push_back({(int32_t)ra, (int32_t)m, (int32_t)ja, (int32_t)jb});
    }
    void stair(int depth, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2, int64_t m2)
    {
        if (m > 0) at(depth).stair.push_back({(int32_t)ra, (int32_t)m, (int32_t)ja, (int32_t)jb});
        if (m2 > 0) at(depth).stair.push_back({(int32_t)ra2, (int32_t)m2, (int32_t)ja, (int32_t)jb});
    }
};

// cap: the engine's chunk capacity (LwsRect::cap)
static std::unique_ptr<SymPlan> sym_plan_build(const int64_t *key, int64_t cap, hipStream_t s)
{
    std::unique_ptr<SymPlan> P(new SymPlan());
    memcpy(P->key, key, sizeof(P->key));
    const int64_t rlo = key[0], rhi = key[1], lo = key[2], hi = key[3];
    SymPlanSink sink;
    sink.scan_cells = key[5]; sink.scan_cols = key[6];
    const SymStairs st{lo, hi};
    stair_decompose(st, sink, key[4], lo, hi, rlo, rhi);
    auto add_rows = [&](const std::vector<LwsRectD> &v, SymPlan::Rows &R) {
        R.rd = (int64_t)P->hrd.size(); R.nr = (int64_t)v.size(); R.pre = (int64_t)P->hpre.size();
        int64_t run = 0;
        for (const LwsRectD &x : v) { P->hpre.push_back((int32_t)run); run += x.m; }
        P->hpre.push_back((int32_t)run);
        R.rows = run;
        P->hrd.insert(P->hrd.end(), v.begin(), v.end());
    };
    for (const SymPlanSink::Lists &L : sink.d) {
        SymPlan::Depth D;
        D.rd = (int64_t)P->hrd.size(); D.nr = (int64_t)L.big.size();
        P->hrd.insert(P->hrd.end(), L.big.begin(), L.big.end());
        int64_t hmax = 0;
        for (const LwsRectD &x : L.big) { int64_t h = 1; while (2 * h <= x.m) h *= 2; hmax = std::max(hmax, h); }
        for (int64_t h = hmax; h >= 1; h /= 2) {                       // rows h - 1 (+ 2h u) of every rectangle with m >= h
            SymPlan::Level lv;
            lv.h = h; lv.pre = (int64_t)P->hpre.size();
            int64_t cnt = 0, chunks = 0;
            for (const LwsRectD &x : L.big) {
                P->hpre.push_back((int32_t)cnt);
                const int64_t c = lws_level_rows(x.m, h);
                cnt += c;
                if (c > 0) chunks += lws_level_chunks((int64_t)x.jb - x.ja + 1, c);
            }
            P->hpre.push_back((int32_t)cnt);
            lv.cnt = cnt; lv.cap = std::min(cap, chunks);
            D.levels.push_back(lv);
        }
        add_rows(L.small, D.small);
        add_rows(L.stair, D.stair);
        P->depths.push_back(std::move(D));
    }
    P->rd.alloc(std::max<size_t>(P->hrd.size(), 1)); P->pre.alloc(std::max<size_t>(P->hpre.size(), 1));
    if (!P->hrd.empty()) CP_HIP(hipMemcpyAsync(P->rd.p, P->hrd.data(), sizeof(LwsRectD) * P->hrd.size(), hipMemcpyHostToDevice, s));
    if (!P->hpre.empty()) CP_HIP(hipMemcpyAsync(P->pre.p, P->hpre.data(), sizeof(int32_t) * P->hpre.size(), hipMemcpyHostToDevice, s));
    return P;
}

// ------------------------------------------------------------------ per-matrix state: the engine's scratch and the plans
struct SymTotalWork {
    DBuf<int32_t> opt;
    LwsRect<SymLast<int64_t>> Ri;
    LwsRect<SymLast<double>> Rf;
    std::vector<std::unique_ptr<SymPlan>> plans;       // a K-layer run has two geometries: the full layers and the last row
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

static const SymPlan &sym_plan_get(SymTotalWork *T, const int64_t *key, int64_t cap, hipStream_t s)
{
    for (const auto &P : T->plans) if (!memcmp(P->key, key, sizeof(P->key))) return *P;
    if (T->plans.size() >= 8) {                  // (plans of other option settings: wait for the launches that read them, then drop them)
        CP_HIP(hipStreamSynchronize(s));
        T->plans.clear();
    }
    T->plans.push_back(sym_plan_build(key, cap, s));
    return *T->plans.back();
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
        const int64_t key[SymPlan::NKEY] = {rlo, rhi, G.p_lo0, G.p_hi0, g_opt_sym_total_stair_cols, E.brute_cells, E.brute_cols};
        const SymPlan &P = sym_plan_get(T, key, E.cap, s);
        for (const SymPlan::Depth &D : P.depths) {
            for (const SymPlan::Level &lv : D.levels) {
                const LwsBatch B{P.rd.p + D.rd, P.pre.p + lv.pre, D.nr, lv.h, lv.cnt, lv.cap};
                E.level(B);
            }
            E.rows(P.rd.p + D.small.rd, P.pre.p + D.small.pre, D.small.nr, D.small.rows);
            E.rows(P.rd.p + D.stair.rd, P.pre.p + D.stair.pre, D.stair.nr, D.stair.rows);
        }
    } else {
        SymEach<TC> each{E};
        const SymStairs st{G.p_lo0, G.p_hi0};
        stair_decompose(st, each, g_opt_sym_total_stair_cols, G.p_lo0, G.p_hi0, rlo, rhi);
    }
    CP_HIP(hipGetLastError());
    g_sym_total_layers++;
}

template void sym_total_layer<int64_t>(cp_csr_s *, const SymDev &, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void sym_total_layer<double>(cp_csr_s *, const SymDev &, const DevModel<double> &, double, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk
