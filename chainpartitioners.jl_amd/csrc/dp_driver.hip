// dp_driver.hip -- the K-layer dynamic programme of DynamicSplitter.jl:15-50.  dp_path decides the engine of a run and
// constrained_route how a ConstrainedCost runs: the only two places that combine the models' gates with the objective, the loop order
// and the options.  One driver object, DpRun<TC>, prepares what its path needs and switches on it per layer; the one-shot
// (run_dynamic), windowed (run_dynamic_windowed) and row-tiled step (dp_begin / cp_dp_s::step_layer) entries loop over it.
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include "weight.hpp"
#include "sym.hpp"
#include "envelope.hpp"
#include <memory>

namespace cpk {

// ------------------------------------------------------------------ small kernels used by the driver
// per-column count of entries whose previous occurrence lies before `thr` (thr = 0: first occurrences)
__global__ void k_col_count_prev_lt(const int64_t *__restrict__ pos, const int32_t *__restrict__ prev, int32_t thr,
                                    int32_t *__restrict__ out, int64_t n)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    int32_t k = 0;
    for (int64_t q = pos[c]; q < pos[c + 1]; q++) k += (prev[q] < thr);
    out[c] = k;
}

// layer 1: cst[r] = f(1, j', 1) with nets(0, r) = #first occurrences in columns [0, r)   (DynamicSplitter.jl:26-31)
template <typename TC>
__global__ void k_layer1(int64_t n, const int64_t *__restrict__ pos, const int64_t *__restrict__ firsts_before,
                         const int64_t *__restrict__ lpos, DevModel<TC> M, TC alpha, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    int64_t nn = firsts_before ? firsts_before[r] : 0;
    int64_t nl = (M.kind == CP_MODEL_HYPEREDGE_CUT) ? lpos[r] : 0;     // rows whose last column < r
    cst[r] = dm_apply(M, alpha, r, pos[r], nn, nl);
    ptr[r] = 0;
}

// diff[0] |= "the two cost rows differ somewhere" (bitwise comparison: the tables are compared, not the values' meaning)
template <typename TC>
__global__ void __launch_bounds__(256) k_rows_differ(const TC *__restrict__ a, const TC *__restrict__ b, int64_t n1, int32_t *__restrict__ diff)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool d = false;
    if (i < n1) {
        static_assert(sizeof(TC) == 8, "cost rows are 8-byte elements");
        d = reinterpret_cast<const unsigned long long *>(a)[i] != reinterpret_cast<const unsigned long long *>(b)[i];
    }
    if (__ballot(d) && (threadIdx.x & 63) == 0) atomicOr(diff, 1);
}

template <typename TC> struct BigCost;
template <> struct BigCost<int64_t> { static __host__ __device__ int64_t v() { return (int64_t)1 << 61; } };
template <> struct BigCost<double> { static __host__ __device__ double v() { return 1152921504606846976.0; } };      // 2^60

// W[p] = cst[p] inside [lo, hi] (0-based rows), a huge value outside
template <typename TC>
__global__ void __launch_bounds__(256) k_mask_row(int64_t n1, int64_t lo, int64_t hi, const TC *__restrict__ cst, TC *__restrict__ W)
{
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n1) W[p] = (p >= lo && p <= hi) ? cst[p] : BigCost<TC>::v();
}

// is the valley search of dp_bottleneck.hip exact for this model?  Needs a cost that grows with its part: every beta >= 0
// (hyperedge cut: cost = d*b_cut + l*(b_self - b_cut) with d, l growing, so b_cut >= 0 and b_self >= b_cut).  alpha, alpha[k]
// are free.  Element type: Work / Connectivity costs are sums of terms that are EACH monotone in the part (counts times a
// non-negative beta) and IEEE addition is monotone, so non-integral Float64 parameters keep the valley.  The hyperedge cost is
// evaluated as fl(l*b_self) + fl((d-l)*b_cut) (HyperedgeCutCosts.jl:21) and its (d - l) term is NOT monotone in the part:
// with non-integral betas the rounded value can rise by an ulp while the part shrinks and the valley breaks (35 of 360 layers
// differed from the literal sweep for (0,0,0,.1,.1), (0,0,0,.7,.1), (.3,.1,0,.3,.3)).  Those go to the general sweep; with
// integer-valued parameters and totals below 2^53 every product and sum is exact and the real-number argument holds.
// Int64 costs of every kind need the bound of model_exact_on: a cost that wraps past 2^63 stops growing with its part.
static bool fast_bottleneck_ok(const cp_model_t *m, int64_t n, int64_t N, int64_t K)
{
    auto P = [&](int i) { return m->dtype == CP_I64 ? (double)m->p_i64[i] : m->p_f64[i]; };
    if (m->dtype == CP_I64 && !model_exact_on(m, n, N, K)) return false;
    if (!(P(CP_P_VERTEX) >= 0 && P(CP_P_PIN) >= 0)) return false;
    if (m->kind == CP_MODEL_WORK) return true;
    if (m->kind == CP_MODEL_CONNECTIVITY) return P(CP_P_NET) >= 0;
    // the monotonized symmetric cost is the Connectivity cost on the pattern with its diagonal added (sym.hpp): the same conditions
    if (m->kind == CP_MODEL_MONO_SYM_CONNECTIVITY) return P(CP_P_DIA_NET) >= 0;
    if (m->kind == CP_MODEL_HYPEREDGE_CUT)
        return P(CP_P_CUT_NET) >= 0 && P(CP_P_SELF_NET) >= P(CP_P_CUT_NET) && model_exact_on(m, n, N, K);
    return false;
}

// ------------------------------------------------------------------ the path decision
DpPath dp_path(const cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *m)
{
    // (force_brute: every scalable engine off)
    const bool total = combine == CP_COMBINE_SUM && !g_opt_force_brute, bottleneck = combine == CP_COMBINE_MAX && !g_opt_force_brute;
    if (model_is_env(m->kind)) {
        // never the O(n log^2 n) total scheme of dp_total.hip: the span satisfies the quadrangle inequality in neither direction.
        // The total objective in splitter order splits at the cut column instead (envelope_total.hip)
        if (bottleneck && env_valley_ok(m, A->m, A->n, A->N, K)) return DpPath::EnvValley;
        if (total && order == CP_ORDER_SPLITTER && A->n >= g_opt_env_dc_min_n && env_dc_ok(m, A->m, A->n, A->N, K)) return DpPath::EnvDc;
        CP_REQUIRE(A->n <= g_opt_brute_max_n, CP_EUNSUPPORTED,
                   "AffineEnvelopeModel: the total objective outside the divide-and-conquer gate (a non-integral Float64 model, costs past "
                   "2^60 / 2^51, n < env_dc_min_n, force_brute) and the bottleneck objective outside the valley gate (a negative beta, "
                   "wrapping Int64 costs, force_brute) run the O(n^2) device sweep: n too large");
        return DpPath::EnvSweep;
    }
    const bool sym = model_is_sym(m->kind);        // (of that family only the monotonized model passes fast_bottleneck_ok)
    if (total && fast_total_ok(m, A->n, A->N, K)) return DpPath::Total;
    // the family's total objective: both loop orders (the chunker order passes no part index: alpha_of).  sym_total_min_n is where the
    // divide and conquer overtakes the sweep; a sweep that would be refused is no competitor, so there it runs from the first n at
    // which it is a decomposition at all (below SYM_TOTAL_FLOOR columns it is one whole-row scan, which is the sweep)
    if (total && sym && g_opt_sym_total && sym_total_ok(m, A->n, A->N, K) &&
        (A->n >= g_opt_sym_total_min_n || (A->n > g_opt_brute_max_n && A->n >= SYM_TOTAL_FLOOR)))
        return DpPath::SymTotal;
    if (bottleneck && fast_bottleneck_ok(m, A->n, A->N, K)) return sym ? DpPath::SymValley : DpPath::Valley;
    CP_REQUIRE(A->n <= g_opt_brute_max_n, CP_EUNSUPPORTED,
               "model/objective outside the O(n log^2 n) class and n too large for the O(n^2) device sweep");
    return sym ? DpPath::SymSweep : DpPath::Sweep;
}

// ------------------------------------------------------------------ the driver object
// One K-layer run for cost type TC: the path, what it needs prepared, the device model, the argmin table and how a layer is launched.
// layer1() and layer() only enqueue; who waits for the stream, and when, is the entry's business (the one-shot entries never wait per
// layer).
template <typename TC>
struct DpRun : cp_dp_s {
    cp_model_t mdl{};                          // own copy (with its alphas): a step handle outlives the caller's struct
    std::vector<TC> alpha_k_host;
    HostModel<TC> HM;
    DBuf<int32_t> cnt0;                        // layer-1 scratch: stays until the stream has run layer 1
    DBuf<int64_t> firsts, scan_tmp;
    SymHost SH;                                // the symmetric paths' counters (sym_prepare)
    EnvDev ED{};                               // the envelope paths' tree (env_prepare)
    int64_t *ptr_tab = nullptr;                // host tables (n+1) x K filled by dump_layer, or null: none asked for
    TC *cst_tab = nullptr;

    size_t n1() const { return (size_t)A->n + 1; }
    int32_t *ptr_row(int64_t k) { return ptr.p + (size_t)(k - 1) * n1(); }

    void begin(cp_csr_s *A_, int64_t K_, int32_t combine_, int32_t order_, const cp_model_t *model)
    {
        A = A_; K = K_; combine = combine_; order = order_; mdl = *model;
        if (model->alpha_k && model->n_alpha_k > 0) {
            alpha_k_host.assign((const TC *)model->alpha_k, (const TC *)model->alpha_k + model->n_alpha_k);
            mdl.alpha_k = alpha_k_host.data();
        }
        path = dp_path(A, K, combine, order, &mdl);
        switch (path) {
        case DpPath::EnvValley: case DpPath::EnvDc: case DpPath::EnvSweep:
            ED = env_prepare(A);
            break;
        default:
            ensure_links(A);
            if (hyperedge()) ensure_self(A);
            if (model_is_sym(mdl.kind)) sym_prepare(A, &mdl, SH);
            if (path == DpPath::Total) work = dp_total_work_get<TC>(A);       // (kept in the matrix handle between calls)
        }
        build_dev_model<TC>(&mdl, HM, A->stream);
        ptr.alloc((size_t)K * n1());
    }
    bool hyperedge() const { return mdl.kind == CP_MODEL_HYPEREDGE_CUT; }      // the kind that reads the self-net arrays (ensure_self)

    // splitter order passes the part index (per-part alpha[k]); the chunker loop order calls f(j,j') (DynamicSplitter.jl:64)
    TC alpha_of(int64_t k) const
    {
        if (order == CP_ORDER_SPLITTER && k >= 1 && k <= (int64_t)alpha_k_host.size()) return alpha_k_host[(size_t)k - 1];
        return model_param<TC>(&mdl, CP_P_ALPHA);
    }

    // layer 1, all rows: a column scan (DynamicSplitter.jl:26-31)
    void layer1(TC *cur)
    {
        hipStream_t s = A->stream;
        const int64_t n = A->n;
        switch (path) {
        case DpPath::SymValley: case DpPath::SymTotal: case DpPath::SymSweep: sym_layer1<TC>(A, SH.d, HM.d, alpha_of(1), cur, ptr_row(1)); return;
        case DpPath::EnvValley: case DpPath::EnvDc: case DpPath::EnvSweep: env_layer1<TC>(A, ED, HM.d, alpha_of(1), cur, ptr_row(1)); return;
        default: break;                        // Total, Valley, Sweep: the column scan below
        }
        const bool has_nets = mdl.kind == CP_MODEL_CONNECTIVITY || mdl.kind == CP_MODEL_HYPEREDGE_CUT || mdl.kind == CP_MODEL_COLBLOCK;
        if (has_nets) {
            cnt0.alloc((size_t)(n > 0 ? n : 1)); firsts.alloc(n1());
            if (n > 0) hipLaunchKernelGGL(k_col_count_prev_lt, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, A->pos.p, A->prev.p, 0, cnt0.p, n);
            exclusive_scan_i32(cnt0.p, firsts.p, n, scan_tmp, s);
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_layer1<TC>), dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, n, A->pos.p,
                           has_nets ? firsts.p : nullptr, hyperedge() ? A->lpos.p : nullptr, HM.d, alpha_of(1), cur, ptr_row(1));
        CP_HIP(hipGetLastError());
    }

    // layer k >= 2, rows [rlo, rhi] (0-based), from the previous layer's cost row
    void layer(int64_t k, const TC *prev, TC *cur, int64_t rlo, int64_t rhi, const DpWindow &win = DpWindow())
    {
        switch (path) {
        case DpPath::Total:
            if (win.j0)       // a work budget: the limits [win.lo, win.hi] themselves, not the masked row (nothing outside them is read)
                dp_total_budget_layer<TC>(A, HM.d, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi, win.lo, win.hi, win.j0, win.j0_host);
            else dp_total_layer<TC>(A, HM.d, alpha_of(k), prev, cur, ptr_row(k), work, rlo, rhi, win.w);
            break;
        case DpPath::Valley:
            dp_bottleneck_layer<TC>(A, HM.d, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi, win.w, win.lo, win.hi, win.j0);
            break;
        case DpPath::SymValley: {
            // kind 11 under max: the valley search over D's links and counter, pins from overpos; the formula is Connectivity's slot for slot
            DevModel<TC> Mc = HM.d;
            Mc.kind = CP_MODEL_CONNECTIVITY;
            const SymWork *SW = sym_work_get(A);
            const BnPattern pat{SW->dpos.p, SW->dpos32.p, SW->pin32.p, SW->dprev.p, SW->dnext.p, SW->Nd, &SW->dia.d};
            dp_bottleneck_layer<TC>(A, Mc, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi, win.w, win.lo, win.hi, win.j0, &pat);
            break;
        }
        case DpPath::SymTotal: sym_total_layer<TC>(A, SH.d, HM.d, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi); break;
        case DpPath::SymSweep: sym_brute_layer<TC>(A, SH.d, HM.d, alpha_of(k), combine, prev, cur, ptr_row(k), rlo, rhi); break;
        case DpPath::EnvValley: env_valley_layer<TC>(A, ED, HM.d, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi); break;
        case DpPath::EnvDc: env_dc_layer<TC>(A, ED, HM.d, alpha_of(k), prev, cur, ptr_row(k), rlo, rhi); break;
        case DpPath::EnvSweep: env_sweep_layer<TC>(A, ED, HM.d, alpha_of(k), combine, prev, cur, ptr_row(k), rlo, rhi); break;
        case DpPath::Sweep: dp_brute_layer<TC>(A, HM.d, alpha_of(k), combine, prev, cur, ptr_row(k), rlo, rhi); break;
        }
    }

    // rows [rlo, rhi] of layer k into the host tables (waits for the stream); fill: the other rows become zeros(Ti) / fill(typemax)
    void dump_layer(int64_t k, const TC *cst_dev, int64_t rlo, int64_t rhi, bool fill)
    {
        if (!ptr_tab) return;
        hipStream_t s = A->stream;
        std::vector<TC> hc(n1());
        std::vector<int32_t> hp(n1());
        CP_HIP(hipMemcpyAsync(hc.data(), cst_dev, sizeof(TC) * n1(), hipMemcpyDeviceToHost, s));
        CP_HIP(hipMemcpyAsync(hp.data(), ptr_row(k), sizeof(int32_t) * n1(), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        int64_t *pt = ptr_tab + (size_t)(k - 1) * n1();
        TC *ct = cst_tab + (size_t)(k - 1) * n1();
        for (int64_t r = fill ? 0 : rlo; r <= (fill ? A->n : rhi); r++) {
            const bool keep = r >= rlo && r <= rhi;
            pt[r] = keep ? (int64_t)hp[(size_t)r] + 1 : 0;
            ct[r] = keep ? hc[(size_t)r] : CostTraits<TC>::typemax();
        }
    }

    // unravel_splits (DynamicSplitter.jl:89-99): K dependent single-element reads of ptr
    void unravel(int64_t *spl_out)
    {
        hipStream_t s = A->stream;
        int64_t at = A->n;
        spl_out[K] = at + 1;
        for (int64_t k = K; k >= 1; k--) {
            int32_t v = 0;
            CP_HIP(hipMemcpyAsync(&v, ptr_row(k) + at, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            at = v;
            spl_out[k - 1] = at + 1;
        }
    }

    int32_t step_layer(int64_t k, const void *prev, void *cur) override;
    int32_t block_tables(int32_t *nplanes_out, int64_t *opt_out, int64_t *nets_out, int64_t *selfnets_out) override
    {
        CP_REQUIRE(path == DpPath::Total && work, CP_EUNSUPPORTED, "block tables exist on the O(n log^2 n) path only");
        const int nb = dp_total_block_tables<TC>(A, work, opt_out, nets_out, selfnets_out);
        if (nplanes_out) *nplanes_out = nb;
        return CP_OK;
    }
};

// ------------------------------------------------------------------ the K-part DP driver (unconstrained)
template <typename TC>
static int32_t run_dynamic_t(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, int64_t *spl_out, const DpTables &tabs)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    const size_t n1 = (size_t)n + 1;
    DpRun<TC> D;
    D.begin(A, K, combine, order, mdl);
    D.ptr_tab = tabs.ptr_tab; D.cst_tab = pick<TC>(tabs.cst_i64, tabs.cst_f64);
    DBuf<TC> cstA(n1), cstB(n1);
    D.layer1(cstA.p);
    D.dump_layer(1, cstA.p, 0, n, true);
    TC *prevc = cstA.p, *curc = cstB.p;
    // cp_set_option("fixed_point", 1) -- OFF by default: a layer is a function of the previous layer's cost row alone (the model
    // does not depend on k unless per-part alphas are given), so once a full layer reproduces its input row bit for bit every
    // later layer repeats it: its argmin row is copied instead of recomputed.  Exact, but it turns K layers into two for
    // costs where empty parts are free (alpha = 0): a property of the input, kept out of the default so that timings mean
    // "K layers computed".
    const bool fp_ok = g_opt_fixed_point && !(order == CP_ORDER_SPLITTER && mdl->alpha_k && mdl->n_alpha_k > 0);
    DBuf<int32_t> diff(1);
    auto first_row = [&](int64_t k) { return k == K ? n : 0; };      // layer K: row n+1 only (DynamicSplitter.jl:34)
    for (int64_t k = 2; k <= K; k++) {
        D.layer(k, prevc, curc, first_row(k), n);
        D.dump_layer(k, curc, first_row(k), n, true);
        if (fp_ok && k < K) {
            int32_t hd = 1;
            CP_HIP(hipMemsetAsync(diff.p, 0, sizeof(int32_t), s));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rows_differ<TC>), dim3((unsigned)cdiv((int64_t)n1, 256)), dim3(256), 0, s, prevc, curc, (int64_t)n1, diff.p);
            CP_HIP(hipMemcpyAsync(&hd, diff.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            if (!hd) {                               // fixed point: layers k+1 .. K repeat layer k
                for (int64_t k2 = k + 1; k2 <= K; k2++) {
                    CP_HIP(hipMemcpyAsync(D.ptr_row(k2), D.ptr_row(k), sizeof(int32_t) * n1, hipMemcpyDeviceToDevice, s));
                    D.dump_layer(k2, curc, first_row(k2), n, true);
                }
                break;
            }
        }
        std::swap(prevc, curc);
    }
    D.unravel(spl_out);
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

int32_t run_dynamic(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, int64_t *spl_out, const DpTables &tabs)
{
    return with_cost_type(mdl->dtype, [&](auto tag) { return run_dynamic_t<decltype(tag)>(A, K, combine, order, mdl, spl_out, tabs); });
}

// ------------------------------------------------------------------ the K-part DP under a width constraint
// partition_stripe(A, K, DynamicTotal{Splitter,Chunker}(ConstrainedCost(f, VertexCount(), w_max)))   DynamicSplitter.jl:206-314.
// Layer k lives on the rows j' in [j'_lo[k], j'_hi[k]] (column_constraints :144-172; for the width weight: closed forms), its
// candidates are j in [max(j'_lo[k-1], j' - w_max), min(j', j'_hi[k-1])] (:233-246), ties -> largest j.  The previous layer's
// window enters through its cost row -- a value no real total reaches outside the window -- and the width through the windowed
// geometry of dp_total_layer; the rows are restricted to the layer's window (the row-tile mechanism of the multi-GPU path).
// The chunker loop order (:260-314) fills the same cells with the same recurrence (part_constraints :174-204 describes the
// same windows column by column) and calls the cost without the part index.
static void width_windows(int64_t n, int64_t K, int64_t w, std::vector<int64_t> &lo, std::vector<int64_t> &hi)
{
    lo.assign((size_t)K + 1, 0); hi.assign((size_t)K + 1, 0);           // 1-based k, 1-based j'
    int64_t jp = n + 1;
    for (int64_t k = K; k >= 1; k--) { lo[(size_t)k] = jp; jp = std::max<int64_t>(1, jp > w ? jp - w : 1); }
    int64_t j = 1;
    for (int64_t k = 1; k <= K; k++) { hi[(size_t)k] = (w >= n + 1 - j) ? n + 1 : j + w; j = hi[(size_t)k]; }
}

// combine = CP_COMBINE_MAX (DynamicBottleneck*(ConstrainedCost(...))): the same windows; the valley search of dp_bottleneck.hip takes
// the layer's candidate limits directly (no masked row: the crossing is searched inside [max(lo[k-1], j' - w), min(j', hi[k-1])],
// where the previous layer's costs are finite and still grow with the prefix -- dropping the last column of a feasible prefix
// keeps every width <= w).

// column_constraints (DynamicSplitter.jl:144-172) from that array: j'_lo walks back from n + 1 (:150-158, the first step taken
// unconditionally), j'_hi forward from 1 (:161-169).  1-based j', as the reference's vectors.
static void weight_windows(int64_t n, int64_t K, const std::vector<int32_t> &j0, std::vector<int64_t> &lo, std::vector<int64_t> &hi)
{
    lo.assign((size_t)K + 1, 0); hi.assign((size_t)K + 1, 0);
    int64_t jp = n + 1;
    for (int64_t k = K; k >= 1; k--) { lo[(size_t)k] = jp; jp = std::min<int64_t>(jp, (int64_t)j0[(size_t)jp - 1] + 1); }
    int64_t j = 1;
    for (int64_t k = 1; k <= K; k++) {
        // the largest j' >= j with j0(j') <= j: j0 is non-decreasing in j'
        const int64_t fit = (int64_t)(std::upper_bound(j0.begin(), j0.end(), (int32_t)(j - 1)) - j0.begin());     // #rows with j0 <= j - 1 (0-based) = the largest such j' (1-based)
        hi[(size_t)k] = std::max<int64_t>(j, fit);
        j = hi[(size_t)k];
    }
}

// route Width: parts of at most route.width columns; Weight: the monotone work weight's budget wmax_i64 / wmax_f64 through its j0 array
template <typename TC>
static int32_t run_dynamic_windowed_t(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, ConstrainedRoute route,
                                      const cp_model_t *weight, int64_t wmax_i64, double wmax_f64, int64_t *spl_out, const DpTables &tabs)
{
    CP_REQUIRE(route.kind != ConstrainedRoute::OneWave, CP_EINTERNAL, "the one-wave route has no windowed form");
    const bool by_weight = route.kind == ConstrainedRoute::Weight;
    int64_t *const ptr_tab = tabs.ptr_tab;
    TC *const cst_tab = pick<TC>(tabs.cst_i64, tabs.cst_f64);
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    const size_t n1 = (size_t)n + 1;
    std::vector<int64_t> lo, hi;
    DBuf<int32_t> j0;
    std::vector<int32_t> hj;
    if (by_weight) {                                                     // a general monotone weight: its j0 array
        CP_REQUIRE(weight && weight->kind == CP_MODEL_WORK && !weight->alpha_k, CP_EINTERNAL, "general weights: an AffineWorkModel without per-part alpha");
        j0.alloc(n1);
        const unsigned gw = (unsigned)cdiv((int64_t)n1, 256);
        if (weight->dtype == CP_I64)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_weight_j0<int64_t>), dim3(gw), dim3(256), 0, s, n, A->pos.p, weight->p_i64[CP_P_ALPHA],
                               weight->p_i64[CP_P_VERTEX], weight->p_i64[CP_P_PIN], wmax_i64, j0.p);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_weight_j0<double>), dim3(gw), dim3(256), 0, s, n, A->pos.p, weight->p_f64[CP_P_ALPHA],
                               weight->p_f64[CP_P_VERTEX], weight->p_f64[CP_P_PIN], wmax_f64, j0.p);
        CP_HIP(hipGetLastError());
        hj.resize(n1);
        CP_HIP(hipMemcpyAsync(hj.data(), j0.p, sizeof(int32_t) * n1, hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        weight_windows(n, K, hj, lo, hi);
    } else {
        width_windows(n, K, route.width, lo, hi);
    }
    if (tabs.win_lo) for (int64_t k = 1; k <= K; k++) { tabs.win_lo[k - 1] = lo[(size_t)k]; tabs.win_hi[k - 1] = hi[(size_t)k]; }
    if (ptr_tab) for (size_t i = 0; i < (size_t)K * n1; i++) { ptr_tab[i] = 0; cst_tab[i] = CostTraits<TC>::typemax(); }
    if (hi[(size_t)K] < n + 1) {                                         // infeasible (:217-222): a degenerate partition, no exception
        for (int64_t k = 0; k < K; k++) spl_out[k] = 1;
        spl_out[K] = n + 1;
        return CP_INFEASIBLE;
    }
    DpRun<TC> D;
    D.begin(A, K, combine, order, mdl);                                  // (constrained_route admitted the model: never the O(n^2) sweep)
    D.ptr_tab = ptr_tab; D.cst_tab = cst_tab;
    CP_REQUIRE(!by_weight || combine == CP_COMBINE_MAX || D.path == DpPath::Total, CP_EINTERNAL, "general weights: the total objective needs an inverse-Monge model");
    DpWindow win;
    win.w = by_weight ? 0 : std::min<int64_t>(route.width, std::max<int64_t>(n, 1));     // (wider than the matrix: every window is [0, r])
    win.j0 = j0.p; win.j0_host = by_weight ? hj.data() : nullptr;
    DBuf<TC> cst(n1), Wm(n1);
    D.layer1(cst.p);
    D.dump_layer(1, cst.p, lo[1] - 1, hi[1] - 1, false);
    for (int64_t k = 2; k <= K; k++) {
        win.lo = lo[(size_t)k - 1] - 1; win.hi = hi[(size_t)k - 1] - 1;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mask_row<TC>), dim3((unsigned)cdiv((int64_t)n1, 256)), dim3(256), 0, s, (int64_t)n1, win.lo, win.hi, cst.p, Wm.p);
        D.layer(k, Wm.p, cst.p, lo[(size_t)k] - 1, hi[(size_t)k] - 1, win);
        D.dump_layer(k, cst.p, lo[(size_t)k] - 1, hi[(size_t)k] - 1, false);
    }
    D.unravel(spl_out);                                                  // (every visited cell lies in its layer's window)
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

int32_t run_dynamic_windowed(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, ConstrainedRoute route,
                             const cp_model_t *weight, int64_t wmax_i64, double wmax_f64, int64_t *spl_out, const DpTables &tabs)
{
    return with_cost_type(mdl->dtype, [&](auto tag) {
        return run_dynamic_windowed_t<decltype(tag)>(A, K, combine, order, mdl, route, weight, wmax_i64, wmax_f64, spl_out, tabs);
    });
}

// ------------------------------------------------------------------ the route of a ConstrainedCost
// the scalable paths take: a model of the inverse-Monge class (total cost) or one the valley search is exact for (bottleneck),
// under a width w_max >= 1
static bool windowed_ok(cp_csr_s *A, int64_t K, int32_t combine, const cp_model_t *model, int64_t wmax)
{
    if (wmax < 1 || g_opt_force_brute) return false;
    if (!dp_takes_kind(model->kind, DP_KINDS_AFFINE)) return false;
    // bottleneck: the searched-crossings walk carries the candidate limits (Int64 costs; dp_bottleneck.hip)
    if (combine == CP_COMBINE_MAX) return model->dtype == CP_I64 && g_opt_bn_wave >= 2 && fast_bottleneck_ok(model, A->n, A->N, K);
    return combine == CP_COMBINE_SUM && fast_total_ok(model, A->n, A->N, K);
}

ConstrainedRoute constrained_route(cp_csr_s *A, int64_t K, int32_t combine, const cp_model_t *model, const cp_model_t *weight,
                                   int64_t wmax_i64, double wmax_f64)
{
    // width weights (VertexCount, AffineWorkModel(alpha, c, 0)): the equivalent number of columns; -2: not a width
    const int64_t wv = weight ? width_of_weight(weight, A->n, wmax_i64, wmax_f64) : wmax_i64;
    if (windowed_ok(A, K, combine, model, wv)) return {ConstrainedRoute::Width, wv};
    // bottleneck under any monotone work weight (pins, vertices + pins): the valley search with the weight's j0 array (Int64 costs only)
    if (combine == CP_COMBINE_MAX && wv == -2 && monotone_work_weight(weight) && model->dtype == CP_I64 && windowed_ok(A, K, combine, model, 1))
        return {ConstrainedRoute::Weight, 0};
    // total cost under such a weight: the two-staircase divide and conquer of dp_total_budget.hip (either cost type, both loop orders)
    if (combine == CP_COMBINE_SUM && budget_total_ok(A, K, model, weight, wmax_i64, wmax_f64)) return {ConstrainedRoute::Weight, 0};
    return {ConstrainedRoute::OneWave, 0};
}

// ------------------------------------------------------------------ row-tiled DP (one rank = one tile of rows per layer)
// cp_dp_*: the same layers as run_dynamic, but a rank computes only rows [row_lo, row_hi) of every layer and the caller
// completes the layer's cost vector with a collective (RCCL all_gather over xGMI) before the next layer.  Every step returns
// with its stream drained.
int32_t dp_begin(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *model, int64_t row_lo, int64_t row_hi,
                 cp_dp_s **out)
{
    return with_cost_type(model->dtype, [&](auto tag) -> int32_t {
        using TC = decltype(tag);
        std::unique_ptr<DpRun<TC>> D(new DpRun<TC>());
        D->begin(A, K, combine, order, model);
        D->rlo = row_lo - 1; D->rhi = row_hi - 2;
        D->lay_lo.assign((size_t)K + 1, 0); D->lay_hi.assign((size_t)K + 1, -1);      // (a layer this rank never computes owns no row)
        CP_HIP(hipMemsetAsync(D->ptr.p, 0, D->ptr.bytes(), A->stream));
        CP_HIP(hipStreamSynchronize(A->stream));
        *out = D.release();
        return CP_OK;
    });
}

template <typename TC>
int32_t DpRun<TC>::step_layer(int64_t k, const void *prev, void *cur)
{
    hipStream_t s = A->stream;
    if (k == 1) {                                  // every rank computes the whole first layer: a column scan, no exchange needed
        layer1((TC *)cur);
        CP_HIP(hipStreamSynchronize(s));
        cnt0.release(); firsts.release(); scan_tmp.release();
        return CP_OK;
    }
    CP_REQUIRE(prev && cur && k >= 2 && k <= K, CP_EINVAL, "bad layer");
    const int64_t lo = rlo < 0 ? 0 : rlo, hi = rhi > A->n ? A->n : rhi;
    lay_lo[(size_t)k] = lo; lay_hi[(size_t)k] = hi;
    if (hi >= lo) {
        CP_REQUIRE(wwin == 0 || path == DpPath::Total, CP_EUNSUPPORTED, "the width window needs the O(n log^2 n) path");
        DpWindow win;
        win.w = wwin;
        layer(k, (const TC *)prev, (TC *)cur, lo, hi, win);
    }
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

}  // namespace cpk
