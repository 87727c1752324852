// envelope.hip -- the envelope cost family (envelope.hpp) on the device: the reference's tree and the sparse table, the batched
// tree query, oracle batches, bound_stripe, and the layers of the K-part DP of DynamicSplitter.jl:15-50 in splitter order.
//
// The DP has two kernels.  The candidate sweep is the literal loop, for both objectives and any sign pattern: one lane per row, the
// wave walks the candidate column downwards and every lane keeps the running (lo, hi) of its own range, so a candidate costs one
// wave-uniform leaf load.  The valley search serves the bottleneck objective while every beta >= 0: f(j, j', k) then does not fall
// with j' and does not rise with j, the previous layer's costs do not fall, so j -> max(cst[j, k-1], f(j, j', k)) is a valley; its
// floor is at the first j with cst[j, k-1] >= f(j, j', k) or at the one before, and the reference's winner -- the largest j whose
// value is the minimum (`<=` at DynamicSplitter.jl:40) -- is found by a second binary search over the previous layer.  The total
// objective has no such path: the span satisfies the quadrangle inequality in neither direction; its scalable path
// splits the span at a cut column instead (envelope_total.hip).
#include "envelope.hpp"
#include "dp.hpp"
#include "wavelet.hpp"
#include <cmath>

namespace cpk {

int64_t g_env_valley_layers = 0;

static int32_t cllog2_e(int64_t x)
{
    int32_t h = 0;
    while (((int64_t)1 << h) < x) h++;
    return h;
}

static void env_work_free(void *w) { delete reinterpret_cast<EnvWork *>(w); }
static void env_work_reset(void *w)
{
    EnvWork *E = reinterpret_cast<EnvWork *>(w);
    E->have_tree = E->have_table = false;      // (the arrays stay allocated, as the link arrays do)
    E->dc_kv.release(); E->dc_pv.release(); E->dc_ib.release(); E->dc_bt.release(); E->dc_pa.release();      // (workspace, not a cache: dropped)
}

EnvWork *env_work_get(cp_csr_s *A)
{
    if (!A->env_work) {
        A->env_work = new EnvWork();
        A->env_work_free_fn = env_work_free;
        A->env_work_reset_fn = env_work_reset;
    }
    return reinterpret_cast<EnvWork *>(A->env_work);
}

// ------------------------------------------------------------------ the two structures
// out[c], c < cnt: the leaf of column c -- the first and the last stored entry as the reference reads them (EnvelopeMatrices.jl:15-21),
// 1-based; (m + 1, 0) for an empty column and for the padding c >= n
__global__ void __launch_bounds__(256) k_env_leaves(int64_t n, int64_t cnt, int32_t m, const int64_t *__restrict__ pos, const int32_t *__restrict__ row,
                                                    int2 *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cnt) return;
    int2 v = make_int2(m + 1, 0);
    if (c < n) {
        const int64_t q0 = pos[c], q1 = pos[c + 1];
        if (q0 < q1) v = make_int2(row[q0] + 1, row[q1 - 1] + 1);
    }
    out[c] = v;
}

// the nodes t = 2^h .. 2^(h+1) - 1 from their children 2t, 2t + 1 (:26-30); node t lives at tree[t - 1]
__global__ void __launch_bounds__(256) k_env_tree_level(int64_t first, int2 *__restrict__ tree)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= first) return;                                   // the level holds `first` = 2^h nodes
    const int64_t t = first + i;
    tree[t - 1] = env_join(tree[2 * t - 1], tree[2 * t]);
}

// table level t from level t - 1: [c, c + 2^t) = [c, c + 2^(t-1)) u [c + 2^(t-1), c + 2^t), clipped at n
__global__ void __launch_bounds__(256) k_env_table_level(int64_t n, int64_t half, const int2 *__restrict__ below, int2 *__restrict__ lev)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    int2 v = below[c];
    if (c + half < n) v = env_join(v, below[c + half]);
    lev[c] = v;
}

void ensure_env_tree(cp_csr_s *A)
{
    EnvWork *W = env_work_get(A);
    if (W->have_tree) return;
    CP_REQUIRE(A->n >= 1, CP_EINVAL, "rowenvelope needs n >= 1 (cllog2(0) has no meaning)");
    hipStream_t s = A->stream;
    const int32_t H = cllog2_e(A->n);
    const int64_t nleaf = (int64_t)1 << H;
    W->H = H;
    W->tree.ensure((size_t)(2 * nleaf - 1));
    {
        ProfScope ps(PROF_ENV_BUILD, s, 0.0);
        hipLaunchKernelGGL(k_env_leaves, dim3((unsigned)cdiv(nleaf, 256)), dim3(256), 0, s, A->n, nleaf, (int32_t)A->m, A->pos.p, A->row.p,
                           W->tree.p + (nleaf - 1));
        for (int32_t h = H - 1; h >= 0; h--) {
            const int64_t first = (int64_t)1 << h;
            hipLaunchKernelGGL(k_env_tree_level, dim3((unsigned)cdiv(first, 256)), dim3(256), 0, s, first, W->tree.p);
        }
    }
    CP_HIP(hipGetLastError());
    W->have_tree = true;
}

void ensure_env_table(cp_csr_s *A)
{
    EnvWork *W = env_work_get(A);
    if (W->have_table) return;
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    int32_t L = 0;
    while (n > 0 && ((int64_t)1 << L) <= n) L++;              // floor(log2 n) + 1
    W->L = L;
    W->table.ensure((size_t)(n > 0 ? n * L : 1));
    if (n > 0) {
        ProfScope ps(PROF_ENV_BUILD, s, 0.0);
        const unsigned g = (unsigned)cdiv(n, 256);
        hipLaunchKernelGGL(k_env_leaves, dim3(g), dim3(256), 0, s, n, n, (int32_t)A->m, A->pos.p, A->row.p, W->table.p);
        for (int32_t t = 1; t < L; t++)
            hipLaunchKernelGGL(k_env_table_level, dim3(g), dim3(256), 0, s, n, (int64_t)1 << (t - 1), W->table.p + (size_t)(t - 1) * (size_t)n,
                               W->table.p + (size_t)t * (size_t)n);
    }
    CP_HIP(hipGetLastError());
    W->have_table = true;
}

EnvDev env_prepare(cp_csr_s *A)
{
    ensure_env_table(A);
    EnvDev E;
    E.tab = env_work_get(A)->table.p; E.pos = A->pos.p; E.n = A->n; E.m = (int32_t)A->m;
    return E;
}

// getindex (EnvelopeMatrices.jl:35-57): both ends climb while j <= j'; one lane per query
__global__ void __launch_bounds__(256) k_env_query(int64_t nq, int32_t H, int32_t m, const int2 *__restrict__ tree, const int64_t *__restrict__ J,
                                                   const int64_t *__restrict__ Jp, int64_t *__restrict__ lo_out, int64_t *__restrict__ hi_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    int2 res = make_int2(m + 1, 0);
    int64_t j = (((int64_t)1 << H) - 1) + J[i], jp = (((int64_t)1 << H) - 1) + (Jp[i] - 1);
    while (j <= jp) {
        res = env_join(res, env_join(tree[j - 1], tree[jp - 1]));
        j = (j + 1) >> 1;
        jp = (jp - 1) >> 1;
    }
    lo_out[i] = res.x; hi_out[i] = res.y;
}

// ------------------------------------------------------------------ oracle batches
template <typename TC>
__global__ void __launch_bounds__(256) k_env_eval(int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ Rr, const int64_t *__restrict__ Kk,
                                                  EnvDev E, DevModel<TC> M, TC *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    out[i] = env_eval<TC>(E, M, dm_alpha(M, Kk ? Kk[i] : (int64_t)0), P[i], Rr[i]);
}

template <typename TC>
int32_t run_env_eval(cp_csr_s *A, const cp_model_t *mdl, int64_t nq, const int64_t *j, const int64_t *jp, const int64_t *k, TC *out)
{
    hipStream_t s = A->stream;
    if (nq <= 0) return CP_OK;
    std::vector<int64_t> hp((size_t)nq), hr((size_t)nq);
    for (int64_t i = 0; i < nq; i++) {
        CP_REQUIRE(j[i] >= 1 && jp[i] >= j[i] && jp[i] <= A->n + 1, CP_EINVAL, "oracle query needs 1 <= j <= j' <= n+1");
        hp[(size_t)i] = j[i] - 1; hr[(size_t)i] = jp[i] - 1;
    }
    const EnvDev E = env_prepare(A);
    DBuf<int64_t> dP((size_t)nq), dR((size_t)nq), dK;
    DBuf<TC> dO((size_t)nq);
    CP_HIP(hipMemcpyAsync(dP.p, hp.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(dR.p, hr.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    if (k) { dK.alloc((size_t)nq); CP_HIP(hipMemcpyAsync(dK.p, k, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s)); }
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    {
        ProfScope ps(PROF_QUERY, s, 0.0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_env_eval<TC>), dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, nq, dP.p, dR.p, k ? dK.p : (const int64_t *)nullptr,
                           E, HM.d, dO.p);
    }
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(out, dO.p, sizeof(TC) * (size_t)nq, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

// ------------------------------------------------------------------ bound_stripe
static int64_t env_fld(int64_t a, int64_t b)
{
    int64_t q = a / b, r = a % b;
    if (r != 0 && ((r < 0) != (b < 0))) q -= 1;
    return q;
}
static double env_fld(double a, int64_t b) { return std::floor(a / (double)b); }

// the model form (EnvelopeCosts.jl:43-53), for the model and for its oracle alike: the oracle form (:31-41) calls ocl(1, n + 1),
// which has no method, and evidently means this value.  Reads the scalar alpha: the reference's model has no alpha[k].
template <typename TC>
int32_t env_bound_stripe(cp_csr_s *A, int64_t K, const cp_model_t *mdl, TC *lo, TC *hi)
{
    const TC a = model_param<TC>(mdl, CP_P_ALPHA), bv = model_param<TC>(mdl, CP_P_VERTEX), bp = model_param<TC>(mdl, CP_P_PIN),
             bn = model_param<TC>(mdl, CP_P_NET);
    CP_REQUIRE(bv >= 0 && bp >= 0 && bn >= 0, CP_EINVAL, "bound_stripe asserts beta >= 0");      // (a NaN fails it too)
    CP_REQUIRE(A->N > 0, CP_EINVAL, "bound_stripe(AffineEnvelopeModel): a pattern without nonzeros has no row extrema");
    CP_HIP(hipSetDevice(A->device));
    const EnvDev E = env_prepare(A);
    const int64_t n = A->n;
    int t = 0;
    while (((int64_t)2 << t) <= n) t++;                        // floor(log2 n)
    int2 e[2];
    CP_HIP(hipMemcpyAsync(&e[0], E.tab + (size_t)t * (size_t)n, sizeof(int2), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipMemcpyAsync(&e[1], E.tab + (size_t)t * (size_t)n + (size_t)(n - ((int64_t)1 << t)), sizeof(int2), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipStreamSynchronize(A->stream));
    const int64_t d = (int64_t)std::max(e[0].y, e[1].y) - (int64_t)std::min(e[0].x, e[1].x);      // extrema(A.rowval): hi - lo
    *hi = cadd(cadd(cadd(a, cmulc(n, bv)), cmulc(A->N, bp)), cmulc(d, bn));
    *lo = cadd(a, env_fld(cadd(cadd(cmulc(n, bv), cmulc(A->N, bp)), cmulc(d, bn)), K));
    return CP_OK;
}

// ------------------------------------------------------------------ the K-part DP
// Float64: finite parameters and every beta >= 0 -- rounded addition is monotone, every term is a non-negative beta times a count
// that grows with the range, max is exact.  Int64: beta >= 0 and no sum that can wrap: K*max|alpha| + n*b_vertex + N*b_pin +
// m*b_net < 2^60, in the style of model_exact_on.
bool env_valley_ok(const cp_model_t *m, int64_t m_rows, int64_t n, int64_t N, int64_t K)
{
    if (m->dtype == CP_I64) {
        if (m->p_i64[CP_P_VERTEX] < 0 || m->p_i64[CP_P_PIN] < 0 || m->p_i64[CP_P_NET] < 0) return false;
        u128 amax = mag128(m->p_i64[CP_P_ALPHA]);
        if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
        const u128 bound = amax * (u128)(K > 0 ? K : 1) + (u128)m->p_i64[CP_P_VERTEX] * (u128)(n > 0 ? n : 0) +
                           (u128)m->p_i64[CP_P_PIN] * (u128)(N > 0 ? N : 0) + (u128)m->p_i64[CP_P_NET] * (u128)(m_rows > 0 ? m_rows : 0);
        return bound < ((u128)1 << 60);
    }
    for (int i = 0; i <= CP_P_NET; i++) if (!std::isfinite(m->p_f64[i])) return false;
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) if (!std::isfinite(((const double *)m->alpha_k)[i])) return false;
    return m->p_f64[CP_P_VERTEX] >= 0 && m->p_f64[CP_P_PIN] >= 0 && m->p_f64[CP_P_NET] >= 0;
}

// layer 1: cst[j', 1] = f(1, j', 1)  (DynamicSplitter.jl:26-31)
template <typename TC>
__global__ void __launch_bounds__(256) k_env_layer1(EnvDev E, DevModel<TC> M, TC alpha, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > E.n) return;
    cst[r] = env_eval<TC>(E, M, alpha, 0, r);
    ptr[r] = 0;
}

// the literal candidate sweep: 64 rows per wave walk the candidates p downwards together; column p's leaf is a wave-uniform load
// that every lane whose range holds the column folds into its running (lo, hi).  A candidate replaces the incumbent only when
// strictly better, so among equal values the largest p wins, as in k_brute_layer.
template <typename TC>
__global__ void __launch_bounds__(256) k_env_sweep(int64_t r_lo, int64_t r_hi, EnvDev E, DevModel<TC> M, TC alpha, int32_t g,
                                                   const TC *__restrict__ W, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t r0 = r_lo + wave * 64;
    if (r0 > r_hi) return;
    int64_t r = r0 + lane;
    const bool live = r <= r_hi;
    const int64_t rtop = r0 + 63 < r_hi ? r0 + 63 : r_hi;
    if (!live) r = rtop;                                       // (idle lanes evaluate in bounds and store nothing)
    const int64_t posr = E.pos[r];
    int32_t lo = E.m + 1, hi = 0;
    TC best = (TC)0;
    int64_t bp = -1;
    for (int64_t p = rtop; p >= 0; p--) {
        if (p < rtop) {                                        // (p < rtop <= n: a column)
            const int2 leaf = E.tab[p];
            if (p < r) { lo = leaf.x < lo ? leaf.x : lo; hi = leaf.y > hi ? leaf.y : hi; }
        }
        if (r >= p) {
            const int64_t d = (int64_t)hi - (int64_t)lo;
            const TC v = comb(g, W[p], env_apply(M.p, alpha, r - p, posr - E.pos[p], d > 0 ? d : (int64_t)0));
            if (bp < 0 || v < best) { best = v; bp = p; }
        }
    }
    if (live) { cst[r] = best; ptr[r] = (int32_t)bp; }
}

// the valley search, one lane per row: the first p in [0, r] with W[p] >= f(p, r) (none: r + 1), the floor there or one before,
// then the largest p of that value -- right of the crossing the value is W[p], which does not fall
template <typename TC>
__global__ void __launch_bounds__(256) k_env_valley(int64_t r_lo, int64_t r_hi, EnvDev E, DevModel<TC> M, TC alpha, const TC *__restrict__ W,
                                                    TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    const int64_t r = r_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > r_hi) return;
    int64_t lo = 0, hi = r + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (W[mid] >= env_eval<TC>(E, M, alpha, mid, r)) hi = mid; else lo = mid + 1;
    }
    const int64_t ps = lo;
    const bool has_r = ps <= r, has_l = ps > 0;
    const TC vr = has_r ? W[ps] : (TC)0;
    const TC vl = has_l ? env_eval<TC>(E, M, alpha, ps - 1, r) : (TC)0;      // left of the crossing the value is f: W[ps - 1] < f(ps - 1, r)
    TC best;
    int64_t bp;
    if (has_r && (!has_l || vr <= vl)) {
        lo = ps; hi = r;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (W[mid] <= vr) lo = mid; else hi = mid - 1;
        }
        best = vr; bp = lo;
    } else {
        best = vl; bp = ps - 1;
    }
    cst[r] = best; ptr[r] = (int32_t)bp;
}

template <typename TC>
void env_layer1(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, TC *cst, int32_t *ptr)
{
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_env_layer1<TC>), dim3((unsigned)cdiv(A->n + 1, 256)), dim3(256), 0, A->stream, E, M, alpha, cst, ptr);
    CP_HIP(hipGetLastError());
}

template <typename TC>
void env_sweep_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, int32_t combine, const TC *W, TC *cst, int32_t *ptr,
                     int64_t r_lo, int64_t r_hi)
{
    if (r_hi < r_lo) return;
    const int64_t waves = cdiv(r_hi - r_lo + 1, (int64_t)64);
    ProfScope ps(PROF_ENV_SWEEP, A->stream, 0.0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_env_sweep<TC>), dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, A->stream, r_lo, r_hi, E, M, alpha, combine, W,
                       cst, ptr);
    CP_HIP(hipGetLastError());
}

template <typename TC>
void env_valley_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst, int32_t *ptr, int64_t r_lo, int64_t r_hi)
{
    if (r_hi < r_lo) return;
    g_env_valley_layers++;
    ProfScope ps(PROF_ENV_VALLEY, A->stream, 0.0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_env_valley<TC>), dim3((unsigned)cdiv(r_hi - r_lo + 1, 256)), dim3(256), 0, A->stream, r_lo, r_hi, E, M, alpha, W,
                       cst, ptr);
    CP_HIP(hipGetLastError());
}

template int32_t run_env_eval<int64_t>(cp_csr_s *, const cp_model_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t *);
template int32_t run_env_eval<double>(cp_csr_s *, const cp_model_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, double *);
template int32_t env_bound_stripe<int64_t>(cp_csr_s *, int64_t, const cp_model_t *, int64_t *, int64_t *);
template int32_t env_bound_stripe<double>(cp_csr_s *, int64_t, const cp_model_t *, double *, double *);
template void env_layer1<int64_t>(cp_csr_s *, const EnvDev &, const DevModel<int64_t> &, int64_t, int64_t *, int32_t *);
template void env_layer1<double>(cp_csr_s *, const EnvDev &, const DevModel<double> &, double, double *, int32_t *);
template void env_sweep_layer<int64_t>(cp_csr_s *, const EnvDev &, const DevModel<int64_t> &, int64_t, int32_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void env_sweep_layer<double>(cp_csr_s *, const EnvDev &, const DevModel<double> &, double, int32_t, const double *, double *, int32_t *, int64_t, int64_t);
template void env_valley_layer<int64_t>(cp_csr_s *, const EnvDev &, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void env_valley_layer<double>(cp_csr_s *, const EnvDev &, const DevModel<double> &, double, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk

using namespace cpk;

// ------------------------------------------------------------------ rowenvelope through the C ABI
// The handle is a cp_count_t of kind CP_COUNT_ENVELOPE: it names the matrix whose cache holds the tree, so cp_count_destroy frees
// it as well, and cp_count_query refuses it.
extern "C" {

int32_t cp_envelope_build(cp_csr_t A, cp_count_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(A->device));
        ensure_env_tree(A);
        CP_HIP(hipStreamSynchronize(A->stream));
        prof_collect();
        cp_count_s *h = new cp_count_s();
        h->A = A; h->kind = CP_COUNT_ENVELOPE;
        *out = h;
        return CP_OK;
    });
}

int32_t cp_envelope_query(cp_count_t h, int64_t nq, const int64_t *j, const int64_t *jp, int64_t *lo_out, int64_t *hi_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(h && h->kind == CP_COUNT_ENVELOPE && (nq == 0 || (j && jp && lo_out && hi_out)), CP_EINVAL, "bad argument");
        if (nq <= 0) return CP_OK;
        cp_csr_s *A = h->A;
        for (int64_t i = 0; i < nq; i++) CP_REQUIRE(j[i] >= 1 && jp[i] >= j[i] && jp[i] <= A->n + 1, CP_EINVAL, "env[j, j'] needs 1 <= j <= j' <= n+1");
        CP_HIP(hipSetDevice(A->device));
        hipStream_t s = A->stream;
        ensure_env_tree(A);                                    // (again after cp_csr_reset_cache)
        const EnvWork *W = env_work_get(A);
        DBuf<int64_t> dj((size_t)nq), djp((size_t)nq), dlo((size_t)nq), dhi((size_t)nq);
        CP_HIP(hipMemcpyAsync(dj.p, j, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
        CP_HIP(hipMemcpyAsync(djp.p, jp, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
        {
            ProfScope ps(PROF_QUERY, s, 0.0);
            hipLaunchKernelGGL(k_env_query, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, nq, W->H, (int32_t)A->m, W->tree.p, dj.p, djp.p, dlo.p, dhi.p);
        }
        CP_HIP(hipGetLastError());
        CP_HIP(hipMemcpyAsync(lo_out, dlo.p, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        CP_HIP(hipMemcpyAsync(hi_out, dhi.p, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        prof_collect();
        return CP_OK;
    });
}

int32_t cp_envelope_tree(cp_count_t h, int64_t *dims_out, int64_t *tree_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(h && h->kind == CP_COUNT_ENVELOPE && dims_out, CP_EINVAL, "bad argument");
        cp_csr_s *A = h->A;
        CP_HIP(hipSetDevice(A->device));
        ensure_env_tree(A);
        const EnvWork *W = env_work_get(A);
        dims_out[0] = W->H; dims_out[1] = A->m; dims_out[2] = A->n;
        if (!tree_out) { CP_HIP(hipStreamSynchronize(A->stream)); return CP_OK; }
        const size_t nodes = ((size_t)2 << W->H) - 1;
        std::vector<int2> ht(nodes);
        CP_HIP(hipMemcpyAsync(ht.data(), W->tree.p, sizeof(int2) * nodes, hipMemcpyDeviceToHost, A->stream));
        CP_HIP(hipStreamSynchronize(A->stream));
        for (size_t t = 0; t < nodes; t++) { tree_out[2 * t] = ht[t].x; tree_out[2 * t + 1] = ht[t].y; }
        return CP_OK;
    });
}

int32_t cp_envelope_destroy(cp_count_t h)
{
    if (h) delete h;
    return CP_OK;
}

}  // extern "C"
