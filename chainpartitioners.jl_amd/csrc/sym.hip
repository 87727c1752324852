// sym.hip -- device construction of the dianet / selfpin counters and the oracle, DP-layer and count entry points of the
// symmetric cost family (sym.hpp).
#include "sym.hpp"
#include "dp.hpp"
#include <rocprim/rocprim.hpp>

namespace cpk {

static int32_t cllog2_s(int64_t x)
{
    int32_t h = 0;
    while (((int64_t)1 << h) < x) h++;
    return h;
}

static void sym_work_free(void *w) { delete reinterpret_cast<SymWork *>(w); }
static void sym_work_reset(void *w)
{
    SymWork *S = reinterpret_cast<SymWork *>(w);
    S->have_d = S->have_dia = S->have_selfpin = S->have_net = S->have_pin = false;      // (the arrays stay allocated, as the link arrays do)
}

SymWork *sym_work_get(cp_csr_s *A)
{
    if (!A->sym_work) {
        A->sym_work = new SymWork();
        A->sym_work_free_fn = sym_work_free;
        A->sym_work_reset_fn = sym_work_reset;
    }
    return reinterpret_cast<SymWork *>(A->sym_work);
}

// ------------------------------------------------------------------ the derived pattern D
// Row c's entries are tq[tpos[c] .. tpos[c+1]) in ascending column order (the stable (row, column) sort of ensure_links): one
// binary search per column finds whether A holds (c, c) and the last column before c that holds row c.
__global__ void k_sym_diag(int64_t n, const int64_t *__restrict__ tpos, const int32_t *__restrict__ tq, const int32_t *__restrict__ col,
                           int32_t *__restrict__ miss, int32_t *__restrict__ diaprev, int32_t *__restrict__ dianext)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int64_t s0 = tpos[c], s1 = tpos[c + 1];
    int64_t lo = s0, hi = s1;                                 // first entry of the row in a column >= c
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (col[tq[mid]] < (int32_t)c) lo = mid + 1; else hi = mid;
    }
    miss[c] = (lo < s1 && col[tq[lo]] == (int32_t)c) ? 0 : 1;
    diaprev[c] = lo > s0 ? col[tq[lo - 1]] : -1;
    dianext[c] = lo < s1 ? col[tq[lo]] : (int32_t)n;          // (read only where the diagonal is missing: then this column is > c)
}

// an entry (i, c) of A: D's column i holds row i, so for i < c the previous column is at least i (hst[i] after `hst[j] = j`, :89)
__global__ void k_sym_dprev(int64_t N, const int32_t *__restrict__ col, const int32_t *__restrict__ row, const int32_t *__restrict__ prev,
                            const int32_t *__restrict__ next, const int64_t *__restrict__ off, int32_t *__restrict__ dprev, int32_t *__restrict__ dnext)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    const int32_t c = col[q], i = row[q];
    int32_t pv = prev[q], nx = next[q];
    if (i < c && pv < i) pv = i;
    if (i > c && nx > i) nx = i;                              // ... and for i > c the next one is at most i
    dprev[q + off[c]] = pv;
    dnext[q + off[c]] = nx;
}

// column pointer of D and the appended diagonal entries (the last entry of their column)
__global__ void k_sym_dpos(int64_t n, const int64_t *__restrict__ pos, const int64_t *__restrict__ off, const int32_t *__restrict__ miss,
                           const int32_t *__restrict__ diaprev, const int32_t *__restrict__ dianext, int64_t *__restrict__ dpos,
                           int32_t *__restrict__ dpos32, int32_t *__restrict__ dprev, int32_t *__restrict__ dnext)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n) return;
    const int64_t d = pos[c] + off[c];
    dpos[c] = d; dpos32[c] = (int32_t)d;
    if (c < n && miss[c]) { dprev[pos[c + 1] + off[c]] = diaprev[c]; dnext[pos[c + 1] + off[c]] = dianext[c]; }
}

__global__ void k_sym_keys(const int32_t *__restrict__ dprev, int32_t *__restrict__ keys, int64_t Nd, int32_t n)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < Nd) keys[q] = n - dprev[q];                       // idx'[q'] = (n+1) - hst[i]  (SparseColorArrays.jl:83, :88)
}

void ensure_sym_links(cp_csr_s *A)
{
    SymWork *S = sym_work_get(A);
    if (S->have_d) return;
    CP_REQUIRE(A->m == A->n, CP_EINVAL, "the symmetric counters need a square pattern");
    CP_REQUIRE(A->N + A->n < ((int64_t)1 << 31) - 1, CP_EUNSUPPORTED, "nnz + n exceeds the 32-bit layout of the dianet keys");
    ensure_links(A);
    hipStream_t s = A->stream;
    const int64_t n = A->n, N = A->N;
    ProfScope ps(PROF_LINKS, s, 12.0 * (double)N + 20.0 * (double)(n + 1));
    DBuf<int32_t> miss((size_t)(n > 0 ? n : 1)), diaprev((size_t)(n > 0 ? n : 1)), dianext((size_t)(n > 0 ? n : 1));
    DBuf<int64_t> off((size_t)n + 1), scratch;
    if (n > 0) hipLaunchKernelGGL(k_sym_diag, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, n, A->tpos.p, A->tq.p, A->col.p, miss.p, diaprev.p, dianext.p);
    exclusive_scan_i32(miss.p, off.p, n, scratch, s);
    int64_t nmiss = 0;
    CP_HIP(hipMemcpyAsync(&nmiss, off.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    S->Nd = N + nmiss;
    S->dpos.ensure((size_t)n + 1); S->dpos32.ensure((size_t)n + 1);
    S->dprev.ensure((size_t)(S->Nd > 0 ? S->Nd : 1) + 16); S->dnext.ensure((size_t)(S->Nd > 0 ? S->Nd : 1) + 16);
    if (N > 0) hipLaunchKernelGGL(k_sym_dprev, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, N, A->col.p, A->row.p, A->prev.p, A->next.p, off.p,
                                  S->dprev.p, S->dnext.p);
    hipLaunchKernelGGL(k_sym_dpos, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, n, A->pos.p, off.p, miss.p, diaprev.p, dianext.p, S->dpos.p,
                       S->dpos32.p, S->dprev.p, S->dnext.p);
    CP_HIP(hipGetLastError());
    CP_HIP(hipStreamSynchronize(s));      // miss / diaprev / off die here
    S->have_d = true;
}

void build_dianet_counter(cp_csr_s *A, WaveletHost &out)
{
    ensure_sym_links(A);
    SymWork *S = sym_work_get(A);
    hipStream_t s = A->stream;
    const int64_t Nd = S->Nd;
    DBuf<int32_t> keys((size_t)(Nd > 0 ? Nd : 1));
    if (Nd > 0) hipLaunchKernelGGL(k_sym_keys, dim3((unsigned)cdiv(Nd, 256)), dim3(256), 0, s, S->dprev.p, keys.p, Nd, (int32_t)A->n);
    wavelet_build(out, keys, Nd, cllog2_s(A->n + 2), s, (int32_t)(A->n + 1));      // key n + 1: the first occurrence of a row
}

// ------------------------------------------------------------------ selfpin: points (n+1 - min(i,j), max(i,j)) bucketed by max(i,j)
__global__ void k_sp_pairs(int64_t N, const int32_t *__restrict__ col, const int32_t *__restrict__ row, uint32_t *__restrict__ kmax,
                           uint32_t *__restrict__ val, int32_t n)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    const int32_t c = col[q], i = row[q];
    kmax[q] = (uint32_t)(c > i ? c : i);
    val[q] = (uint32_t)(n - (c < i ? c : i));                 // idx'[q'] = (n+1) - min  (SparseColorArrays.jl:304), 1-based min
}
// out[r] = first sorted position whose key >= r, r = 0..n
__global__ void k_sp_starts(const uint32_t *__restrict__ skey, int64_t *__restrict__ out, int64_t n, int64_t N)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)skey[mid] < r) lo = mid + 1; else hi = mid;
    }
    out[r] = lo;
}

void build_selfpin_counter(cp_csr_s *A, WaveletHost &out, DBuf<int64_t> &spos)
{
    CP_REQUIRE(A->m == A->n, CP_EINVAL, "the symmetric counters need a square pattern");
    ensure_links(A);                                          // col[q]
    hipStream_t s = A->stream;
    const int64_t n = A->n, N = A->N;
    const size_t Na = (size_t)(N > 0 ? N : 1);
    spos.ensure((size_t)n + 1);
    DBuf<int32_t> keys(Na);
    DBuf<uint32_t> kin(Na), kout(Na), vin(Na);
    if (N > 0) {
        hipLaunchKernelGGL(k_sp_pairs, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, N, A->col.p, A->row.p, kin.p, vin.p, (int32_t)n);
        unsigned end_bit = 1;
        while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)(n > 1 ? n : 2)) end_bit++;
        size_t tmp_bytes = 0;                                 // a stable sort: the order inside a bucket is the reference's (:299-307)
        CP_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin.p, kout.p, vin.p, (uint32_t *)keys.p, (size_t)N, 0u, end_bit, s));
        DBuf<char> tmp(tmp_bytes > 0 ? tmp_bytes : 1);
        CP_HIP(rocprim::radix_sort_pairs((void *)tmp.p, tmp_bytes, kin.p, kout.p, vin.p, (uint32_t *)keys.p, (size_t)N, 0u, end_bit, s));
        hipLaunchKernelGGL(k_sp_starts, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, kout.p, spos.p, n, N);
        CP_HIP(hipGetLastError());
        CP_HIP(hipStreamSynchronize(s));                      // tmp dies here
    } else {
        CP_HIP(hipMemsetAsync(spos.p, 0, sizeof(int64_t) * ((size_t)n + 1), s));
    }
    wavelet_build(out, keys, N, cllog2_s(n + 2), s);          // (synchronises: kin / kout / vin die after it)
}

// ------------------------------------------------------------------ one call's view
__global__ void k_over_deg(int64_t n, const int64_t *__restrict__ pos, int64_t delta, int32_t *__restrict__ out)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int64_t d = (pos[c + 1] - pos[c]) - delta;          // max(deg - Delta_pins, 0)  (MonotonizedSymmetricConnectivityCosts.jl:85)
    out[c] = (int32_t)(d > 0 ? d : 0);
}

void sym_prepare(cp_csr_s *A, const cp_model_t *mdl, SymHost &H, bool counters)
{
    CP_REQUIRE(model_is_sym(mdl->kind), CP_EINTERNAL, "not a symmetric model");
    CP_REQUIRE(A->m == A->n, CP_EINVAL, "the symmetric cost models need a square pattern (the reference asserts m == n)");
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    SymWork *S = sym_work_get(A);
    H.d.kind = mdl->kind; H.d.n = n; H.d.pos = A->pos.p;
    if (counters && (mdl->kind == CP_MODEL_SYM_CONNECTIVITY || mdl->kind == CP_MODEL_MONO_SYM_CONNECTIVITY)) {
        if (!S->have_dia) { build_dianet_counter(A, S->dia); S->have_dia = true; }
        H.d.dpos = S->dpos.p; H.d.dia = S->dia.d;
    }
    if (counters && mdl->kind == CP_MODEL_SYM_CONNECTIVITY) {
        if (!S->have_net) { ensure_net_counter(A, S->net); S->have_net = true; }
        H.d.net = S->net.d;
    }
    if (counters && mdl->kind == CP_MODEL_SYM_EDGE_CUT) {
        if (!S->have_selfpin) { build_selfpin_counter(A, S->selfpin, S->spos); S->have_selfpin = true; }
        H.d.spos = S->spos.p; H.d.selfpin = S->selfpin.d;
    }
    if (mdl->kind == CP_MODEL_MONO_SYM_CONNECTIVITY) {
        // overpos is a Vector{Ti} in the reference: a Delta_pins that is not an integer has no such vector
        int64_t delta = 0;
        if (mdl->dtype == CP_I64) delta = mdl->p_i64[CP_P_DELTA_PINS];
        else {
            const double v = mdl->p_f64[CP_P_DELTA_PINS];
            CP_REQUIRE(std::floor(v) == v && std::fabs(v) <= 4611686018427387904.0, CP_EINVAL, "Delta_pins must be integer-valued");
            delta = (int64_t)v;
        }
        const int64_t lim = (int64_t)1 << 31;                 // beyond a column's possible length the value no longer matters
        if (delta > lim) delta = lim;
        CP_REQUIRE(delta >= -((int64_t)1 << 30), CP_EUNSUPPORTED, "Delta_pins below -2^30");
        if (!S->have_pin || S->pin_delta != delta) {          // (kept per matrix: the bound and the partition of one call share it)
            S->have_pin = false;
            DBuf<int32_t> od((size_t)(n > 0 ? n : 1));
            DBuf<int64_t> scratch;
            S->pin.ensure((size_t)n + 1); S->pin32.ensure((size_t)n + 1);
            if (n > 0) hipLaunchKernelGGL(k_over_deg, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, n, A->pos.p, delta, od.p);
            exclusive_scan_i32(od.p, S->pin.p, n, scratch, s);
            hipLaunchKernelGGL(k_narrow, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, S->pin.p, S->pin32.p, n + 1);
            CP_HIP(hipGetLastError());
            CP_HIP(hipMemcpyAsync(&S->over_total, S->pin.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));                  // od / scratch die here
            S->pin_delta = delta; S->have_pin = true;
        }
        CP_REQUIRE(S->over_total < ((int64_t)1 << 31) - 1, CP_EUNSUPPORTED, "over-pin total exceeds the 32-bit layout");
        H.over_total = S->over_total; H.pin32 = S->pin32.p;
        H.d.pin = S->pin.p;
    }
}

// ------------------------------------------------------------------ ocl(j, j', k) batches
template <typename TC>
__global__ void k_sym_eval(SymDev S, DevModel<TC> M, int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ R,
                           const int64_t *__restrict__ Kk, TC *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    out[i] = sym_eval<TC>(S, M, dm_alpha(M, Kk ? Kk[i] : (int64_t)0), P[i], R[i]);
}

template <typename TC>
int32_t run_sym_eval(cp_csr_s *A, const cp_model_t *mdl, int64_t nq, const int64_t *j, const int64_t *jp, const int64_t *k, TC *out)
{
    hipStream_t s = A->stream;
    SymHost H;
    sym_prepare(A, mdl, H);                                   // (also for nq == 0: a non-square pattern is refused either way)
    if (nq <= 0) return CP_OK;
    std::vector<int64_t> hp((size_t)nq), hr((size_t)nq);
    for (int64_t i = 0; i < nq; i++) {
        CP_REQUIRE(j[i] >= 1 && jp[i] >= j[i] && jp[i] <= A->n + 1, CP_EINVAL, "oracle query needs 1 <= j <= j' <= n+1");
        hp[(size_t)i] = j[i] - 1; hr[(size_t)i] = jp[i] - 1;
    }
    DBuf<int64_t> dP((size_t)nq), dR((size_t)nq), dK;
    DBuf<TC> dO((size_t)nq);
    CP_HIP(hipMemcpyAsync(dP.p, hp.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(dR.p, hr.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    if (k) { dK.alloc((size_t)nq); CP_HIP(hipMemcpyAsync(dK.p, k, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s)); }
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    {
        ProfScope ps(PROF_QUERY, s, 0.0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sym_eval<TC>), dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, H.d, HM.d, nq, dP.p, dR.p,
                           k ? dK.p : nullptr, dO.p);
    }
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(out, dO.p, sizeof(TC) * (size_t)nq, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}
template int32_t run_sym_eval<int64_t>(cp_csr_s *, const cp_model_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t *);
template int32_t run_sym_eval<double>(cp_csr_s *, const cp_model_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, double *);

// ------------------------------------------------------------------ DP layers: the literal candidate sweep of DynamicSplitter.jl:26-46
template <typename TC>
__global__ void k_sym_layer1(SymDev S, DevModel<TC> M, TC alpha, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > S.n) return;
    cst[r] = sym_eval<TC>(S, M, alpha, (int64_t)0, r);
    ptr[r] = 0;
}

// One wave per row r: lane l takes the candidates p = r - l, r - l - 64, ... downwards and keeps a strictly better one only;
// the wave then keeps the smallest value and, among equal values, the largest p -- the candidate the reference's upward scan with
// `<=` ends on (DynamicSplitter.jl:37-43).
template <typename TC>
__global__ void __launch_bounds__(256) k_sym_brute_layer(SymDev S, DevModel<TC> M, TC alpha, int32_t g, int64_t r_lo, int64_t r_hi,
                                                         const TC *__restrict__ W, TC *__restrict__ cst, int32_t *__restrict__ ptr)
{
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t r = r_lo + wave;
    if (r > r_hi) return;
    TC best = (TC)0;
    int64_t bp = -1;
    for (int64_t p = r - lane; p >= 0; p -= 64) {
        const TC v = comb(g, W[p], sym_eval<TC>(S, M, alpha, p, r));
        if (bp < 0 || v < best) { best = v; bp = p; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const TC ov = __shfl_down(best, o);
        const int64_t op = __shfl_down(bp, o);
        if (op >= 0 && (bp < 0 || ov < best || (ov == best && op > bp))) { best = ov; bp = op; }
    }
    if (lane == 0) { cst[r] = best; ptr[r] = (int32_t)bp; }
}

template <typename TC>
void sym_layer1(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, TC *cst, int32_t *ptr)
{
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sym_layer1<TC>), dim3((unsigned)cdiv(A->n + 1, 256)), dim3(256), 0, A->stream, S, M, alpha, cst, ptr);
    CP_HIP(hipGetLastError());
}

template <typename TC>
void sym_brute_layer(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, int32_t combine, const TC *W, TC *cst_out,
                     int32_t *ptr_out, int64_t r_lo, int64_t r_hi)
{
    if (r_hi < r_lo) return;
    hipStream_t s = A->stream;
    ProfScope ps(PROF_BRUTE, s, 0.0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sym_brute_layer<TC>), dim3((unsigned)cdiv(r_hi - r_lo + 1, 4)), dim3(256), 0, s, S, M, alpha, combine,
                       r_lo, r_hi, W, cst_out, ptr_out);
    CP_HIP(hipGetLastError());
}

template void sym_layer1<int64_t>(cp_csr_s *, const SymDev &, const DevModel<int64_t> &, int64_t, int64_t *, int32_t *);
template void sym_layer1<double>(cp_csr_s *, const SymDev &, const DevModel<double> &, double, double *, int32_t *);
template void sym_brute_layer<int64_t>(cp_csr_s *, const SymDev &, const DevModel<int64_t> &, int64_t, int32_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void sym_brute_layer<double>(cp_csr_s *, const SymDev &, const DevModel<double> &, double, int32_t, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk
