// plaid_cut.hip -- the plaid edge-cut costs (cut.hpp) on the device: oracle batches, the three bound_stripe forms, and the K-part DP
// of DynamicSplitter.jl:15-50 in splitter order.
//
// For a fixed part k the cost of a column range is a difference of prefix values: with L_k[c] the entries of the columns < c whose
// row part k owns,
//   primary    f(p, r, k) = alpha_k + S_k[r] - S_k[p],   S_k[c] = c*b_vertex + L_k[c]*b_self_pin + (pos[c] - L_k[c])*b_cut_pin
//   secondary  f(p, r, k) = const_k + S_k[r] - S_k[p],   S_k[c] = L_k[c]*b_self_pin - L_k[c]*b_cut_pin,
//                                                        const_k = alpha_k + nv_k*b_vertex + w_k*b_cut_pin
// so a total-cost layer cst[r] = min_p W[p] + f(p, r, k) is const_k + S_k[r] + (prefix minimum of W[p] - S_k[p] over p <= r), the
// largest minimising p winning ties (DynamicSplitter.jl:40): one scan of n + 1 values per layer.  That reassociates the sums, so it
// runs only while every value is the true integer (cut_scan_exact); everything else takes the literal candidate sweep.
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include "cut.hpp"
#include <vector>

namespace cpk {

int64_t g_cut_scan_layers = 0;

template <typename TC>
__device__ __forceinline__ TC cut_f(const CutLayer<TC> &Y, const int64_t *__restrict__ pos, const int32_t *__restrict__ Lc, int64_t p, int64_t r)
{
    const int64_t l = (int64_t)Lc[r] - Lc[p];
    if (Y.secondary) return cut_apply(Y.p, Y.alpha, Y.nvk, l, Y.wk - l);
    return cut_apply(Y.p, Y.alpha, r - p, l, (pos[r] - pos[p]) - l);
}

template <typename TC>
__device__ __forceinline__ TC cut_S(const CutLayer<TC> &Y, const int64_t *__restrict__ pos, const int32_t *__restrict__ Lc, int64_t c)
{
    const int64_t L = Lc[c];
    if (Y.secondary) return cadd(cmulc(L, Y.p[CP_P_SELF_PIN]), cmulc(-L, Y.p[CP_P_CUT_PIN]));
    return cadd(cadd(cmulc(c, Y.p[CP_P_VERTEX]), cmulc(L, Y.p[CP_P_SELF_PIN])), cmulc(pos[c] - L, Y.p[CP_P_CUT_PIN]));
}

// ------------------------------------------------------------------ oracle batches
// one wave per query: the entries of the columns [p, r) whose row part k owns
__global__ void __launch_bounds__(256) k_cut_counts(int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ Rr,
                                                    const int64_t *__restrict__ Kk, const int64_t *__restrict__ pos,
                                                    const int32_t *__restrict__ row, const int32_t *__restrict__ owner, int64_t *__restrict__ out_l)
{
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (i >= nq) return;
    const int32_t k = (int32_t)Kk[i];
    int64_t l = 0;
    for (int64_t q = pos[P[i]] + lane; q < pos[Rr[i]]; q += 64) l += (owner[row[q]] == k);
    for (int o = 32; o > 0; o >>= 1) l += __shfl_down(l, o);
    if (lane == 0) out_l[i] = l;
}

template <typename TC>
__global__ void k_cut_apply(int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ Rr, const int64_t *__restrict__ Kk,
                            int secondary, const int64_t *__restrict__ pos, const int64_t *__restrict__ tpos, const int64_t *__restrict__ pspl,
                            const int64_t *__restrict__ cl, DevModel<TC> M, TC *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int64_t p = P[i], r = Rr[i], k = Kk[i], l = cl[i];
    const TC alpha = dm_alpha(M, k);
    if (!secondary) out[i] = cut_apply(M.p, alpha, r - p, l, (pos[r] - pos[p]) - l);
    else {
        const int64_t s0 = pspl[k - 1] - 1, s1 = pspl[k] - 1;                    // rows of part k (0-based range)
        out[i] = cut_apply(M.p, alpha, s1 - s0, l, (tpos[s1] - tpos[s0]) - l);
    }
}

template <typename TC>
int32_t run_cut_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp,
                     const int64_t *k, TC *out)
{
    hipStream_t s = A->stream;
    if (nq <= 0) return CP_OK;
    const bool sec = mdl->kind == CP_MODEL_SECONDARY_EDGE_CUT;
    CP_REQUIRE(k, CP_EINVAL, "the plaid cost models take the part number k");
    CP_REQUIRE(!sec || (Pi && Pi->spl), CP_EINVAL, "the secondary edge-cut model needs a SplitPartition of the rows");
    if (sec) ensure_links(A);                                                    // tpos
    PlaidPart R;
    upload_part(A, Pi, sec, R);
    std::vector<int64_t> hp((size_t)nq), hr((size_t)nq);
    for (int64_t i = 0; i < nq; i++) {
        CP_REQUIRE(j[i] >= 1 && jp[i] >= j[i] && jp[i] <= A->n + 1 && k[i] >= 1 && k[i] <= R.K, CP_EINVAL, "oracle query out of range");
        hp[(size_t)i] = j[i] - 1; hr[(size_t)i] = jp[i] - 1;
    }
    DBuf<int64_t> dP((size_t)nq), dR((size_t)nq), dK((size_t)nq), cl((size_t)nq);
    DBuf<TC> dO((size_t)nq);
    CP_HIP(hipMemcpyAsync(dP.p, hp.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(dR.p, hr.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(dK.p, k, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    hipLaunchKernelGGL(k_cut_counts, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, nq, dP.p, dR.p, dK.p, A->pos.p, A->row.p, R.owner.p, cl.p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_apply<TC>), dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, nq, dP.p, dR.p, dK.p, sec ? 1 : 0,
                       A->pos.p, sec ? A->tpos.p : (const int64_t *)nullptr, sec ? R.spl.p : (const int64_t *)nullptr, cl.p, HM.d, dO.p);
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(out, dO.p, sizeof(TC) * (size_t)nq, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    return CP_OK;
}

// ------------------------------------------------------------------ bound_stripe
static int64_t cut_fld(int64_t a, int64_t b)
{
    int64_t q = a / b, r = a % b;
    if (r != 0 && ((r < 0) != (b < 0))) q -= 1;
    return q;
}
static double cut_fld(double a, int64_t b) { return std::floor(a / (double)b); }

template <typename TC>
int32_t cut_bound_stripe(cp_csr_s *A, int64_t K, const cp_rowpart_t *Pi, const cp_model_t *mdl, bool oracle_form, TC *lo, TC *hi)
{
    const TC a = model_param<TC>(mdl, CP_P_ALPHA), bv = model_param<TC>(mdl, CP_P_VERTEX), bs = model_param<TC>(mdl, CP_P_SELF_PIN),
             bc = model_param<TC>(mdl, CP_P_CUT_PIN);
    CP_REQUIRE(!(bv < 0 || bs < 0 || bc < 0) && bv == bv && bs == bs && bc == bc, CP_EINVAL, "bound_stripe asserts beta >= 0");
    const TC bmin = std::min(bs, bc), bmax = std::max(bs, bc);
    if (mdl->kind == CP_MODEL_PRIMARY_EDGE_CUT) {                                // PrimaryEdgeCutCosts.jl:28-39 (Pi dropped: Costs.jl:17-19)
        *hi = cadd(cadd(a, cmulc(A->n, bv)), cmulc(A->N, bmax));
        *lo = cadd(a, cut_fld(cadd(cmulc(A->n, bv), cmulc(A->N, bmin)), K));
        return CP_OK;
    }
    CP_REQUIRE(Pi && Pi->spl && Pi->K >= 1, CP_EINVAL, "the secondary edge-cut model needs a SplitPartition of the rows");
    const int64_t Kp = Pi->K, m = A->m;
    CP_REQUIRE(Pi->spl[0] == 1 && Pi->spl[Kp] == m + 1, CP_EINVAL, "split vector must run from 1 to m+1");
    for (int64_t k = 0; k < Kp; k++) CP_REQUIRE(Pi->spl[k] <= Pi->spl[k + 1], CP_EINVAL, "split vector out of range");
    CP_REQUIRE(!oracle_form || K <= Kp, CP_EINVAL, "the secondary model is evaluated for parts 1..K of Pi");
    CP_HIP(hipSetDevice(A->device));
    ensure_links(A);
    std::vector<int64_t> tpos((size_t)m + 1);                                    // pins of every part of Pi: the row pointer of A
    CP_HIP(hipMemcpyAsync(tpos.data(), A->tpos.p, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipStreamSynchronize(A->stream));
    auto work = [&](int64_t k, TC bp) {                                          // alpha + nv*b_vertex + np*b_pin of part k + 1
        const int64_t s0 = Pi->spl[k] - 1, s1 = Pi->spl[k + 1] - 1;
        return cadd(cadd(a, cmulc(s1 - s0, bv)), cmulc(tpos[(size_t)s1] - tpos[(size_t)s0], bp));
    };
    if (oracle_form) {                                                           // SecondaryEdgeCutCosts.jl:40-57: parts 1..K, min / max of the betas
        *lo = 0; *hi = 0;
        for (int64_t k = 0; k < K; k++) { *lo = std::max(*lo, work(k, bmin)); *hi = std::max(*hi, work(k, bmax)); }
    } else {                                                                     // :20-28: bottleneck_value(adj_A, Pi, AffineWorkModel(...)), all parts
        *lo = CostTraits<TC>::typemin(); *hi = CostTraits<TC>::typemin();
        for (int64_t k = 0; k < Kp; k++) { *lo = std::max(*lo, work(k, bs)); *hi = std::max(*hi, work(k, bc)); }
    }
    return CP_OK;
}

// ------------------------------------------------------------------ the K-part DP
__global__ void k_cut_flags(int64_t N, int32_t k, const int32_t *__restrict__ row, const int32_t *__restrict__ owner, int32_t *__restrict__ flag)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < N) flag[q] = owner[row[q]] == k ? 1 : 0;
}

// L_k[c] = the exclusive scan of the flags at pos[c], c = 0 .. n
__global__ void k_cut_gather(int64_t n, const int64_t *__restrict__ pos, const int32_t *__restrict__ Lq, int32_t *__restrict__ Lc)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= n) Lc[c] = Lq[pos[c]];
}

// layer 1: cst[j', 1] = f(1, j', 1)  (DynamicSplitter.jl:26-31)
template <typename TC>
__global__ void k_cut_layer1(int64_t n, CutLayer<TC> Y, const int64_t *__restrict__ pos, const int32_t *__restrict__ Lc, TC *__restrict__ cst,
                             int32_t *__restrict__ ptr)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    cst[r] = cut_f(Y, pos, Lc, 0, r);
    ptr[r] = 0;
}

// the literal candidate sweep: 64 rows per wave walk the candidates p downwards together (wave-uniform loads), so among equal
// values the largest p wins
template <typename TC>
__global__ void __launch_bounds__(256) k_cut_sweep(int64_t r_lo, int64_t r_hi, CutLayer<TC> Y, int32_t g, const int64_t *__restrict__ pos,
                                                   const int32_t *__restrict__ Lc, const TC *__restrict__ W, TC *__restrict__ cst,
                                                   int32_t *__restrict__ ptr)
{
    int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    int64_t r0 = r_lo + wave * 64;
    if (r0 > r_hi) return;
    int64_t r = r0 + lane;
    bool live = r <= r_hi;
    int64_t rtop = r0 + 63 < r_hi ? r0 + 63 : r_hi;
    if (!live) r = rtop;                                       // (idle lanes evaluate in bounds and store nothing)
    TC best = (TC)0;
    int64_t bp = -1;
    for (int64_t p = rtop; p >= 0; p--) {
        if (r >= p) {
            TC v = comb(g, W[p], cut_f(Y, pos, Lc, p, r));
            if (bp < 0 || v < best) { best = v; bp = p; }
        }
    }
    if (live) { cst[r] = best; ptr[r] = (int32_t)bp; }
}

// ---- the prefix-min scan with the rightmost argmin.  Elements are (value, index) pairs, index < 0: no element; of two elements
// the right one wins unless the left one is strictly smaller.  A block scans CUT_TILE elements: CUT_I per thread serially, a wave64
// shuffle scan of the thread aggregates, the wave aggregates through LDS.  Across blocks: the block aggregates are scanned by one
// block (k_cut_scan_aggs) and folded in by k_cut_scan_finish -- two levels, no block waits for another.
constexpr int CUT_T = 256, CUT_I = 4, CUT_TILE = CUT_T * CUT_I;

template <typename TC>
__device__ __forceinline__ void cut_fold(TC lv, int32_t li, TC &rv, int32_t &ri)      // (rv, ri) = left (+) right
{
    if (ri < 0 || (li >= 0 && lv < rv)) { rv = lv; ri = li; }
}

// inclusive scan of one pair per lane over the wave
template <typename TC>
__device__ __forceinline__ void cut_wave_scan(TC &v, int32_t &i, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        TC lv = __shfl_up(v, o);
        int32_t li = __shfl_up(i, o);
        if (lane >= o) cut_fold(lv, li, v, i);
    }
}

// inclusive scan of one pair per thread over a block of NW waves; also returns the block aggregate and (pv, pi), the aggregate of
// the waves before the thread's own.  sv / si: NW slots of LDS
template <typename TC, int NW>
__device__ __forceinline__ void cut_block_scan(TC &v, int32_t &i, TC &tot_v, int32_t &tot_i, TC &pv, int32_t &pi, TC *sv, int32_t *si)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    cut_wave_scan(v, i, lane);
    if (lane == 63) { sv[w] = v; si[w] = i; }
    __syncthreads();
    pv = (TC)0; pi = -1;                                      // the waves before this one, then all of them
    tot_v = (TC)0; tot_i = -1;
    for (int t = 0; t < NW; t++) {
        TC xv = sv[t]; int32_t xi = si[t];
        cut_fold(tot_v, tot_i, xv, xi);
        tot_v = xv; tot_i = xi;
        if (t + 1 == w) { pv = tot_v; pi = tot_i; }
    }
    cut_fold(pv, pi, v, i);
    __syncthreads();                                          // (sv / si may be written again)
}

// level 1: the tile's inclusive scan of v[p] = W[p] - S_k[p] into (tv, ti), its aggregate into (av, ai)[block]
template <typename TC>
__global__ void __launch_bounds__(CUT_T) k_cut_scan_tiles(int64_t n1, CutLayer<TC> Y, const int64_t *__restrict__ pos, const int32_t *__restrict__ Lc,
                                                          const TC *__restrict__ W, TC *__restrict__ tv, int32_t *__restrict__ ti,
                                                          TC *__restrict__ av, int32_t *__restrict__ ai)
{
    __shared__ TC sv[CUT_T / 64];
    __shared__ int32_t si[CUT_T / 64];
    const int64_t base = (int64_t)blockIdx.x * CUT_TILE + (int64_t)threadIdx.x * CUT_I;
    TC v[CUT_I]; int32_t ix[CUT_I];
    TC run = (TC)0; int32_t ri = -1;
#pragma unroll
    for (int t = 0; t < CUT_I; t++) {
        const int64_t c = base + t;
        if (c < n1) {
            TC x = csub(W[c], cut_S(Y, pos, Lc, c)); int32_t xi = (int32_t)c;
            cut_fold(run, ri, x, xi);
            run = x; ri = xi;
        }
        v[t] = run; ix[t] = ri;
    }
    TC tot_v, pv; int32_t tot_i, pi;
    cut_block_scan<TC, CUT_T / 64>(run, ri, tot_v, tot_i, pv, pi, sv, si);      // run / ri: now inclusive of this thread's items
    // the exclusive prefix of the thread: the inclusive value of the thread before it, or of the waves before for lane 0
    TC ev = __shfl_up(run, 1); int32_t ei = __shfl_up(ri, 1);
    if ((threadIdx.x & 63) == 0) { ev = pv; ei = pi; }
#pragma unroll
    for (int t = 0; t < CUT_I; t++) {
        const int64_t c = base + t;
        if (c < n1) { TC xv = v[t]; int32_t xi = ix[t]; cut_fold(ev, ei, xv, xi); tv[c] = xv; ti[c] = xi; }
    }
    if (threadIdx.x == CUT_T - 1) { av[blockIdx.x] = tot_v; ai[blockIdx.x] = tot_i; }
}

// level 2: inclusive scan of the nb block aggregates in place, one block, strips of 1024 with a carry
template <typename TC>
__global__ void __launch_bounds__(1024) k_cut_scan_aggs(int64_t nb, TC *__restrict__ av, int32_t *__restrict__ ai)
{
    __shared__ TC sv[16];
    __shared__ int32_t si[16];
    TC cv = (TC)0; int32_t ci = -1;                            // the strips before this one (the same in every thread)
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + threadIdx.x;
        TC v = (TC)0; int32_t x = -1;
        if (i < nb) { v = av[i]; x = ai[i]; }
        TC tot_v, pv; int32_t tot_i, pi;
        cut_block_scan<TC, 16>(v, x, tot_v, tot_i, pv, pi, sv, si);
        cut_fold(cv, ci, v, x);
        if (i < nb) { av[i] = v; ai[i] = x; }
        cut_fold(cv, ci, tot_v, tot_i);
        cv = tot_v; ci = tot_i;
    }
}

// level 3: cst[r] = const_k + S_k[r] + min, ptr[r] = argmin, the blocks before r's folded in
template <typename TC>
__global__ void __launch_bounds__(256) k_cut_scan_finish(int64_t n1, CutLayer<TC> Y, TC constk, const int64_t *__restrict__ pos,
                                                         const int32_t *__restrict__ Lc, const TC *__restrict__ tv, const int32_t *__restrict__ ti,
                                                         const TC *__restrict__ av, const int32_t *__restrict__ ai, TC *__restrict__ cst,
                                                         int32_t *__restrict__ ptr)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n1) return;
    const int64_t b = r / CUT_TILE;
    TC v = tv[r]; int32_t i = ti[r];
    if (b > 0) cut_fold(av[b - 1], ai[b - 1], v, i);
    cst[r] = cadd(cadd(constk, cut_S(Y, pos, Lc, r)), v);
    ptr[r] = i;
}

// one layer by the scan, three launches: cst[r] = constk + S_k[r] + min over p <= r of W[p] - S_k[p], ptr[r] the largest minimiser.
// Also the secondary connectivity cost's layer (plaid_total.hip), whose S_k has the secondary edge-cut form over another prefix count.
template <typename TC>
void cut_scan_layer(hipStream_t s, int64_t n1, const CutLayer<TC> &Y, TC constk, const int64_t *pos, const int32_t *Lc, const TC *W,
                    CutScanWork<TC> &ws, TC *cst, int32_t *ptr)
{
    const int64_t nb = cdiv(n1, (int64_t)CUT_TILE);
    ws.tv.ensure((size_t)n1); ws.ti.ensure((size_t)n1); ws.av.ensure((size_t)nb); ws.ai.ensure((size_t)nb);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_scan_tiles<TC>), dim3((unsigned)nb), dim3(CUT_T), 0, s, n1, Y, pos, Lc, W, ws.tv.p, ws.ti.p, ws.av.p, ws.ai.p);
    if (nb > 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_scan_aggs<TC>), dim3(1), dim3(1024), 0, s, nb, ws.av.p, ws.ai.p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_scan_finish<TC>), dim3((unsigned)cdiv(n1, 256)), dim3(256), 0, s, n1, Y, constk, pos, Lc, ws.tv.p, ws.ti.p,
                       ws.av.p, ws.ai.p, cst, ptr);
}
template void cut_scan_layer<int64_t>(hipStream_t, int64_t, const CutLayer<int64_t> &, int64_t, const int64_t *, const int32_t *, const int64_t *, CutScanWork<int64_t> &, int64_t *, int32_t *);
template void cut_scan_layer<double>(hipStream_t, int64_t, const CutLayer<double> &, double, const int64_t *, const int32_t *, const double *, CutScanWork<double> &, double *, int32_t *);

// The scan is the sweep only while no sum rounds or wraps.  model_exact_on bounds every total by B = K*max|alpha| + n*|b_vertex| +
// N*max(|b_self_pin|, |b_cut_pin|); the scan also forms S_k (at most 2B: the secondary one is a difference of two products) and
// W - S_k (at most 3B), so Float64 needs 4B < 2^53.  Int64: B < 2^60 keeps 3B below 2^63.
static bool cut_scan_exact(const cp_model_t *m, int64_t n, int64_t N, int64_t K)
{
    if (!model_exact_on(m, n, N, K)) return false;
    if (m->dtype == CP_I64) return true;
    double amax = std::fabs(m->p_f64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, std::fabs(((const double *)m->alpha_k)[i]));
    const double B = amax * (double)K + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)n +
                     std::max(std::fabs(m->p_f64[CP_P_SELF_PIN]), std::fabs(m->p_f64[CP_P_CUT_PIN])) * (double)N;
    return 4.0 * B < 9007199254740992.0;
}

template <typename TC> static TC cut_alpha(const cp_model_t *m, int64_t k)
{
    if (m->alpha_k && k >= 1 && k <= m->n_alpha_k) return ((const TC *)m->alpha_k)[k - 1];
    return model_param<TC>(m, CP_P_ALPHA);
}

template <typename TC>
int32_t run_cut_dynamic(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, const cp_rowpart_t *Pi,
                        int64_t *spl_out, int64_t *ptr_tab, TC *cst_tab)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, N = A->N;
    const bool sec = mdl->kind == CP_MODEL_SECONDARY_EDGE_CUT;
    CP_REQUIRE(order == CP_ORDER_SPLITTER, CP_EUNSUPPORTED, "the plaid cost models need the part number: splitter loop order only");
    const bool scan = combine == CP_COMBINE_SUM && !g_opt_force_brute && cut_scan_exact(mdl, n, N, K);
    CP_REQUIRE(scan || n <= g_opt_brute_max_n, CP_EUNSUPPORTED, "plaid cost models run the O(n^2) device sweep: n too large");
    CP_REQUIRE(!sec || (Pi && Pi->spl), CP_EINVAL, "the secondary edge-cut model needs a SplitPartition of the rows");
    if (sec) ensure_links(A);                                        // tpos
    PlaidPart R;
    upload_part(A, Pi, sec, R);
    CP_REQUIRE(K <= R.K, CP_EINVAL, "the plaid edge-cut models are evaluated for parts 1..K of Pi");
    const size_t n1 = (size_t)n + 1;
    DBuf<TC> cstA(n1), cstB(n1);
    DBuf<int32_t> ptr((size_t)K * n1), flag((size_t)(N > 0 ? N : 1)), Lq((size_t)N + 1), Lc(n1);
    CutScanWork<TC> ws;
    DBuf<int64_t> scratch;
    std::vector<int64_t> htpos;
    if (sec) {                                                       // pins of every part of Pi: tpos = row pointer of A
        htpos.resize((size_t)A->m + 1);
        CP_HIP(hipMemcpyAsync(htpos.data(), A->tpos.p, sizeof(int64_t) * (size_t)(A->m + 1), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
    }
    std::vector<TC> hc;
    std::vector<int32_t> hp;
    TC *prevc = cstA.p, *curc = cstB.p;
    for (int64_t k = 1; k <= K; k++) {
        CutLayer<TC> Y;
        memset(&Y, 0, sizeof(Y));
        Y.secondary = sec ? 1 : 0;
        Y.alpha = cut_alpha<TC>(mdl, k);
        for (int i = 0; i < 5; i++) Y.p[i] = model_param<TC>(mdl, i);
        if (sec) {
            const int64_t s0 = R.hspl[(size_t)k - 1] - 1, s1 = R.hspl[(size_t)k] - 1;
            Y.nvk = s1 - s0; Y.wk = htpos[(size_t)s1] - htpos[(size_t)s0];
        }
        // L_k: flag the entries part k owns, scan the flags, read the scan at the column starts (a heavy column costs nothing extra)
        if (N > 0) hipLaunchKernelGGL(k_cut_flags, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, N, (int32_t)k, A->row.p, R.owner.p, flag.p);
        exclusive_scan_i32_i32(flag.p, Lq.p, N, scratch, s);
        hipLaunchKernelGGL(k_cut_gather, dim3((unsigned)cdiv((int64_t)n1, 256)), dim3(256), 0, s, n, A->pos.p, Lq.p, Lc.p);
        int32_t *pk = ptr.p + (size_t)(k - 1) * n1;
        const int64_t rlo = (k == K && K > 1) ? n : 0;               // layer K: row n+1 only (DynamicSplitter.jl:34); the scan computes the
                                                                     // whole layer in its one pass, and only that row is kept
        if (k == 1) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_layer1<TC>), dim3((unsigned)cdiv((int64_t)n1, 256)), dim3(256), 0, s, n, Y, A->pos.p, Lc.p, curc, pk);
        } else if (scan) {
            const TC constk = sec ? cadd(cadd(Y.alpha, cmulc(Y.nvk, Y.p[CP_P_VERTEX])), cmulc(Y.wk, Y.p[CP_P_CUT_PIN])) : Y.alpha;
            ProfScope ps(PROF_SCAN, s, 0.0);
            cut_scan_layer<TC>(s, (int64_t)n1, Y, constk, A->pos.p, Lc.p, prevc, ws, curc, pk);
            g_cut_scan_layers++;
        } else {
            const int64_t waves = cdiv(n - rlo + 1, (int64_t)64);
            ProfScope ps(PROF_BRUTE, s, 0.0);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cut_sweep<TC>), dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, rlo, n, Y, combine, A->pos.p, Lc.p,
                               prevc, curc, pk);
        }
        CP_HIP(hipGetLastError());
        if (ptr_tab) {                                               // rows outside [rlo, n]: zeros(Ti) / fill(typemax), as run_dynamic's tables
            hc.resize(n1); hp.resize(n1);
            CP_HIP(hipMemcpyAsync(hc.data(), curc, sizeof(TC) * n1, hipMemcpyDeviceToHost, s));
            CP_HIP(hipMemcpyAsync(hp.data(), pk, sizeof(int32_t) * n1, hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            for (int64_t r = 0; r <= n; r++) {
                ptr_tab[(size_t)(k - 1) * n1 + (size_t)r] = r >= rlo ? (int64_t)hp[(size_t)r] + 1 : 0;
                cst_tab[(size_t)(k - 1) * n1 + (size_t)r] = r >= rlo ? hc[(size_t)r] : CostTraits<TC>::typemax();
            }
        }
        std::swap(prevc, curc);
    }
    std::vector<int64_t> spl((size_t)K + 1);
    spl[(size_t)K] = n;
    for (int64_t k = K; k >= 1; k--) {                               // unravel_splits (DynamicSplitter.jl:89-99)
        int32_t v = 0;
        CP_HIP(hipMemcpyAsync(&v, ptr.p + (size_t)(k - 1) * n1 + (size_t)spl[(size_t)k], sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        spl[(size_t)k - 1] = v;
    }
    for (int64_t k = 0; k <= K; k++) spl_out[k] = spl[(size_t)k] + 1;
    prof_collect();
    return CP_OK;
}

template int32_t run_cut_eval<int64_t>(cp_csr_s *, const cp_model_t *, const cp_rowpart_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t *);
template int32_t run_cut_eval<double>(cp_csr_s *, const cp_model_t *, const cp_rowpart_t *, int64_t, const int64_t *, const int64_t *, const int64_t *, double *);
template int32_t cut_bound_stripe<int64_t>(cp_csr_s *, int64_t, const cp_rowpart_t *, const cp_model_t *, bool, int64_t *, int64_t *);
template int32_t cut_bound_stripe<double>(cp_csr_s *, int64_t, const cp_rowpart_t *, const cp_model_t *, bool, double *, double *);
template int32_t run_cut_dynamic<int64_t>(cp_csr_s *, int64_t, int32_t, int32_t, const cp_model_t *, const cp_rowpart_t *, int64_t *, int64_t *, int64_t *);
template int32_t run_cut_dynamic<double>(cp_csr_s *, int64_t, int32_t, int32_t, const cp_model_t *, const cp_rowpart_t *, int64_t *, int64_t *, double *);

}  // namespace cpk
