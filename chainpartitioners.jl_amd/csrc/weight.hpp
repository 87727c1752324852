// weight.hpp -- the weights of ConstrainedCost(f, w, w_max) that bound a part from the left: j0(j'), the first column whose part up
// to j' fits, is non-decreasing in j' (dp_driver.hip: windowed splitters; chunk_lws.hip: the scalable DynamicTotalChunker).
#pragma once
#include "model.hpp"

namespace cpk {

// Any monotone weight w(j, j') = alpha + b_v (j' - j) + b_p (pos[j'] - pos[j]) with b_v, b_p >= 0 (AffineWorkModel: pins per part,
// work per part): the part [j, j') fits iff j >= j0(j'), the first column whose part up to j' fits -- non-decreasing in j'.  The
// reference finds it by advancing j0 while w(j0, j', k) > w_max (DynamicSplitter.jl:235-237); with a monotone weight that is this
// array, found by bisection in the weight's own arithmetic (WorkCosts.jl:17).  j0[r] (0-based row r = j' - 1, 0-based column),
// r + 1 when not even the empty part fits.
template <typename TW>
__global__ void __launch_bounds__(256) k_weight_j0(int64_t n, const int64_t *__restrict__ pos, TW alpha, TW bv, TW bp, TW wmax, int32_t *__restrict__ j0)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const int64_t pr = pos[r];
    auto fits = [&](int64_t p) { return cadd(cadd(alpha, cmulc(r - p, bv)), cmulc(pr - pos[p], bp)) <= wmax; };
    int64_t lo = 0, hi = r + 1;                            // first p in [0, r] that fits; r + 1: none
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (fits(mid)) hi = mid; else lo = mid + 1; }
    j0[r] = (int32_t)lo;
}

// A weight that is a function of the WIDTH only -- VertexCount(), or AffineWorkModel(alpha, c, 0) with c > 0 (the reference's own
// tests constrain with AffineWorkModel(0, 1, 0), test/test_Partitioners.jl:178-183,256-261) -- bounds the parts by a number of
// columns: the largest nv with w(nv) = alpha + nv c <= w_max, evaluated in the weight's own arithmetic and order (WorkCosts.jl:17;
// the pin term is nv * 0 = 0).  -> that width (0: only empty parts fit, -1: not even those), or -2: not a width weight.
inline int64_t width_of_weight(const cp_model_t *w, int64_t n, int64_t wmax_i64, double wmax_f64)
{
    if (!w) return -2;
    if (w->kind == CP_MODEL_VERTEX_COUNT) return wmax_i64;
    if (w->kind != CP_MODEL_WORK || w->alpha_k) return -2;
    auto fits_i = [&](int64_t nv) { return cadd(cadd(w->p_i64[CP_P_ALPHA], cmulc(nv, w->p_i64[CP_P_VERTEX])), cmulc((int64_t)0, w->p_i64[CP_P_PIN])) <= wmax_i64; };
    auto fits_f = [&](int64_t nv) { return cadd(cadd(w->p_f64[CP_P_ALPHA], cmulc(nv, w->p_f64[CP_P_VERTEX])), cmulc((int64_t)0, w->p_f64[CP_P_PIN])) <= wmax_f64; };
    const bool is_i = w->dtype == CP_I64;
    if (is_i ? !(w->p_i64[CP_P_PIN] == 0 && w->p_i64[CP_P_VERTEX] > 0) : !(w->p_f64[CP_P_PIN] == 0.0 && w->p_f64[CP_P_VERTEX] > 0.0)) return -2;
    auto fits = [&](int64_t nv) { return is_i ? fits_i(nv) : fits_f(nv); };
    if (!fits(0)) return -1;
    int64_t lo = 0, hi = n + 1;                       // fits(lo); the weight grows with nv: the largest nv <= n + 1 that fits
    if (fits(hi)) return hi;
    while (hi - lo > 1) { const int64_t mid = lo + ((hi - lo) >> 1); if (fits(mid)) lo = mid; else hi = mid; }
    return lo;
}

// AffineWorkModel(alpha, b_v, b_p) with b_v, b_p >= 0: grows with its part (k_weight_j0)
inline bool monotone_work_weight(const cp_model_t *w)
{
    if (!w || w->kind != CP_MODEL_WORK || w->alpha_k) return false;
    return w->dtype == CP_I64 ? (w->p_i64[CP_P_VERTEX] >= 0 && w->p_i64[CP_P_PIN] >= 0) : (w->p_f64[CP_P_VERTEX] >= 0 && w->p_f64[CP_P_PIN] >= 0);
}

// ... and, for an Int64 weight, one whose values cannot wrap on an n-column, N-nonzero pattern: |alpha| + (n + 1) |b_v| + (N + 1) |b_p|
// + |w_max| below 2^62 (a wrapped weight does not grow with its part).  Float64 weights: always.
inline bool work_weight_no_wrap(const cp_model_t *w, int64_t n, int64_t N, int64_t wmax_i64)
{
    if (w->dtype != CP_I64) return true;
    const u128 b = mag128(w->p_i64[CP_P_ALPHA]) + mag128(w->p_i64[CP_P_VERTEX]) * (u128)(n + 1) + mag128(w->p_i64[CP_P_PIN]) * (u128)(N + 1) + mag128(wmax_i64);
    return b < ((u128)1 << 62);
}

}  // namespace cpk
