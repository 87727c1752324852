// model.hpp -- device-side evaluation of the cost models, bit-for-bit in the reference's
// evaluation order (left to right, one Int->Float conversion per product, no FMA contraction;
// the translation unit is compiled with -ffp-contract=off):
//   AffineWorkModel           alpha + nv*b_vertex + np*b_pin                       WorkCosts.jl:17
//   AffineConnectivityModel   ... + nn*b_net                                       ConnectivityCosts.jl:20
//   AffineHyperedgeCutModel   ... + nl*b_self_net + (nn-nl)*b_cut_net              HyperedgeCutCosts.jl:21
//   ColumnBlockComponentCostModel  alpha_col(w) + nn*beta_col(w)                   BlockCosts.jl:17
#pragma once
#include "common.hpp"
#include <cmath>
#include <algorithm>

namespace cpk {

template <typename TC> struct CostTraits;
template <> struct CostTraits<int64_t> {
    static constexpr bool is_int = true;
    __host__ __device__ static int64_t typemax() { return INT64_MAX; }
    __host__ __device__ static int64_t typemin() { return INT64_MIN; }
};
template <> struct CostTraits<double> {
    static constexpr bool is_int = false;
    __host__ __device__ static double typemax() { return __builtin_huge_val(); }
    __host__ __device__ static double typemin() { return -__builtin_huge_val(); }
};

// Julia Int64 arithmetic wraps; do integer adds/muls through uint64
__host__ __device__ __forceinline__ int64_t cadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__host__ __device__ __forceinline__ double cadd(double a, double b) { return a + b; }
__host__ __device__ __forceinline__ int64_t csub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
__host__ __device__ __forceinline__ double csub(double a, double b) { return a - b; }
__host__ __device__ __forceinline__ int64_t cmulc(int64_t cnt, int64_t b) { return (int64_t)((uint64_t)cnt * (uint64_t)b); }
__host__ __device__ __forceinline__ double cmulc(int64_t cnt, double b) { return (double)cnt * b; }
__host__ __device__ __forceinline__ int64_t cmulv(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__host__ __device__ __forceinline__ double cmulv(double a, double b) { return a * b; }

template <typename TC>
struct DevModel {
    int32_t kind;
    TC p[5];
    const TC *alpha_k;      // device copy or nullptr
    int64_t n_alpha_k;
    // block-column components (COLBLOCK / BLOCK): constants or device tables
    int32_t ac_const, bc_const[CP_MAX_R];
    TC ac_c, bc_c[CP_MAX_R];
    const TC *ac_tab, *bc_tab[CP_MAX_R];
    int64_t ac_len, bc_len[CP_MAX_R];
    int64_t ac_lo, bc_lo[CP_MAX_R];       // width of table entry 0
    int32_t R;
};

template <typename TC>
__host__ __device__ __forceinline__ TC dm_alpha(const DevModel<TC> &m, int64_t k)
{
    if (m.alpha_k && k >= 1 && k <= m.n_alpha_k) return m.alpha_k[k - 1];
    return m.p[CP_P_ALPHA];
}

template <typename TC>
__device__ __forceinline__ TC dm_comp(int32_t is_const, TC c, const TC *tab, int64_t len, int64_t lo, int64_t w)
{
    if (is_const) return c;
    w -= lo;
    if (w < 0) w = 0;
    if (w >= len) w = len - 1;     // the host mirror sizes the tables for every width a method can evaluate
    return tab[w];
}

// alpha + (nv*b_vertex + np*b_pin)^gamma  (test_Partitioners.jl:60,70); Float64 models only
__device__ __forceinline__ double pw_apply(double alpha, const double *p, int64_t nv, int64_t np)
{
    double x = (double)nv * p[CP_P_VERTEX] + (double)np * p[CP_P_PIN];
    double g = p[CP_P_GAMMA];
    return alpha + (g == 2.0 ? x * x : pow(x, g));
}
__device__ __forceinline__ int64_t pw_apply(int64_t, const int64_t *, int64_t, int64_t) { return 0; }

// model applied to counts; alpha is resolved by the caller (per-part alpha[k] or scalar)
template <typename TC>
__device__ __forceinline__ TC dm_apply(const DevModel<TC> &m, TC alpha, int64_t nv, int64_t np, int64_t nn, int64_t nl)
{
    switch (m.kind) {
    case CP_MODEL_WORK:
        return cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN]));
    case CP_MODEL_CONNECTIVITY:
        return cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])), cmulc(nn, m.p[CP_P_NET]));
    case CP_MODEL_HYPEREDGE_CUT:
        return cadd(cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])),
                         cmulc(nl, m.p[CP_P_SELF_NET])), cmulc(nn - nl, m.p[CP_P_CUT_NET]));
    case CP_MODEL_COLBLOCK:
        return cadd(dm_comp(m.ac_const, m.ac_c, m.ac_tab, m.ac_len, m.ac_lo, nv),
                    cmulc(nn, dm_comp(m.bc_const[0], m.bc_c[0], m.bc_tab[0], m.bc_len[0], m.bc_lo[0], nv)));
    case CP_MODEL_VERTEX_COUNT:
        return (TC)nv;
    case CP_MODEL_POWER_WORK:
        return pw_apply(alpha, m.p, nv, np);
    case CP_MODEL_PRIMARY: case CP_MODEL_SECONDARY:     // nn = local nets, nl = remote nets (PrimaryConnectivityCosts.jl:20)
        return cadd(cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])), cmulc(nn, m.p[CP_P_LOCAL_NET])),
                    cmulc(nl, m.p[CP_P_REMOTE_NET]));
    default:
        return (TC)0;
    }
}

template <typename TC>
__device__ __forceinline__ TC comb(int32_t g, TC a, TC b)
{
    if (g == CP_COMBINE_SUM) return cadd(a, b);
    return a > b ? a : b;
}

// The model families with counters of their own (sym.hpp, envelope.hpp)
inline bool model_is_sym(int32_t kind) { return kind >= CP_MODEL_SYM_CONNECTIVITY && kind <= CP_MODEL_SYM_EDGE_CUT; }
inline bool model_is_env(int32_t kind) { return kind == CP_MODEL_ENVELOPE; }

// The kinds the K-layer stripe DP driver (dp_driver.hip) takes, as nested sets: each caller names the largest it serves.
enum DpKinds {
    DP_KINDS_AFFINE,       // Work / Connectivity / HyperedgeCut: the only kinds of the scalable constrained paths
    DP_KINDS_TILED,        // + ColumnBlockComponent: the row-tiled entry
    DP_KINDS_STRIPE,       // + PowerWork and the symmetric family: the one-shot partition entry
    DP_KINDS_TABLES,       // + the envelope model: the tables entry
};
inline bool dp_takes_kind(int32_t kind, DpKinds set)
{
    if (kind == CP_MODEL_WORK || kind == CP_MODEL_CONNECTIVITY || kind == CP_MODEL_HYPEREDGE_CUT) return true;
    if (kind == CP_MODEL_COLBLOCK) return set >= DP_KINDS_TILED;
    if (kind == CP_MODEL_POWER_WORK || model_is_sym(kind)) return set >= DP_KINDS_STRIPE;
    return model_is_env(kind) && set >= DP_KINDS_TABLES;
}

// |v| in 128 bits (|INT64_MIN| included): the Int64 exactness gates sum parameter magnitudes times counts without wrapping
typedef unsigned __int128 u128;
inline u128 mag128(int64_t v) { return v < 0 ? (u128)0 - (u128)(__int128)v : (u128)v; }

// Int64 model, or a Float64 model whose scalar parameters are all integer-valued (then every cost is an exactly
// represented integer).  Neither makes sums exact by itself: Float64 rounds above 2^53 and Int64 wraps (cadd / cmulc, as
// Julia does) -- model_exact_on adds the bound.
inline bool model_all_integral(const cp_model_t *m)
{
    if (m->dtype == CP_I64) return true;
    if (m->kind == CP_MODEL_POWER_WORK) return false;
    for (int i = 0; i < 5; i++) if (std::floor(m->p_f64[i]) != m->p_f64[i] || std::fabs(m->p_f64[i]) > 9e15) return false;
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) { double v = ((const double *)m->alpha_k)[i]; if (std::floor(v) != v) return false; }
    return true;
}

// ... and bounded so: the exact-arithmetic paths (O(n log^2 n) DP, windowed DP, valley search, (min,+) chunk scan) reassociate
// sums, rely on inverse-Monge / monotone costs and argue about ties, which is the reference's sequential arithmetic only while
// every cost and every running total is the true integer.  Largest reachable |total| of a K-part partition of an n-column,
// N-nonzero pattern: K*|alpha| + n*|b_vertex| + N*|b_pin| + N*max|b_net-like| (column blocks: K*max|alpha_col| + N*max|beta_col|).
// Float64: below 2^53.  Int64: a wrapped total is none of the three (a wrapped cost is neither inverse-Monge nor monotone), so
// the bound is computed exactly in 128 bits and kept below 2^60 -- which also keeps every real total under the 2^61 that marks
// "outside the window" (BigCost, CsInf) and sentinel + cost from wrapping.  Other Int64 kinds: no bound, not exact.
inline bool model_exact_on(const cp_model_t *m, int64_t n, int64_t N, int64_t K)
{
    if (!model_all_integral(m)) return false;
    if (m->dtype == CP_I64) {
        auto comp_max = [&](const cp_component_t &c) {
            u128 r = mag128(c.c_i64);
            if (!c.is_const) { r = 0; if (c.table) for (int64_t i = 0; i < c.len; i++) r = std::max(r, mag128(((const int64_t *)c.table)[i])); }
            return r;
        };
        u128 amax, bv = 0, bp = 0, bnet;
        int64_t Nnet = N;                      // how many entries the net-like count can reach
        if (m->kind == CP_MODEL_MONO_SYM_CONNECTIVITY) {
            // the Connectivity bound on the pattern with its diagonal added: the dianet count reaches N + n; p[4] is Delta_pins, no cost
            amax = mag128(m->p_i64[CP_P_ALPHA]);
            if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
            bv = mag128(m->p_i64[CP_P_VERTEX]); bp = mag128(m->p_i64[CP_P_OVER_PIN]); bnet = mag128(m->p_i64[CP_P_DIA_NET]);
            Nnet = N + n;
        } else if (m->kind == CP_MODEL_COLBLOCK) {
            amax = comp_max(m->alpha_col);
            bnet = comp_max(m->beta_col[0]);
        } else if (dp_takes_kind(m->kind, DP_KINDS_AFFINE)) {
            amax = mag128(m->p_i64[CP_P_ALPHA]);
            if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
            bv = mag128(m->p_i64[CP_P_VERTEX]); bp = mag128(m->p_i64[CP_P_PIN]);
            bnet = std::max(mag128(m->p_i64[3]), mag128(m->p_i64[4]));
        } else if (m->kind == CP_MODEL_PRIMARY_EDGE_CUT || m->kind == CP_MODEL_SECONDARY_EDGE_CUT) {
            // every pin is a self pin or a cut pin: K*max|alpha| + n*|b_vertex| + N*max(|b_self_pin|, |b_cut_pin|)
            amax = mag128(m->p_i64[CP_P_ALPHA]);
            if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
            bv = mag128(m->p_i64[CP_P_VERTEX]);
            bnet = std::max(mag128(m->p_i64[CP_P_SELF_PIN]), mag128(m->p_i64[CP_P_CUT_PIN]));
        } else {
            return false;
        }
        const u128 bound = amax * (u128)(K > 0 ? K : 1) + bv * (u128)(n > 0 ? n : 0) + bp * (u128)(N > 0 ? N : 0) + bnet * (u128)(Nnet > 0 ? Nnet : 0);
        return bound < ((u128)1 << 60);
    }
    double amax = std::fabs(m->p_f64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, std::fabs(((const double *)m->alpha_k)[i]));
    // (the edge-cut pair: this bounds the totals only; the prefix-min scan also forms W - S_k and asks for more -- cut_scan_exact, plaid_cut.hip)
    if (m->kind == CP_MODEL_PRIMARY_EDGE_CUT || m->kind == CP_MODEL_SECONDARY_EDGE_CUT)
        return amax * (double)(K > 0 ? K : 1) + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)n +
               std::max(std::fabs(m->p_f64[CP_P_SELF_PIN]), std::fabs(m->p_f64[CP_P_CUT_PIN])) * (double)N < 9007199254740992.0;
    const bool mono = m->kind == CP_MODEL_MONO_SYM_CONNECTIVITY;
    double bnet = mono ? std::fabs(m->p_f64[CP_P_DIA_NET]) : std::max(std::fabs(m->p_f64[3]), std::fabs(m->p_f64[4]));
    double bound = amax * (double)(K > 0 ? K : 1) + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)n + std::fabs(m->p_f64[CP_P_PIN]) * (double)N + bnet * (double)(mono ? N + n : N);
    return bound < 9007199254740992.0;       // 2^53
}

// is the O(n log^2 n) total-cost scheme exact for this model?  Needs W[p]+f(p,r) inverse-Monge:
// modular terms (alpha, vertices, pins) are free; the net count is submodular, so beta_net >= 0;
// hyperedge cost = d*b_cut + l*(b_self - b_cut) needs b_cut >= 0 and b_self <= b_cut.
// Both element types qualify only while every reachable total is exact (model_exact_on): a Float64 model needs integer-valued
// parameters and totals below 2^53, an Int64 model totals below 2^60 -- a wrapped Int64 total is not inverse-Monge.
inline bool fast_total_ok(const cp_model_t *m, int64_t n, int64_t N, int64_t K)
{
    if (!model_exact_on(m, n, N, K)) return false;
    auto P = [&](int i) { return m->dtype == CP_I64 ? (double)m->p_i64[i] : m->p_f64[i]; };
    if (m->kind == CP_MODEL_WORK) return true;
    if (m->kind == CP_MODEL_CONNECTIVITY) return P(CP_P_NET) >= 0;
    if (m->kind == CP_MODEL_HYPEREDGE_CUT) return P(CP_P_CUT_NET) >= 0 && P(CP_P_SELF_NET) <= P(CP_P_CUT_NET);
    return false;
}

// The same question for the symmetric family (sym.hpp), a predicate of its own: is the divide and conquer of sym_total.hip exact?
// All three costs are modular terms plus multiples of counts that are submodular in the column range -- the net count of A, the net
// count dianet of the derived pattern D -- or supermodular -- selfpin, the entries with both ends inside the range:
//   kind 11   modular + dianet*b_dia_net                                          b_dia_net >= 0
//   kind 10   modular + net*b_local_net + (dianet - nv)*(b_remote_net - b_local_net)      b_local_net >= 0, b_remote_net >= b_local_net
//   kind 12   modular + selfpin*(b_self_pin - b_cut_pin)                           b_self_pin <= b_cut_pin
// alpha, alpha[k], b_vertex and b_pin / b_over_pin are free.  Every reachable total must be exact, as for fast_total_ok: integer-valued
// parameters, and K*max|alpha| + n*|b_vertex| + ... below 2^60 (Int64, in 128 bits) or 2^53 (Float64), where the counts reach
//   kind 11   what model_exact_on bounds
//   kind 10   N pins, and N + n for each of the two net terms (local + remote = net <= N, remote <= dianet <= N + n)
//   kind 12   N pins in all, each a self pin or a cut pin
// n < 2^30 and the 32-bit layout of D's keys (ensure_sym_links) hold besides.
inline bool sym_total_ok(const cp_model_t *m, int64_t n, int64_t N, int64_t K)
{
    if (!model_is_sym(m->kind) || !model_all_integral(m)) return false;
    if (n < 0 || N < 0 || n >= ((int64_t)1 << 30) || N + n >= ((int64_t)1 << 31) - 1) return false;
    auto P = [&](int i) { return m->dtype == CP_I64 ? (double)m->p_i64[i] : m->p_f64[i]; };
    if (m->kind == CP_MODEL_MONO_SYM_CONNECTIVITY) return P(CP_P_DIA_NET) >= 0 && model_exact_on(m, n, N, K);
    const bool conn = m->kind == CP_MODEL_SYM_CONNECTIVITY;
    if (conn ? !(P(CP_P_LOCAL_NET) >= 0 && P(CP_P_REMOTE_NET) >= P(CP_P_LOCAL_NET)) : !(P(CP_P_SELF_PIN) <= P(CP_P_CUT_PIN))) return false;
    const int64_t Kk = K > 0 ? K : 1;
    if (m->dtype == CP_I64) {
        u128 amax = mag128(m->p_i64[CP_P_ALPHA]);
        if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
        u128 bound = amax * (u128)Kk + mag128(m->p_i64[CP_P_VERTEX]) * (u128)n;
        if (conn) bound += mag128(m->p_i64[CP_P_PIN]) * (u128)N + (mag128(m->p_i64[CP_P_LOCAL_NET]) + mag128(m->p_i64[CP_P_REMOTE_NET])) * (u128)(N + n);
        else bound += std::max(mag128(m->p_i64[CP_P_SELF_PIN]), mag128(m->p_i64[CP_P_CUT_PIN])) * (u128)N;
        return bound < ((u128)1 << 60);
    }
    double amax = std::fabs(m->p_f64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, std::fabs(((const double *)m->alpha_k)[i]));
    double bound = amax * (double)Kk + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)n;
    if (conn) bound += std::fabs(m->p_f64[CP_P_PIN]) * (double)N + (std::fabs(m->p_f64[CP_P_LOCAL_NET]) + std::fabs(m->p_f64[CP_P_REMOTE_NET])) * (double)(N + n);
    else bound += std::max(std::fabs(m->p_f64[CP_P_SELF_PIN]), std::fabs(m->p_f64[CP_P_CUT_PIN])) * (double)N;
    return bound < 9007199254740992.0;       // 2^53
}

// ... and for the plaid connectivity pair (plaid.hip), kinds 8 / 9 under a row partition Pi: the exact total-cost paths of
// plaid_total.hip.  max|alpha| over the scalar and the per-part values, in 128 bits / as a double:
inline u128 model_amax128(const cp_model_t *m)
{
    u128 amax = mag128(m->p_i64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
    return amax;
}
inline double model_amax_f64(const cp_model_t *m)
{
    double amax = std::fabs(m->p_f64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, std::fabs(((const double *)m->alpha_k)[i]));
    return amax;
}
// Primary, layer k: f(p, r, k) = alpha_k + (r - p)*b_vertex + pins*b_pin + b_local_net*nets_k(p, r) + b_remote_net*nets_notk(p, r), nets_k
// the net count of the rows Pi gives to part k and nets_notk = nets - nets_k that of all other rows.  Both are net counts of row
// sub-matrices, hence submodular in the column range: with b_local_net >= 0 and b_remote_net >= 0 the cost is modular plus
// non-negative multiples of submodular counts, which is the inverse-Monge property lws_rect.hpp asks for (bound_stripe asserts the
// same two signs).  alpha, alpha[k], b_vertex and b_pin are free.  The objective is a sum and the loop order is the splitter's (the
// cost needs k).  Every reachable total is exact: integer-valued parameters and K*max|alpha| + n*|b_vertex| + N*|b_pin| +
// N*max(b_local_net, b_remote_net) -- the nets of disjoint column ranges sum to at most N -- below 2^60 (Int64, in 128 bits) or 2^53
// (Float64).  n < 2^30.
inline bool plaid_total_ok(const cp_model_t *m, int64_t n, int64_t N, int64_t K, int32_t combine, int32_t order)
{
    if (m->kind != CP_MODEL_PRIMARY || combine != CP_COMBINE_SUM || order != CP_ORDER_SPLITTER || !model_all_integral(m)) return false;
    if (n < 0 || N < 0 || n >= ((int64_t)1 << 30)) return false;
    const int64_t Kk = K > 0 ? K : 1;
    if (m->dtype == CP_I64) {
        if (m->p_i64[CP_P_LOCAL_NET] < 0 || m->p_i64[CP_P_REMOTE_NET] < 0) return false;
        const u128 bound = model_amax128(m) * (u128)Kk + mag128(m->p_i64[CP_P_VERTEX]) * (u128)n + mag128(m->p_i64[CP_P_PIN]) * (u128)N +
                           std::max(mag128(m->p_i64[CP_P_LOCAL_NET]), mag128(m->p_i64[CP_P_REMOTE_NET])) * (u128)N;
        return bound < ((u128)1 << 60);
    }
    if (!(m->p_f64[CP_P_LOCAL_NET] >= 0) || !(m->p_f64[CP_P_REMOTE_NET] >= 0)) return false;
    const double bound = model_amax_f64(m) * (double)Kk + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)n + std::fabs(m->p_f64[CP_P_PIN]) * (double)N +
                         std::max(m->p_f64[CP_P_LOCAL_NET], m->p_f64[CP_P_REMOTE_NET]) * (double)N;
    return bound < 9007199254740992.0;       // 2^53
}
// Secondary, layer k: f(i, i', k) = const_k + (P_k[i'] - P_k[i])*(b_local_net - b_remote_net), P_k[c] the columns < c that hold a row of
// part k, const_k = alpha_k + nv_k*b_vertex + w_k*b_pin + d_k*b_remote_net: the prefix-difference form of the edge-cut pair, so a layer
// is one prefix-min scan for any sign of the two betas.  The scan reassociates the sums and is the sweep only while every value is the
// true integer: B = K*max|alpha| + m*|b_vertex| + N*|b_pin| + N*max(|b_local_net|, |b_remote_net|) bounds the totals (m: the rows Pi
// splits); the scan also forms S_k (at most 2B) and W - S_k (at most 3B), so an integral Float64 model needs 4B < 2^53 and Int64 B < 2^60,
// as cut_scan_exact (plaid_cut.hip).
inline bool plaid_scan_exact(const cp_model_t *m, int64_t mrows, int64_t N, int64_t K, int32_t combine, int32_t order)
{
    if (m->kind != CP_MODEL_SECONDARY || combine != CP_COMBINE_SUM || order != CP_ORDER_SPLITTER || !model_all_integral(m)) return false;
    if (mrows < 0 || N < 0) return false;
    const int64_t Kk = K > 0 ? K : 1;
    if (m->dtype == CP_I64) {
        const u128 bound = model_amax128(m) * (u128)Kk + mag128(m->p_i64[CP_P_VERTEX]) * (u128)mrows + mag128(m->p_i64[CP_P_PIN]) * (u128)N +
                           std::max(mag128(m->p_i64[CP_P_LOCAL_NET]), mag128(m->p_i64[CP_P_REMOTE_NET])) * (u128)N;
        return bound < ((u128)1 << 60);
    }
    const double B = model_amax_f64(m) * (double)Kk + std::fabs(m->p_f64[CP_P_VERTEX]) * (double)mrows + std::fabs(m->p_f64[CP_P_PIN]) * (double)N +
                     std::max(std::fabs(m->p_f64[CP_P_LOCAL_NET]), std::fabs(m->p_f64[CP_P_REMOTE_NET])) * (double)N;
    return 4.0 * B < 9007199254740992.0;
}

// host: build a DevModel from the C-ABI struct, uploading alpha_k / tables
template <typename TC>
struct HostModel {
    DevModel<TC> d;
    DBuf<TC> alpha_k;
    DBuf<TC> tabs[2 + 2 * CP_MAX_R];
};

template <typename TC> inline TC model_param(const cp_model_t *m, int i);
template <> inline int64_t model_param<int64_t>(const cp_model_t *m, int i) { return m->p_i64[i]; }
template <> inline double model_param<double>(const cp_model_t *m, int i) { return m->p_f64[i]; }
// The one place the C ABI's dtype becomes a C++ cost type:  with_cost_type(m->dtype, [&](auto tag) { using TC = decltype(tag); ... })
template <typename F> inline auto with_cost_type(int32_t dtype, F &&f) { return dtype == CP_I64 ? f(int64_t()) : f(double()); }
// of a paired (Int64, Float64) argument, the one that belongs to TC
template <typename TC> inline TC *pick(int64_t *i64, double *f64);
template <> inline int64_t *pick<int64_t>(int64_t *i64, double *) { return i64; }
template <> inline double *pick<double>(int64_t *, double *f64) { return f64; }
template <typename TC> inline TC comp_const(const cp_component_t &c);
template <> inline int64_t comp_const<int64_t>(const cp_component_t &c) { return c.c_i64; }
template <> inline double comp_const<double>(const cp_component_t &c) { return c.c_f64; }

template <typename TC>
void build_dev_model(const cp_model_t *m, HostModel<TC> &H, hipStream_t s)
{
    memset(&H.d, 0, sizeof(H.d));
    H.d.kind = m->kind;
    for (int i = 0; i < 5; i++) H.d.p[i] = model_param<TC>(m, i);
    if (m->alpha_k && m->n_alpha_k > 0) {
        H.alpha_k.alloc((size_t)m->n_alpha_k);
        CP_HIP(hipMemcpyAsync(H.alpha_k.p, m->alpha_k, sizeof(TC) * (size_t)m->n_alpha_k, hipMemcpyHostToDevice, s));
        H.d.alpha_k = H.alpha_k.p;
        H.d.n_alpha_k = m->n_alpha_k;
    }
    H.d.R = m->R;
    auto up = [&](const cp_component_t &c, int slot, int32_t &is_c, TC &cc, const TC *&tab, int64_t &len, int64_t &lo) {
        is_c = c.is_const;
        cc = comp_const<TC>(c);
        tab = nullptr; len = 0; lo = c.lo;
        if (!c.is_const && c.table && c.len > 0) {
            H.tabs[slot].alloc((size_t)c.len);
            CP_HIP(hipMemcpyAsync(H.tabs[slot].p, c.table, sizeof(TC) * (size_t)c.len, hipMemcpyHostToDevice, s));
            tab = H.tabs[slot].p; len = c.len;
        }
    };
    if (m->kind == CP_MODEL_COLBLOCK || m->kind == CP_MODEL_BLOCK) {
        up(m->alpha_col, 0, H.d.ac_const, H.d.ac_c, H.d.ac_tab, H.d.ac_len, H.d.ac_lo);
        for (int r = 0; r < m->R && r < CP_MAX_R; r++)
            up(m->beta_col[r], 1 + r, H.d.bc_const[r], H.d.bc_c[r], H.d.bc_tab[r], H.d.bc_len[r], H.d.bc_lo[r]);
    }
}

}  // namespace cpk
