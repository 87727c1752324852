// envelope.hpp -- the envelope cost family: row span of a column range.
//   rowenvelope / EnvelopeMatrix   EnvelopeMatrices.jl:10-57
//   AffineEnvelopeModel            EnvelopeCosts.jl:5-20, oracle :66-73
//       f(j, j', k) = alpha_k + (j' - j)*b_vertex + (pos[j'] - pos[j])*b_pin + d*b_net,   d = max(hi - lo, 0),
//       (lo, hi) = env[j, j']: the least first row and the greatest last row of the columns [j, j'); an empty range is (m + 1, 0)
// Two structures hold the same integers, both built once per resident matrix and kept on the handle (cp_csr_s::env_work) until the
// cache is dropped:
//   the reference's implicit tree: H = cllog2(n), 2^(H+1) - 1 nodes, leaves past n padded with (m + 1, 0); cp_envelope_tree
//       downloads it and cp_envelope_query walks it bottom-up as getindex does;
//   a sparse table for the cost paths: level t holds the (lo, hi) of the 2^t columns from each start, so a range is two loads
//       (8 B * n * (floor(log2 n) + 1) of device memory).
// A header of its own, like sym.hpp and cut.hpp: dm_apply and OracleDev do not know this kind.
#pragma once
#include "csr.hpp"
#include "model.hpp"

namespace cpk {

// how the entries without an envelope path refuse the kind
#define CP_REFUSE_ENV(m, what) \
    CP_REQUIRE(!((m) && cpk::model_is_env((m)->kind)), CP_EUNSUPPORTED, "AffineEnvelopeModel has no device path in " what)

// per matrix, kept on the handle
struct EnvWork {
    bool have_tree = false, have_table = false;
    int32_t H = 0;                 // tree height
    int32_t L = 0;                 // table levels: floor(log2 n) + 1 (0 for n == 0)
    DBuf<int2> tree;               // node t (1-based, the reference's order) at tree[t - 1]; values are the reference's 1-based rows
    DBuf<int2> table;              // level t, start c (0-based) at table[t * n + c]: columns [c, min(c + 2^t, n))
    // workspace of the divide-and-conquer total layer (envelope_total.hip), dropped with the cache: four keys of 8 B per row, their
    // in-block tables (6 B per key and row), the tables over block minima (4 B per key, level and block of 64), one-row partials
    DBuf<int64_t> dc_kv, dc_pv;
    DBuf<uint8_t> dc_ib;
    DBuf<int32_t> dc_bt, dc_pa;
};
EnvWork *env_work_get(cp_csr_s *A);
void ensure_env_tree(cp_csr_s *A);         // needs n >= 1 (cllog2(0) has no meaning)
void ensure_env_table(cp_csr_s *A);

struct EnvDev {
    const int2 *tab;               // the sparse table (level 0: the per-column leaves)
    const int64_t *pos;            // A's column pointer (0-based)
    int64_t n;
    int32_t m;
};

__device__ __forceinline__ int2 env_join(int2 a, int2 b) { return make_int2(a.x < b.x ? a.x : b.x, a.y > b.y ? a.y : b.y); }

// d(p, r) of the 0-based column range [p, r): two loads
__device__ __forceinline__ int64_t env_span(const EnvDev &E, int64_t p, int64_t r)
{
    if (r <= p) return 0;
    const int t = 63 - __clzll((long long)(r - p));
    const int2 a = E.tab[(int64_t)t * E.n + p], b = E.tab[(int64_t)t * E.n + (r - ((int64_t)1 << t))];
    const int2 e = env_join(a, b);
    const int64_t d = (int64_t)e.y - (int64_t)e.x;
    return d > 0 ? d : 0;
}

// the model applied to its counts, left to right as the reference writes it (EnvelopeCosts.jl:20), one conversion per product
template <typename TC>
__host__ __device__ __forceinline__ TC env_apply(const TC *p, TC alpha, int64_t nv, int64_t np, int64_t d)
{
    return cadd(cadd(cadd(alpha, cmulc(nv, p[CP_P_VERTEX])), cmulc(np, p[CP_P_PIN])), cmulc(d, p[CP_P_NET]));
}

// the oracle of the Bisect splitters and the DP kernels; an oracle type of its own, so the kernels of the other models are
// instantiated unchanged
template <typename TC>
struct EnvOracleDev {
    DevModel<TC> M;
    int64_t n;
    EnvDev E;
};

template <typename TC>
__device__ __forceinline__ TC env_eval(const EnvDev &E, const DevModel<TC> &M, TC alpha, int64_t p, int64_t r)
{
    return env_apply(M.p, alpha, r - p, E.pos[r] - E.pos[p], env_span(E, p, r));
}

template <typename TC>
__device__ __forceinline__ TC oracle_eval_dev(const EnvOracleDev<TC> &O, int64_t j, int64_t jp, int64_t k)
{
    return env_eval<TC>(O.E, O.M, dm_alpha(O.M, k), j - 1, jp - 1);      // EnvelopeCosts.jl:66-73
}

// envelope.hip
extern int64_t g_env_valley_layers;        // DP layers the valley search ran (cp_get_stat("env_valley_layers"))
EnvDev env_prepare(cp_csr_s *A);           // builds the table if need be
template <typename TC>
int32_t run_env_eval(cp_csr_s *A, const cp_model_t *mdl, int64_t nq, const int64_t *j, const int64_t *jp, const int64_t *k, TC *out);
// bound_stripe, the model form (EnvelopeCosts.jl:43-53)
template <typename TC>
int32_t env_bound_stripe(cp_csr_s *A, int64_t K, const cp_model_t *mdl, TC *lo, TC *hi);
// is the valley search the literal bottleneck DP for this model?  
bool env_valley_ok(const cp_model_t *m, int64_t m_rows, int64_t n, int64_t N, int64_t K);
// the layers of the K-part DP in splitter order (dp_driver.hip loops over them); rows [r_lo, r_hi] 0-based
template <typename TC>
void env_layer1(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, TC *cst, int32_t *ptr);
template <typename TC>
void env_sweep_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, int32_t combine, const TC *W, TC *cst, int32_t *ptr,
                     int64_t r_lo, int64_t r_hi);
template <typename TC>
void env_valley_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst, int32_t *ptr,
                      int64_t r_lo, int64_t r_hi);

// envelope_total.hip: the total objective by divide and conquer over the cut column
extern int64_t g_env_dc_layers;            // DP layers >= 2 it ran (cp_get_stat("env_dc_layers"))
extern int64_t g_opt_env_dc_min_n;         // smallest n it takes; below, the candidate sweep (cp_set_option("env_dc_min_n"))
// are the regrouped sums the literal total DP for this model?  Any sign of the betas; exact integers only
bool env_dc_ok(const cp_model_t *m, int64_t m_rows, int64_t n, int64_t N, int64_t K);
// one row (r_lo == r_hi: a single reduction over the candidates) or all rows 0 .. n
template <typename TC>
void env_dc_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst, int32_t *ptr, int64_t r_lo, int64_t r_hi);

}  // namespace cpk
