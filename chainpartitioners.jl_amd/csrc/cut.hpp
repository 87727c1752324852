// cut.hpp -- the plaid edge-cut costs: pins of a part split by the row partition Pi into SELF pins (row owned by the same part
// number) and CUT pins (the others).
//   AffinePrimaryEdgeCutModel    /root/reference/src/PrimaryEdgeCutCosts.jl:5-18, oracle :51-57
//       f(j, j', k) = alpha_k + (j' - j)*b_vertex + l*b_self_pin + (w - l)*b_cut_pin,  w = pos[j'] - pos[j]
//   AffineSecondaryEdgeCutModel  /root/reference/src/SecondaryEdgeCutCosts.jl:5-18, oracle :78-85
//       f(i, i', k) = alpha_k + nv_k*b_vertex + l*b_self_pin + (w_k - l)*b_cut_pin,    nv_k / w_k: vertices / pins of part k of Pi
// with l = #{entries of the columns [j, j') whose row part k owns} in both.  The reference counts l through partwise(A, Pi) and a
// pin counter; here it is a difference of prefix counts by owner (plaid_cut.hip) or of the partwise column pointer (bisect.hip).
// A header of its own, like sym.hpp: dm_apply and OracleDev do not know these kinds, so the kernels of the other models are
// instantiated unchanged.
#pragma once
#include "csr.hpp"
#include "model.hpp"

namespace cpk {

inline bool model_is_cut(int32_t kind) { return kind == CP_MODEL_PRIMARY_EDGE_CUT || kind == CP_MODEL_SECONDARY_EDGE_CUT; }

// the model applied to its counts, left to right as the reference writes it (PrimaryEdgeCutCosts.jl:18), one conversion per product
template <typename TC>
__host__ __device__ __forceinline__ TC cut_apply(const TC *p, TC alpha, int64_t nv, int64_t nself, int64_t ncut)
{
    return cadd(cadd(cadd(alpha, cmulc(nv, p[CP_P_VERTEX])), cmulc(nself, p[CP_P_SELF_PIN])), cmulc(ncut, p[CP_P_CUT_PIN]));
}

// the oracle of the Bisect splitters over partwise(A, Pi) (PartwiseCounts.jl:1-60): the entries of part k in the columns < j are
// the partwise column pointer at the rank of j among the part's columns -- O(log) per call, no net counter
template <typename TC>
struct CutOracleDev {
    DevModel<TC> M;
    int64_t n;
    int32_t secondary;
    const int64_t *pos;                    // A's column pointer (0-based)
    const int64_t *pios, *prm, *ppos;      // partwise: part offsets (K+1), columns (n'), column pointer (n'+1); 1-based values
    const int64_t *spl, *tpos;             // secondary: the row split (1-based) and the row pointer of A (0-based)
};

// PartwiseCount rank (PartwiseCounts.jl:86-88): pios[k] + searchsortedfirst(prm[pios[k] : pios[k+1]-1], j) - 1
template <typename TC>
__device__ __forceinline__ int64_t cut_rank(const CutOracleDev<TC> &O, int64_t j, int64_t k)
{
    int64_t lo = O.pios[k - 1], hi = O.pios[k];
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        if (O.prm[mid - 1] < j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename TC>
__device__ __forceinline__ TC oracle_eval_dev(const CutOracleDev<TC> &O, int64_t j, int64_t jp, int64_t k)
{
    const int64_t l = O.ppos[cut_rank(O, jp, k) - 1] - O.ppos[cut_rank(O, j, k) - 1];
    const TC alpha = dm_alpha(O.M, k);
    if (O.secondary) {                                                     // SecondaryEdgeCutCosts.jl:78-85
        const int64_t s0 = O.spl[k - 1] - 1, s1 = O.spl[k] - 1;
        return cut_apply(O.M.p, alpha, s1 - s0, l, (O.tpos[s1] - O.tpos[s0]) - l);
    }
    return cut_apply(O.M.p, alpha, jp - j, l, (O.pos[jp - 1] - O.pos[j - 1]) - l);      // PrimaryEdgeCutCosts.jl:51-57
}

// what a kernel of plaid_cut.hip needs to evaluate the cost of part k
template <typename TC>
struct CutLayer {
    int32_t secondary;
    TC alpha;                  // alpha_k
    int64_t nvk, wk;           // secondary: vertices / pins of part k of Pi
    TC p[5];
};

// plaid_cut.hip
// One total-cost layer as a prefix-min scan with the reference's tie rule (the largest minimiser), for a cost of the form
// f(p, r, k) = constk + S_k[r] - S_k[p]:  cst[r] = constk + S_k[r] + min over p <= r of W[p] - S_k[p].  S_k comes from Y and the prefix
// counts Lc[0 .. n1): secondary form S_k[c] = Lc[c]*p[CP_P_SELF_PIN] - Lc[c]*p[CP_P_CUT_PIN] (pos unused), primary form as plaid_cut.hip
// states it.  Exact only while no intermediate rounds or wraps: the caller's gate.  Only enqueues.
template <typename TC> struct CutScanWork { DBuf<TC> tv, av; DBuf<int32_t> ti, ai; };
template <typename TC>
void cut_scan_layer(hipStream_t s, int64_t n1, const CutLayer<TC> &Y, TC constk, const int64_t *pos, const int32_t *Lc, const TC *W,
                    CutScanWork<TC> &ws, TC *cst, int32_t *ptr);
extern int64_t g_cut_scan_layers;          // DP layers the prefix-min scan ran (cp_get_stat("cut_scan_layers"))
template <typename TC>
int32_t run_cut_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp,
                     const int64_t *k, TC *out);
// the K-part DP; ptr_tab / cst_tab: the host tables of cp_dynamic_tables, or null
template <typename TC>
int32_t run_cut_dynamic(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, const cp_rowpart_t *Pi,
                        int64_t *spl_out, int64_t *ptr_tab, TC *cst_tab);
// bound_stripe: the primary form (PrimaryEdgeCutCosts.jl:28-39), the secondary model form (SecondaryEdgeCutCosts.jl:20-28) and the
// secondary oracle form (:40-57) the Bisect splitters get
template <typename TC>
int32_t cut_bound_stripe(cp_csr_s *A, int64_t K, const cp_rowpart_t *Pi, const cp_model_t *mdl, bool oracle_form, TC *lo, TC *hi);

}  // namespace cpk
