// sym.hpp -- the symmetric cost family: one partition for the rows and the columns of a square pattern
// (/root/reference/src/SymmetricConnectivityCosts.jl, MonotonizedSymmetricConnectivityCosts.jl, SymmetricEdgeCutCosts.jl).
//
// dianet(j, j') (SparseColorArrays.jl:72-99) is the net count of the derived pattern D: column j of A followed by one entry for
// row j iff the column does not hold it.  D never exists as rows: its column pointer dpos and its link array dprev (previous
// column of D holding the entry's row, -1 if none) are built from A's links, and its counter is the net counter over them.
// selfpin(j, j') (:281-318) counts the points (n+1 - min(i,j), max(i,j)) of the nonzeros, bucketed by max(i,j) with a stable
// sort: the nonzeros of A[j:j'-1, j:j'-1].
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include "wavelet.hpp"

namespace cpk {

// what the device needs to evaluate a symmetric cost on [p, r) (0-based columns)
struct SymDev {
    int32_t kind;
    int64_t n;
    const int64_t *pos;       // A's column pointer
    const int64_t *dpos;      // D's column pointer (kinds 10, 11)
    const int64_t *pin;       // prefix of max(deg - Delta_pins, 0) (kind 11): the reference's overpos, 0-based
    const int64_t *spos;      // entries with max(i, j) < c (kind 12)
    WaveletDev net, dia, selfpin;
};

// the three cost formulas, left to right as the reference writes them
template <typename TC>
__device__ __forceinline__ TC sym_eval(const SymDev &S, const DevModel<TC> &M, TC alpha, int64_t p, int64_t r)
{
    const int64_t nv = r - p;
    if (S.kind == CP_MODEL_MONO_SYM_CONNECTIVITY) {                         // MonotonizedSymmetricConnectivityCosts.jl:33, :107-113
        const int64_t w = S.pin[r] - S.pin[p];
        const int64_t d = (S.dpos[r] - S.dpos[p]) - wt_count_le(S.dia, S.n - p, S.dpos[r]);
        return cadd(cadd(cadd(alpha, cmulc(nv, M.p[CP_P_VERTEX])), cmulc(w, M.p[CP_P_OVER_PIN])), cmulc(d, M.p[CP_P_DIA_NET]));
    }
    const int64_t w = S.pos[r] - S.pos[p];
    if (S.kind == CP_MODEL_SYM_CONNECTIVITY) {                              // SymmetricConnectivityCosts.jl:19, :47-55
        const int64_t d = w - wt_count_le(S.net, S.n - p, S.pos[r]);
        const int64_t rem = (S.dpos[r] - S.dpos[p]) - wt_count_le(S.dia, S.n - p, S.dpos[r]) - nv;
        const int64_t loc = d - rem;
        return cadd(cadd(cadd(cadd(alpha, cmulc(nv, M.p[CP_P_VERTEX])), cmulc(w, M.p[CP_P_PIN])), cmulc(loc, M.p[CP_P_LOCAL_NET])),
                    cmulc(rem, M.p[CP_P_REMOTE_NET]));
    }
    const int64_t l = wt_count_le(S.selfpin, S.n - p, S.spos[r]);           // SymmetricEdgeCutCosts.jl:18, :37-43
    return cadd(cadd(cadd(alpha, cmulc(nv, M.p[CP_P_VERTEX])), cmulc(l, M.p[CP_P_SELF_PIN])), cmulc(w - l, M.p[CP_P_CUT_PIN]));
}

// per matrix, kept on the handle (cp_csr_s::sym_work) until the cache is dropped
struct SymWork {
    bool have_d = false, have_dia = false, have_selfpin = false, have_net = false;
    int64_t Nd = 0;                       // entries of D
    DBuf<int64_t> dpos;                   // n+1
    DBuf<int32_t> dpos32, dprev, dnext;   // n+1 / Nd (+16: vector loads may over-read the tail); dnext: next column of D holding the row, n if none
    // the over-pin prefix of the last Delta_pins asked for (a partition call asks for its bound first, then runs)
    bool have_pin = false;
    int64_t pin_delta = 0, over_total = 0;
    DBuf<int64_t> pin;                    // n+1
    DBuf<int32_t> pin32;
    DBuf<int64_t> spos;                   // n+1
    WaveletHost dia, selfpin, net;
    // the scratch and launch plans of the total-cost layers (sym_total.hip owns the type)
    void *total = nullptr;
    void (*total_free_fn)(void *) = nullptr;
    ~SymWork() { if (total && total_free_fn) total_free_fn(total); }
};
SymWork *sym_work_get(cp_csr_s *A);
void ensure_sym_links(cp_csr_s *A);                                                  // dpos, dpos32, dprev, dnext
void build_dianet_counter(cp_csr_s *A, WaveletHost &out);                            // (a fresh structure: count handles own theirs)
void build_selfpin_counter(cp_csr_s *A, WaveletHost &out, DBuf<int64_t> &spos);

// one call's view: the cached structures of the model's kind plus the pin prefix of its Delta_pins
struct SymHost {
    SymDev d{};
    const int32_t *pin32 = nullptr;
    int64_t over_total = 0;               // sum of max(deg - Delta_pins, 0)
};
// validates (square pattern, integer-valued Delta_pins, 32-bit layout of D) and builds what is missing; counters = false: the pin
// prefix only (bound_stripe needs no counter)
void sym_prepare(cp_csr_s *A, const cp_model_t *mdl, SymHost &S, bool counters = true);

template <typename TC>
int32_t run_sym_eval(cp_csr_s *A, const cp_model_t *mdl, int64_t nq, const int64_t *j, const int64_t *jp, const int64_t *k, TC *out);
// the DP layers of dp_driver.hip for these kinds: every candidate evaluated through the counters
template <typename TC>
void sym_layer1(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, TC *cst, int32_t *ptr);
template <typename TC>
void sym_brute_layer(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, int32_t combine, const TC *W, TC *cst_out,
                     int32_t *ptr_out, int64_t r_lo, int64_t r_hi);

}  // namespace cpk
