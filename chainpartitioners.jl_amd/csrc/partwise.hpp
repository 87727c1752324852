// partwise.hpp -- partwise(A, Pi) (PartwiseCounts.jl:1-60) staged on the device for the callers that evaluate a plaid cost by
// random access: the Bisect splitters (bisect.hip) and the total-cost DP of the plaid connectivity pair (plaid_total.hip).
#pragma once
#include "csr.hpp"
#include "wavelet.hpp"
#include <vector>

namespace cpk {

enum PartwiseNeed {
    PW_RANK,       // pios / prm only: the rank of a column among a part's columns (the secondary connectivity cost)
    PW_PINS,       // + the partwise column pointer (the edge-cut pair: a part's pins are a prefix difference, no counter)
    PW_NETS,       // + the partwise matrix with its net counter (the primary connectivity cost: a part's local nets)
};

struct PartwiseStage {
    int64_t Kp = 0, npr = 0;                     // parts of Pi, columns of the partwise matrix
    std::vector<int64_t> hpios;                  // Kp + 1 part offsets, 1-based as the reference's (also on the host: d_k = hpios[k] - hpios[k-1])
    DBuf<int64_t> pios, prm;                     // Kp + 1 / n' : 1-based values
    DBuf<int64_t> ppos;                          // PW_PINS: n' + 1, 1-based values
    cp_csr_t Ap = nullptr;                       // PW_NETS: the partwise matrix (its pos is the 0-based column pointer) ...
    WaveletHost lcn;                             // ... and its net counter
    PartwiseStage() = default;
    PartwiseStage(const PartwiseStage &) = delete;
    PartwiseStage &operator=(const PartwiseStage &) = delete;
    ~PartwiseStage() { if (Ap) cp_csr_destroy(Ap); }
};

// Pi: any row partition (asg or spl, checked by the caller to be one of them).  Synchronises the stream: the host staging vectors
// die inside.  Returns the C ABI's status.
int32_t partwise_stage(cp_csr_s *A, const cp_rowpart_t *Pi, PartwiseNeed need, PartwiseStage &S);

}  // namespace cpk
