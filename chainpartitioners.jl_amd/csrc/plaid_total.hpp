// plaid_total.hpp -- the exact total-cost DP of the plaid connectivity pair (kinds 8 / 9) past the candidate sweep: plaid_total.hip.
#pragma once
#include "dp.hpp"
#include <memory>

namespace cpk {

// The engine that runs a K-layer DP of AffinePrimaryConnectivityModel / AffineSecondaryConnectivityModel.  plaid_path (plaid_total.hip)
// is the one place that decides it.
enum class PlaidPath {
    Sweep,         // plaid.hip: the O(n^2) candidate sweep (k_plaid_layer), n <= brute_max_n
    Total,         // primary inside plaid_total_ok: the rectangle engine of lws_rect.hpp with the plaid cell
    Scan,          // secondary inside plaid_scan_exact: the prefix-min scan of plaid_cut.hip
};
// Pure: no allocation, no launch.  Raises CP_EUNSUPPORTED where only the sweep is left and n > brute_max_n.
PlaidPath plaid_path(const cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl);

extern int64_t g_opt_plaid_total;              // 1: on
extern int64_t g_opt_plaid_total_min_n;        // the smallest n the primary path takes where the sweep is allowed too
extern int64_t g_opt_plaid_scan_min_n;         // ... and the secondary scan
constexpr int64_t PLAID_TOTAL_FLOOR = 1024;    // the primary path where the sweep would be refused (n > brute_max_n): LWS_STAIR_COLS
extern int64_t g_opt_plaid_total_scan_cells, g_opt_plaid_total_scan_cols, g_opt_plaid_total_stair_cols;      // the engine's limits
extern int64_t g_plaid_total_layers, g_plaid_scan_layers;      // layers >= 2 each path ran since the last reset

// the state of one K-layer run on either new path: partwise(A, Pi) staged once, the engine's scratch and plans, the scan's buffers
struct PlaidTotalRun { virtual ~PlaidTotalRun() = default; };
template <typename TC>
std::unique_ptr<PlaidTotalRun> plaid_total_begin(cp_csr_s *A, PlaidPath path, const cp_model_t *mdl, const DevModel<TC> &M, const cp_rowpart_t *Pi,
                                                 const PlaidPart &R);
// layer k (1-based) for the rows [rlo, rhi] (0-based); W: the previous layer's cost row (unused for k == 1).  Only enqueues.
template <typename TC>
void plaid_total_layer(PlaidTotalRun *run, int64_t k, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi);

}  // namespace cpk
