// dp.hpp -- internal interfaces between the DP translation units: the engine a K-layer run takes (DpPath), the route of a
// ConstrainedCost (ConstrainedRoute), the drivers' entries and the per-layer functions of every engine.
#pragma once
#include "csr.hpp"
#include "model.hpp"

namespace cpk {

// The engine that runs the layers k >= 2 of a K-layer DP.  dp_path (dp_driver.hip) is the one place that decides it; the gates it
// combines stay with their arguments: fast_total_ok (model.hpp), fast_bottleneck_ok (dp_driver.hip), env_valley_ok (envelope.hip),
// env_dc_ok (envelope_total.hip).
enum class DpPath {
    Total,         // dp_total.hip: the O(n log^2 n) scheme for inverse-Monge totals; under a weight's j0 array dp_total_budget.hip
    Valley,        // dp_bottleneck.hip: the valley search for bottleneck costs that grow with their part
    SymValley,     // ... over the derived pattern of the monotonized symmetric model (sym.hpp)
    SymTotal,      // sym_total.hip: the total objective of the symmetric family by divide and conquer (sym_total_ok, model.hpp)
    SymSweep,      // sym.hip: the O(n^2) candidate sweep over the symmetric counters
    EnvValley,     // envelope.hip: the valley search of the envelope cost
    EnvDc,         // envelope_total.hip: its total objective by divide and conquer
    EnvSweep,      // envelope.hip: its O(n^2) candidate sweep
    Sweep,         // dp_brute.hip: the general O(n^2) sweep
};
// Pure: no allocation, no launch.  Raises CP_EUNSUPPORTED where only a sweep is left and n > brute_max_n.
DpPath dp_path(const cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *model);

}  // namespace cpk

// The handle of the row-tiled step protocol (cp_dp_t) and the base of the K-layer driver DpRun<TC> (dp_driver.hip): what does not
// depend on the cost type.
struct cp_dp_s {
    cp_csr_s *A = nullptr;
    int64_t K = 0;
    int32_t combine = 0, order = 0;
    cpk::DpPath path = cpk::DpPath::Sweep;     // the engine of the layers k >= 2 (dp_path)
    void *work = nullptr;                      // scratch of the total-cost layers (dp_total_work_get)
    cpk::DBuf<int32_t> ptr;                    // K x (n+1) argmins; a step handle fills only its tile rows of layers >= 2
    // step protocol only
    int64_t rlo = 0, rhi = 0;                  // 0-based inclusive row tile (cp_dp_set_rows moves it between layers)
    int64_t wwin = 0;                          // > 0: layers k >= 2 take their candidates from the width window max(0, r - wwin) <= p <= r (cp_dp_set_window)
    std::vector<int64_t> lay_lo, lay_hi;       // the row tile every layer was computed with
    virtual ~cp_dp_s() = default;
    virtual int32_t step_layer(int64_t k, const void *cst_prev_device, void *cst_cur_device) = 0;      // cp_dp_layer
    virtual int32_t block_tables(int32_t *nplanes_out, int64_t *opt_out, int64_t *nets_out, int64_t *selfnets_out) = 0;
};

namespace cpk {

using DpBase = ::cp_dp_s;

// candidate limits of a weight-constrained layer (0-based); default-constructed: unconstrained
struct DpWindow {
    int64_t w = 0;                             // row r takes its candidates from p >= r - w (0: no width)
    int64_t lo = 0, hi = -1;                   // and from the previous layer's row window [lo, hi] (bottleneck; hi < 0: none)
    const int32_t *j0 = nullptr;               // device array (n + 1): p >= j0[r] instead of the width (a general weight)
    const int32_t *j0_host = nullptr;          // ... and its host copy (the total-cost layers of dp_total_budget.hip decompose on the host)
};

// How the DP under ConstrainedCost(f, weight, w_max) runs (constrained_route, dp_driver.hip: the one place that decides it).
struct ConstrainedRoute {
    enum Kind {
        OneWave,   // outside the scalable paths: the one-wave literal kernel (run_dyn_constrained, seq.hip)
        Width,     // parts of at most `width` columns: the windowed geometry of dp_total.hip (sum), the valley search with r - width (max)
        Weight,    // the weight's j0 array: the budget divide and conquer of dp_total_budget.hip (sum), the valley search (max)
    } kind;
    int64_t width;
};
// weight == null: the width w_max = wmax_i64 itself
ConstrainedRoute constrained_route(cp_csr_s *A, int64_t K, int32_t combine, const cp_model_t *model, const cp_model_t *weight,
                                   int64_t wmax_i64, double wmax_f64);

// optional host tables of the drivers below, (n + 1) x K and K entries; cst_i64 / cst_f64: the one matching model->dtype is used
struct DpTables {
    int64_t *ptr_tab = nullptr, *cst_i64 = nullptr;
    double *cst_f64 = nullptr;
    int64_t *win_lo = nullptr, *win_hi = nullptr;          // the layers' row windows (run_dynamic_windowed)
};

// dp_driver.hip: the K-layer drivers.
int32_t run_dynamic(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, int64_t *spl_out, const DpTables &tabs = DpTables());
// route: Width or Weight (constrained_route admitted the pair: never an O(n^2) sweep)
int32_t run_dynamic_windowed(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, ConstrainedRoute route,
                             const cp_model_t *weight, int64_t wmax_i64, double wmax_f64, int64_t *spl_out, const DpTables &tabs = DpTables());
int32_t dp_begin(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *model, int64_t row_lo, int64_t row_hi,
                 cp_dp_s **out);

// one layer of the total-cost DP by the O(n log^2 n) scheme (dp_total.hip)
template <typename TC>
void dp_total_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, void *work,
                    int64_t rlo, int64_t rhi,       // computes rows r in [rlo, rhi] (0-based); the full range is [0, n]
                    int64_t wwin = 0);              // > 0: width window -- the candidates of row r are max(0, r - wwin) <= p <= r
template <typename TC> int dp_total_block_tables(cp_csr_s *A, void *work, int64_t *opt_out, int64_t *nn_out, int64_t *nl_out);   // per-block winners of the last layer (tests)
template <typename TC> void *dp_total_work_get(cp_csr_s *A);      // the handle's scratch for cost type TC (created on first use)
template <typename TC> void *dp_total_work_new();
template <typename TC> void dp_total_work_free(void *w);

// one layer by the general O(n^2) sweep, any combine / any model sign pattern (dp_brute.hip).
// rows [r_lo, r_hi] are computed; window (lo/hi per row) optional.
template <typename TC>
void dp_brute_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, int32_t combine, const TC *W, TC *cst_out,
                    int32_t *ptr_out, int64_t r_lo, int64_t r_hi);

// a pattern other than A's own for the valley search: column pointer, link arrays and net counter of the derived pattern D of
// sym.hpp, and the prefix array the pin count is read from (the monotonized symmetric model)
struct WaveletDev;
struct BnPattern {
    const int64_t *pos; const int32_t *pos32, *pin32, *prev, *next;
    int64_t N;
    const WaveletDev *net;
};
extern int64_t g_bn_sym_layers;                // layers the valley search ran over such a pattern (cp_get_stat("bn_sym_layers"))

// one layer of the bottleneck (g = max) DP for costs that grow with their part, by the valley search (dp_bottleneck.hip)
template <typename TC>
void dp_bottleneck_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out,
                         int64_t r_lo, int64_t r_hi,
                         // candidate limits of a weight-constrained layer (0-based; defaults: none): row r takes max(p_lo0, j0(r)) <= p <= min(r, p_hi0),
                         // j0(r) = r - wwin, or j0[r] when the device array j0 (n + 1 entries) is given
                         int64_t wwin = 0, int64_t p_lo0 = 0, int64_t p_hi0 = -1, const int32_t *j0 = nullptr,
                         const BnPattern *pat = nullptr);      // null: A's own links, counter and pins
extern int64_t g_opt_bn_wave, g_opt_bn_run, g_opt_bn_slack;    // wave-per-run walk (default) and its rows per wave
extern int64_t g_opt_bn_chunk;                 // rows per two-pointer walk (one lane each)

// dp_total_budget.hip: one layer of the total-cost DP under a monotone work budget, for the inverse-Monge models at any n.
// Rows [rlo, rhi] (0-based); row r takes its candidates from max(j0[r], p_lo0) <= p <= min(r, p_hi0), ties -> the largest p; W is
// read inside [p_lo0, p_hi0] only.  j0_dev / j0_host: the weight's j0 array (k_weight_j0) on both sides.  Only enqueues.
template <typename TC>
void dp_total_budget_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi,
                           int64_t p_lo0, int64_t p_hi0, const int32_t *j0_dev, const int32_t *j0_host);
// the gate of that path: an inverse-Monge model with exact totals (fast_total_ok) of kind Work / Connectivity / HyperedgeCut, a monotone
// AffineWorkModel weight without per-part alpha that is not a width and cannot wrap, n < 2^30, N < 2^31 - 1, no force_brute, and
// cp_set_option("budget_total", 1) (the default)
bool budget_total_ok(const cp_csr_s *A, int64_t K, const cp_model_t *model, const cp_model_t *weight, int64_t wmax_i64, double wmax_f64);
extern int64_t g_opt_budget_total;             // 1: on
extern int64_t g_opt_budget_scan_cells, g_opt_budget_scan_cols, g_opt_budget_stair_cols;      // rectangles within both limits / partial rows of blocks below stair_cols columns are scanned whole
extern int64_t g_budget_layers;                // layers that path ran since the last reset (cp_get_stat("budget_layers"))

// sym_total.hip: one layer of the unconstrained total-cost DP of a symmetric model inside sym_total_ok, at any n.  Rows [rlo, rhi]
// (0-based); row r takes its candidates from 0 <= p <= r, ties -> the largest p.  Only enqueues.
struct SymDev;
template <typename TC>
void sym_total_layer(cp_csr_s *A, const SymDev &S, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, int64_t rlo, int64_t rhi);
extern int64_t g_opt_sym_total;                // 1: on
extern int64_t g_opt_sym_total_min_n;          // the smallest n that path takes where the sweep is allowed too (the measured crossover)
constexpr int64_t SYM_TOTAL_FLOOR = 1024;      // ... and where the sweep would be refused (n > brute_max_n): LWS_STAIR_COLS
extern int64_t g_opt_sym_total_batch;          // 1: the rectangles of one depth of the column tree share one launch sequence; 0: one per rectangle
extern int64_t g_opt_sym_total_scan_cells, g_opt_sym_total_scan_cols, g_opt_sym_total_stair_cols;      // as the budget path's limits
extern int64_t g_sym_total_layers;             // layers that path ran since the last reset (cp_get_stat("sym_total_layers"))

// seq.hip
template <typename TC>
int32_t run_dyn_constrained(cp_csr_s *A, int64_t K, int32_t g, int32_t order, const cp_model_t *mdl, const cp_rowpart_t *Pi,
                            const cp_model_t *w, int64_t wi, double wf, int64_t *spl_out);
template <typename TC>
int32_t run_seq_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp,
                     const int64_t *k, TC *out);

// plaid.hip: primary / secondary connectivity costs (need a row partition)
// device copy of the row partition: owner (1-based part of every row) and the split vector (the secondary models); also plaid_cut.hip
struct PlaidPart {
    DBuf<int32_t> owner;
    DBuf<int64_t> spl;
    std::vector<int64_t> hspl;
    int64_t K = 0;
};
void upload_part(cp_csr_s *A, const cp_rowpart_t *Pi, bool need_spl, PlaidPart &R);
template <typename TC>
int32_t run_plaid_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp,
                       const int64_t *k, TC *out);
// the K-part DP; ptr_tab / cst_tab: the host tables of cp_dynamic_tables, or null
template <typename TC>
int32_t run_plaid_dynamic(cp_csr_s *A, int64_t K, int32_t combine, int32_t order, const cp_model_t *mdl, const cp_rowpart_t *Pi,
                          int64_t *spl_out, int64_t *ptr_tab = nullptr, TC *cst_tab = nullptr);

// chunk_scan.hip: DynamicTotalChunker under a VertexCount window as a (min,+) scan; false = not applicable
template <typename TC>
bool pack_dynamic_scan(hipStream_t s, int64_t n, int64_t wmax, const TC *Ftab, TC *cst1, int64_t *spl1);

// chunk_lws.hip: DynamicTotalChunker for any width or monotone work budget as an on-line divide and conquer; lws_ok: the gate
// (cp_set_option("lws", 0) restores the one-wave kernel); run_pack_lws fills the 1-based tables of k_pack_dynamic (spl1 zeroed)
extern int64_t g_opt_lws, g_opt_lws_leaf;      // on / rows per leaf wave (256, 512, 1024 or 2048)
bool lws_ok(const cp_csr_s *A, const cp_model_t *mdl, const cp_model_t *w, int64_t wi, double wf);
template <typename TC>
int32_t run_pack_lws(cp_csr_s *A, const DevModel<TC> &M, const WaveletDev &wnet, const WaveletDev &wself, const cp_model_t *w, int64_t wi,
                     double wf, TC *cst1, int64_t *spl1);

extern int64_t g_opt_gap_nr;                      // 64-row chunks per wave of the gap finish (1 or 2)
extern int64_t g_opt_gap_tau, g_opt_gap_min;   // gap passes in the rounds tau <= gap_tau (-1: none) for tasks of >= gap_min candidates
extern int64_t g_opt_poison, g_poison_hits;    // poison mode (tests): see run_layer
void dp_round_scans_test(const int32_t *a, int64_t na, int64_t na_max, const int32_t *b, int64_t nb, int64_t nb_max, int two, int64_t capT, int64_t capNT,
                         int err_in, int reps, int64_t *offs_out, int64_t *toffs_out, int64_t *res);      // dp_total.hip: cp_test_round_scans
void dp_fix_merge_test(const cp_model_t *model, int64_t ntask, const int64_t *toffs, const int64_t *part_v, const int32_t *part_p, const int32_t *part_nn,
                       const int32_t *part_nl, const int32_t *tile_s, const int32_t *tile_s2, const int32_t *anchor, const int32_t *anchor2, const int32_t *row,
                       const int32_t *plane, int64_t n, int reps, int32_t *p_out, int32_t *nn_out, int32_t *nl_out, int64_t *res);      // dp_total_own.hip: cp_test_fix_merge
extern int64_t g_fix_trips, g_fix_edges;       // what the own-tile merges met since the last reset (tests): see RoundCounts::n_trips / n_edge
extern int64_t g_fix_items;                    // ... and the (task, trip) items they merged, attempts that were redone included (RoundCounts::n_items)
extern int64_t g_opt_leaf;                     // 1: the rounds tau < 6 of an unconstrained layer are one leaf pass (dp_total_leaf.hip)
extern int64_t g_opt_block_tables;             // 1: the leaf pass also stores the per-block winners (cp_dp_block_tables)
extern int64_t g_opt_ra_cache;                 // 1: round A from counts computed once per partition
extern int64_t g_opt_fixed_point;              // 1: layers after a layer that reproduced its input row are copied (run_dynamic)
extern int64_t g_opt_nospec;                   // 1: every layer waits for its exact counts (one host sync per round)
extern int64_t g_spec_redo;                    // layers redone because the prediction missed (diagnostics)
extern int64_t g_opt_rpass_small_tau;           // rounds tau <= this use one lane per row in the right-part pass
extern int64_t g_opt_force_max;                 // see run_layer (force_own)
extern int64_t g_opt_setup_bs;                  // lanes per block of k_setup_short
extern int64_t g_opt_rpass_cap;                 // lane-private entries per row in k_rpass_small, per cent of the mean (200)
extern int64_t g_opt_rpass_ch;                 // columns per wave in k_rpass_wave (power of two >= 16)
extern int64_t g_opt_own_min;                  // tasks with at least this many steps get tiles of their own (>= 64)
extern int64_t g_opt_own_blk;                  // 1: their tiles sit at 256-column blocks and run in block order; 0: tiles counted from each task head (k_own_map)
extern int64_t g_opt_own_split;                // 1: outside round A the own tiles of the planes >= 8 stream only the plane's variable link entries (the gap rounds: gap_split)
extern int64_t g_own_split_tiles;              // own tiles that took that path since the last reset (RoundCounts::n_split)
extern int64_t g_opt_gap_split;                // 1 (and own_split 1): the gap rounds' tiles of the planes >= 8 do the same
extern int64_t g_gap_split_tiles;              // gap tiles that took that path since the last reset (not counted in own_split_tiles)
extern int64_t g_opt_own_pair;                 // 1: outside the gap rounds and the hyperedge costs a wave of k_lpass_own takes two slots of the run order
extern int64_t g_own_pair_waves, g_own_pair_lone;      // waves that ran two tiles / one because the order ended, since the last reset
void dp_own_pair_test(int64_t nt, int64_t wave, int64_t *res);      // dp_total_own.hip: cp_test_own_pair
extern int64_t g_opt_own_pack;                 // 1 (and own_split 1, own_blk 1): split tiles read one packed word per step where the pattern's in-block offsets fit 16 bits
extern int64_t g_own_pack_tiles, g_own_pack_wide;      // tiles that ran packed since the last reset; 1: the pattern of the last split launch fell back to the wide arrays
void dp_own_pack_test(cp_csr_s *A, int32_t *vpk_out, int32_t *vbase_out, int64_t *res);      // dp_total_own.hip: cp_test_own_pack
extern int64_t g_opt_round_alloc;              // 1: k_setup_short reserves list slots and offsets in one atomic per list and block, its last block gives the round's verdict; 0: k_round_scans
void dp_list_alloc_test(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int bs, int64_t capT, int64_t capNT, int64_t o_cap, int err_in, int reps,
                        int64_t fit_ntask, int64_t fit_n, int64_t fit_own_min, int64_t *offs_out, int32_t *slot_a, int64_t *toffs_out, int32_t *slot_b,
                        int32_t *ioffs_out, int64_t *res);      // dp_total.hip: cp_test_list_alloc
extern int64_t g_round_alloc_rounds;          // rounds that took that path since the last reset
extern int64_t g_opt_cr_consume;               // 1: in full layers k_setup_short zeroes the cr / crl cells it reads; the clearing launch runs only while the planes may be dirty
extern int64_t g_cr_consume_rounds, g_cr_clear_launches;      // chunked right passes that ran without / with the clearing launch since the last reset
extern int64_t g_overlap_isect;                // column intersections cp_pack_overlap computed since the last reset (chunk_greedy.hip)
void dp_own_split_test(cp_csr_s *A, int32_t *vpos_out, int32_t *vsa_out, int32_t *vnext_out, int64_t *res);      // dp_total_own.hip: cp_test_own_split
extern int64_t g_opt_short_t, g_opt_short_e;   // k_setup_short: tasks with <= short_t candidates and <= short_e link entries finish in setup
extern int64_t g_opt_force_brute;      // cp_set_option("force_brute", 1)
extern int64_t g_opt_brute_max_n;      // largest n the O(n^2) path accepts
extern int64_t g_opt_dbg;            // cp_set_option("dbg", mask): timing experiments; every bit leaves the tables unchanged (the tests demand it)
// The bits of that mask (callers pass the numbers; the same table is in DESIGN.md section 4e).  Bits 1, 2, 4, 16, 8192, 32768, 65536,
// 131072 and 16777216 are free.  33554432 has one meaning in dp_total.hip and another in dp_bottleneck.hip: take a free bit, not a
// third meaning.
enum DbgBit : int64_t {
    DBG_PRINT_ROUNDS = 8,                // total DP: every round's task counts to stderr
    DBG_NO_INTERIOR = 32,                // k_tile_t0 marks no tile as interior to one task (k_lpass takes its general path everywhere)
    DBG_NO_OWN_TILES = 64,               // every long task stays in the flattened space (no k_lpass_own, no gap passes)
    DBG_POISON = 128,                    // fill the per-tile buffers of a stage before it runs: 0x7F bytes ...
    DBG_POISON_ZERO = 256,               // ... or, with this bit too, zero bytes
    DBG_GAP_ALL_SPECIAL = 512,           // k_lpass_own flags every gap tile: the SLOW gap kernels walk them entry by entry
    DBG_MISPREDICT = 1024,               // speculative layers: every odd round is predicted empty (stages with work are skipped, the layer redone)
    DBG_TINY_BUFFERS = 2048,             // speculative layers: the round verdicts take the buffers for too small (every round dropped, the layer redone)
    DBG_COUNT_NONTRIVIAL = 4096,         // k_setup_short counts the tasks it does not finish itself (RoundCounts::_pad, printed by DBG_PRINT_ROUNDS)
    DBG_COMBINE_BY_SLOT = 16384,         // k_combine / k_combine_win without the leaf pass: threads in plane-slot order
    DBG_RA_ROWMAJOR = 262144,            // unconstrained round A from the cache by the row-major kernel k_ra_layer
    DBG_NO_FORCE_OWN = 524288,           // no round trades its flattened stage for own tiles (LayerWork::force_own ignored)
    DBG_WIN_NO_RA_CACHE = 1048576,       // windowed layers: round A without the cached tables (every head a generic task)
    DBG_WIN_NO_MIR_CACHE = 2097152,      // windowed layers: standard heads from the cache, mirrored heads as generic tasks
    DBG_BN_NO_HINT2 = 4194304,           // bottleneck: starts from the last layer's crossings only, not extrapolated from the last two
    DBG_MIR_ROWMAJOR = 8388608,          // windowed layers: the mirrored heads from their cache by the row-major kernel k_ra_layer
    DBG_RA_ALL_LEVELS = 33554432,        // total DP: round A from the cache computes the levels below LEAF_T too, as without the leaf pass
    DBG_BN_NO_HINT_STARTS = 33554432,    // bottleneck (SAME BIT): the wave-per-run walk brackets its starts instead of taking them from the hint
};

}  // namespace cpk
