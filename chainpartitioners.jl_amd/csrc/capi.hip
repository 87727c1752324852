// capi.hip -- extern "C" entry points of libchainpart.so (include/chainpart.h): argument checks and dispatch.  The K-layer DP
// drivers behind cp_partition_dynamic, cp_dynamic_tables* and cp_dp_* are in dp_driver.hip.
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include "sym.hpp"
#include "cut.hpp"
#include "plaid_total.hpp"
#include "envelope.hpp"
#include "blockcost.hpp"
#include <cmath>
#include <memory>

using namespace cpk;

namespace cpk {

// ------------------------------------------------------------------ small kernels of the oracle batches
// counts for (p, r) ranges: nets = #{q in cols [p,r) : prev[q] < p}, selfnets = #{rows with first in [p,r) and last < r}.
// gridDim.y blocks share one query (grid-stride over its entries) and combine with one atomic per block.
__global__ void __launch_bounds__(256) k_range_counts(int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ Rr,
                                                      const int64_t *__restrict__ pos, const int32_t *__restrict__ prev,
                                                      const int64_t *__restrict__ fpos, const int32_t *__restrict__ flast,
                                                      unsigned long long *__restrict__ nets, unsigned long long *__restrict__ selfnets)
{
    int64_t i = blockIdx.x;
    if (i >= nq) return;
    __shared__ int64_t sh[256];
    int64_t p = P[i], r = Rr[i];
    int64_t stride = (int64_t)gridDim.y * 256, start = (int64_t)blockIdx.y * 256 + threadIdx.x;
    int64_t c = 0;
    if (r > p) {
        int64_t q0 = pos[p], q1 = pos[r];
        int32_t thr = (int32_t)p;
        for (int64_t q = q0 + start; q < q1; q += stride) c += (prev[q] < thr);
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < (unsigned)o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0 && sh[0]) atomicAdd(&nets[i], (unsigned long long)sh[0]);
    __syncthreads();
    if (selfnets) {
        c = 0;
        if (r > p) {
            int64_t s0 = fpos[p], s1 = fpos[r];
            int32_t thr = (int32_t)r;
            for (int64_t s = s0 + start; s < s1; s += stride) c += (flast[s] < thr);
        }
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < (unsigned)o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0 && sh[0]) atomicAdd(&selfnets[i], (unsigned long long)sh[0]);
    }
}

template <typename TC>
__global__ void k_apply_model(int64_t nq, const int64_t *__restrict__ P, const int64_t *__restrict__ Rr, const int64_t *__restrict__ Kk,
                              const int64_t *__restrict__ pos, const int64_t *__restrict__ nets, const int64_t *__restrict__ selfnets,
                              DevModel<TC> M, TC *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    int64_t p = P[i], r = Rr[i];
    TC alpha = dm_alpha(M, Kk ? Kk[i] : (int64_t)0);
    out[i] = dm_apply(M, alpha, r - p, pos[r] - pos[p], nets ? nets[i] : (int64_t)0, selfnets ? selfnets[i] : (int64_t)0);
}

// ------------------------------------------------------------------ helpers
static bool model_known(const cp_model_t *m)
{
    if (!m || m->kind < CP_MODEL_FEASIBLE || m->kind > CP_MODEL_ENVELOPE) return false;
    if (m->kind == CP_MODEL_POWER_WORK) return m->dtype == CP_F64;
    return m->dtype == CP_I64 || m->dtype == CP_F64;
}

// ------------------------------------------------------------------ ocl(j, j', k) batches
template <typename TC>
static int32_t run_oracle_eval(cp_csr_s *A, const cp_model_t *mdl, int64_t nq, const int64_t *j, const int64_t *jp,
                               const int64_t *k, TC *out)
{
    hipStream_t s = A->stream;
    if (nq <= 0) return CP_OK;
    bool has_nets = mdl->kind == CP_MODEL_CONNECTIVITY || mdl->kind == CP_MODEL_HYPEREDGE_CUT || mdl->kind == CP_MODEL_COLBLOCK;
    bool need_self = mdl->kind == CP_MODEL_HYPEREDGE_CUT;
    if (has_nets) ensure_links(A);
    if (need_self) ensure_self(A);
    std::vector<int64_t> hp((size_t)nq), hr((size_t)nq);
    for (int64_t i = 0; i < nq; i++) {
        CP_REQUIRE(j[i] >= 1 && jp[i] >= j[i] && jp[i] <= A->n + 1, CP_EINVAL, "oracle query needs 1 <= j <= j' <= n+1");
        hp[i] = j[i] - 1; hr[i] = jp[i] - 1;
    }
    DBuf<int64_t> dP((size_t)nq), dR((size_t)nq), dK, dN, dS;
    DBuf<TC> dO((size_t)nq);
    CP_HIP(hipMemcpyAsync(dP.p, hp.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(dR.p, hr.data(), sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    if (k) { dK.alloc((size_t)nq); CP_HIP(hipMemcpyAsync(dK.p, k, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s)); }
    if (has_nets) {
        dN.alloc((size_t)nq);
        CP_HIP(hipMemsetAsync(dN.p, 0, dN.bytes(), s));
        if (need_self) { dS.alloc((size_t)nq); CP_HIP(hipMemsetAsync(dS.p, 0, dS.bytes(), s)); }
        int64_t per = nq > 0 ? A->N / nq : 0;
        unsigned gy = (unsigned)(per / 65536 + 1);                   // ~64k entries per block
        if (gy > 2048) gy = 2048;
        ProfScope ps(PROF_QUERY, s, 0.0);
        hipLaunchKernelGGL(k_range_counts, dim3((unsigned)nq, gy), dim3(256), 0, s, nq, dP.p, dR.p, A->pos.p, A->prev.p,
                           need_self ? A->fpos.p : nullptr, need_self ? A->flast.p : nullptr, (unsigned long long *)dN.p,
                           need_self ? (unsigned long long *)dS.p : nullptr);
    }
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_apply_model<TC>), dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, s, nq, dP.p, dR.p,
                       k ? dK.p : nullptr, A->pos.p, has_nets ? dN.p : nullptr, need_self ? dS.p : nullptr, HM.d, dO.p);
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(out, dO.p, sizeof(TC) * (size_t)nq, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

// ------------------------------------------------------------------ what differs between the Int64 and the Float64 body of an entry
static int64_t fld(int64_t a, int64_t b)                    // fld(a, b): Int64 floor division ...
{
    int64_t q = a / b, r = a % b;
    if (r != 0 && ((r < 0) != (b < 0))) q -= 1;
    return q;
}
static double fld(double a, int64_t b) { return std::floor(a / (double)b); }      // ... and floor(a / b) of Float64 costs
static int64_t max_identity(int64_t) { return INT64_MIN; }                        // objective_identity Costs.jl:23-24
static double max_identity(double) { return -INFINITY; }
// Int64 bounds are also reported as Float64 (the bisections search on doubles)
static void also_f64(const int64_t *lo, const int64_t *hi, double *lo_f64, double *hi_f64) { *lo_f64 = (double)*lo; *hi_f64 = (double)*hi; }
static void also_f64(const double *, const double *, double *, double *) {}

// cp_oracle_eval with the result in TC's slot of its (Int64, Float64) pair
template <typename TC>
static int32_t oracle_eval_into(cp_csr_t A, const cp_model_t *model, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp,
                                const int64_t *k, TC *out)
{
    const bool i64 = std::is_same<TC, int64_t>::value;
    return cp_oracle_eval(A, model, Pi, CP_HINT_STEP, nq, j, jp, k, i64 ? (int64_t *)out : nullptr, i64 ? nullptr : (double *)out);
}

// ------------------------------------------------------------------ the counters of cp_get_stat
// fix_trips: tasks the block merge walked in more than one trip; bits 0 / 1 / 2: a task of 1 / FIX_SERIAL / FIX_SERIAL + 1 tiles was
// merged; fix_items: the (task, trip) items the merges were handed (every attempt of a layer: a dropped round lists none).
// own_split_tiles: own tiles that streamed only their plane's variable link entries (layers that were not redone); gap_split_tiles: the
// same for the tiles of the gap rounds, which own_split_tiles does not count.  own_pair_waves / own_pair_lone: waves of k_lpass_own that
// ran two tiles / one because the run order ended ("own_pair"; layers that were not redone).  own_pack_tiles: split tiles, gap rounds
// included, that read the packed words ("own_pack"; layers that were not redone); own_pack_wide: 1 while the pattern of the last split
// launch has an in-block offset beyond 16 bits and runs on the wide arrays.  overlap_isect: column intersections cp_pack_overlap computed.
// bn_sym_layers: DP layers the valley search ran for the monotonized symmetric model.  cut_scan_layers: DP layers of the plaid edge-cut
// models the prefix-min scan ran (plaid_cut.hip).  env_valley_layers: DP layers the valley search ran for the envelope model
// (envelope.hip).  env_dc_layers: layers >= 2 of its total objective the divide and conquer ran (envelope_total.hip).  budget_layers:
// layers >= 2 of the total-cost DP under a work budget that dp_total_budget.hip ran.  blockcost_scan_packs: chunker calls that ran the
// window table over the quotient pattern and the (min,+) scan for a block model; blockcost_wave_evals: oracle queries of a block model
// that k_block_eval answered (blockcost.hip).  sym_total_layers: layers >= 2 of the total objective of a symmetric model that the divide
// and conquer of sym_total.hip ran.  plaid_total_layers / plaid_scan_layers: layers >= 2 of the total objective of the primary / secondary
// plaid connectivity model that the rectangle engine / the prefix-min scan of plaid_total.hip ran.  kept:cp_set_option("poison", 1) starts a
// poison pass by zeroing the other counters and leaves this one.
static const struct { const char *name; int64_t *var; bool kept; } g_stats[] = {
    {"spec_redo", &g_spec_redo, false}, {"poison_hits", &g_poison_hits, false}, {"fix_trips", &g_fix_trips, false},
    {"fix_edges", &g_fix_edges, false}, {"fix_items", &g_fix_items, false}, {"bn_sym_layers", &g_bn_sym_layers, true},
    {"own_split_tiles", &g_own_split_tiles, false}, {"gap_split_tiles", &g_gap_split_tiles, false},
    {"own_pair_waves", &g_own_pair_waves, false}, {"own_pair_lone", &g_own_pair_lone, false},
    {"own_pack_tiles", &g_own_pack_tiles, false}, {"own_pack_wide", &g_own_pack_wide, false},
    {"overlap_isect", &g_overlap_isect, false}, {"cut_scan_layers", &g_cut_scan_layers, false},
    {"cr_consume_rounds", &g_cr_consume_rounds, false}, {"cr_clear_launches", &g_cr_clear_launches, false},
    {"round_alloc_rounds", &g_round_alloc_rounds, false}, {"env_valley_layers", &g_env_valley_layers, false},
    {"env_dc_layers", &g_env_dc_layers, false}, {"budget_layers", &g_budget_layers, false},
    {"blockcost_scan_packs", &g_blockcost_scan_packs, false}, {"blockcost_wave_evals", &g_blockcost_wave_evals, false},
    {"sym_total_layers", &g_sym_total_layers, false},
    {"plaid_total_layers", &g_plaid_total_layers, false}, {"plaid_scan_layers", &g_plaid_scan_layers, false},
};
static void stats_reset(bool all) { for (const auto &c : g_stats) if (all || !c.kept) *c.var = 0; }

// ------------------------------------------------------------------ the options of cp_set_option (DESIGN 4e lists them with their rules)
enum OptRule { OPT_PLAIN, OPT_BOOL, OPT_CLAMP, OPT_POW2 };      // the value as given | value != 0 | clamped to [lo, hi] | lo doubled until >= value or == hi
constexpr int64_t NOLIM_LO = INT64_MIN, NOLIM_HI = INT64_MAX;
static const struct Opt { const char *name; int64_t *var; OptRule rule; int64_t lo, hi; } g_options[] = {
    {"force_brute", &g_opt_force_brute, OPT_PLAIN, 0, 0}, {"brute_max_n", &g_opt_brute_max_n, OPT_PLAIN, 0, 0}, {"dbg", &g_opt_dbg, OPT_PLAIN, 0, 0},
    {"short_t", &g_opt_short_t, OPT_PLAIN, 0, 0}, {"short_e", &g_opt_short_e, OPT_PLAIN, 0, 0}, {"ra_cache", &g_opt_ra_cache, OPT_PLAIN, 0, 0},
    {"leaf", &g_opt_leaf, OPT_PLAIN, 0, 0}, {"block_tables", &g_opt_block_tables, OPT_PLAIN, 0, 0}, {"nospec", &g_opt_nospec, OPT_PLAIN, 0, 0},
    {"rpass_small_tau", &g_opt_rpass_small_tau, OPT_PLAIN, 0, 0}, {"fixed_point", &g_opt_fixed_point, OPT_PLAIN, 0, 0},
    {"bn_wave", &g_opt_bn_wave, OPT_PLAIN, 0, 0},
    {"poison", &g_opt_poison, OPT_PLAIN, 0, 0},                 // (a nonzero value also zeroes the counters of a poison pass)
    {"pool", &g_opt_pool, OPT_BOOL, 0, 0},                      // (1: keep freed device blocks >= 1 MB for reuse; 0: return them, now and from here on)
    {"own_blk", &g_opt_own_blk, OPT_BOOL, 0, 0},                // (1, default: own tiles at 256-column blocks, run in block order; 0: tiles counted from each task head, in task order)
    {"own_split", &g_opt_own_split, OPT_BOOL, 0, 0},            // (1, default: own tiles of the planes >= 8 stream only the plane's variable link entries; 0: the whole columns)
    {"own_pair", &g_opt_own_pair, OPT_BOOL, 0, 0},              // (1, default: outside the gap rounds and the hyperedge costs a wave streams two own tiles; 0: one)
    {"own_pack", &g_opt_own_pack, OPT_BOOL, 0, 0},              // (1, default: split tiles read one packed word per step -- while own_split and own_blk are 1 and the pattern's offsets fit; 0: the wide arrays)
    {"round_alloc", &g_opt_round_alloc, OPT_BOOL, 0, 0},        // (1, default: task set-up reserves its lists' offsets with their slots and ends with the round's verdict; 0: the scan launch k_round_scans)
    {"cr_consume", &g_opt_cr_consume, OPT_BOOL, 0, 0},          // (1, default: full layers leave the right-pass counters zero as set-up reads them, no clearing launch per round; 0: the clear in front of every chunked right pass)
    {"gap_split", &g_opt_gap_split, OPT_BOOL, 0, 0},            // (1, default: so do the gap rounds' tiles of those planes -- while own_split is 1; 0: they stream the whole columns)
    {"lws", &g_opt_lws, OPT_BOOL, 0, 0},                        // (1, default: DynamicTotalChunker past the scan by chunk_lws.hip; 0: the one-wave kernel)
    {"budget_total", &g_opt_budget_total, OPT_BOOL, 0, 0},      // (1, default: total-cost DP under a pin / work budget by dp_total_budget.hip; 0: the one-wave kernel)
    {"blockcost_par", &g_opt_blockcost_par, OPT_BOOL, 0, 0},    // (1, default: BlockComponentCostModel by the quotient-pattern table + scan and the wave-per-query evaluation of blockcost.hip, inside blockcost_exact; 0: the one-wave step oracle)
    {"sym_total", &g_opt_sym_total, OPT_BOOL, 0, 0},            // (1, default: the total objective of a symmetric model inside sym_total_ok by sym_total.hip; 0: the candidate sweep)
    {"sym_total_batch", &g_opt_sym_total_batch, OPT_BOOL, 0, 0},      // (1, default: that path runs the rectangles of one depth of the column tree in one launch sequence; 0: one per rectangle)
    {"sym_total_min_n", &g_opt_sym_total_min_n, OPT_CLAMP, 0, NOLIM_HI},      // (the smallest n that path takes where the sweep is allowed; default 10240, the measured crossover.  Past brute_max_n: from 1024 on)
    {"sym_total_scan_cells", &g_opt_sym_total_scan_cells, OPT_CLAMP, 1, NOLIM_HI},      // (that path's limits, as budget_scan_cells / budget_scan_cols / budget_stair_cols;
    {"sym_total_scan_cols", &g_opt_sym_total_scan_cols, OPT_CLAMP, 1, NOLIM_HI},        //  defaults 2^20 / 1024 / 1024)
    {"sym_total_stair_cols", &g_opt_sym_total_stair_cols, OPT_CLAMP, 1, NOLIM_HI},
    {"plaid_total", &g_opt_plaid_total, OPT_BOOL, 0, 0},        // (1, default: the total objective of the plaid connectivity pair inside plaid_total_ok / plaid_scan_exact by plaid_total.hip; 0: the candidate sweep)
    {"plaid_total_min_n", &g_opt_plaid_total_min_n, OPT_CLAMP, 0, NOLIM_HI},      // (the smallest n the primary path takes where the sweep is allowed; default 1024, the first measured size, at which it already wins.  Past brute_max_n: from 1024 on)
    {"plaid_scan_min_n", &g_opt_plaid_scan_min_n, OPT_CLAMP, 0, NOLIM_HI},        // (the same for the secondary scan; default 1024.  Past brute_max_n: any n)
    {"plaid_total_scan_cells", &g_opt_plaid_total_scan_cells, OPT_CLAMP, 1, NOLIM_HI},      // (the primary path's limits, as sym_total_scan_cells / _scan_cols / _stair_cols;
    {"plaid_total_scan_cols", &g_opt_plaid_total_scan_cols, OPT_CLAMP, 1, NOLIM_HI},        //  defaults 2^20 / 1024 / 1024)
    {"plaid_total_stair_cols", &g_opt_plaid_total_stair_cols, OPT_CLAMP, 1, NOLIM_HI},
    {"budget_scan_cells", &g_opt_budget_scan_cells, OPT_CLAMP, 1, NOLIM_HI},      // (that path: a full rectangle of at most this many cells ...
    {"budget_scan_cols", &g_opt_budget_scan_cols, OPT_CLAMP, 1, NOLIM_HI},        //  ... and columns is scanned whole; default 2^20 / 1024)
    {"budget_stair_cols", &g_opt_budget_stair_cols, OPT_CLAMP, 1, NOLIM_HI},      // (the partial rows of a block below this many columns are scanned whole; default 1024)
    {"rcm_narrow", &g_opt_rcm_narrow, OPT_CLAMP, 0, NOLIM_HI},  // (cp_rcm: BFS levels of at most this many vertices go to the one-workgroup walker; 0: never; beyond its capacity: whenever the level fits)
    {"env_dc_min_n", &g_opt_env_dc_min_n, OPT_CLAMP, 0, NOLIM_HI},          // (AffineEnvelopeModel, total objective: the smallest n the divide and conquer of envelope_total.hip takes; below, the candidate sweep)
    {"greedy_lds_parts", &g_opt_greedy_lds_parts, OPT_CLAMP, 0, 2048},     // (cp_partition_greedy_bottleneck: the walk keeps the part costs and counts in LDS while K <= this; 0: always in global memory)
    {"gap_tau", &g_opt_gap_tau, OPT_CLAMP, NOLIM_LO, 20}, {"gap_min", &g_opt_gap_min, OPT_CLAMP, 8, NOLIM_HI}, {"gap_nr", &g_opt_gap_nr, OPT_CLAMP, 1, 2},
    {"force_max", &g_opt_force_max, OPT_CLAMP, 0, NOLIM_HI}, {"rpass_cap", &g_opt_rpass_cap, OPT_CLAMP, 1, NOLIM_HI},
    {"own_min", &g_opt_own_min, OPT_CLAMP, 64, NOLIM_HI}, {"bn_chunk", &g_opt_bn_chunk, OPT_CLAMP, 1, NOLIM_HI},
    {"bn_slack", &g_opt_bn_slack, OPT_CLAMP, 0, NOLIM_HI}, {"bn_run", &g_opt_bn_run, OPT_CLAMP, 2, NOLIM_HI},
    {"rpass_ch", &g_opt_rpass_ch, OPT_POW2, 16, 4096}, {"setup_bs", &g_opt_setup_bs, OPT_POW2, 64, 1024}, {"lws_leaf", &g_opt_lws_leaf, OPT_POW2, 256, 2048},
};
static int64_t opt_value(const Opt &o, int64_t value)
{
    switch (o.rule) {
    case OPT_BOOL: return value ? 1 : 0;
    case OPT_CLAMP: return value < o.lo ? o.lo : value > o.hi ? o.hi : value;
    case OPT_POW2: { int64_t v = o.lo; while (v < value && v < o.hi) v <<= 1; return v; }
    default: return value;
    }
}

}  // namespace cpk

// =================================================================== extern "C"
extern "C" {

const char *cp_last_error(void) { return g_last_error.c_str(); }
int32_t cp_version(void) { return 100; }

int32_t cp_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

static int32_t csr_create_impl(int64_t m, int64_t n, int64_t N, const int64_t *colptr, const int64_t *rowval,
                               int32_t device, bool on_device, cp_csr_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(out && colptr && (rowval || N == 0), CP_EINVAL, "null argument");
        CP_REQUIRE(m >= 0 && n >= 0 && N >= 0, CP_EINVAL, "negative dimension");
        CP_REQUIRE(n < (int64_t)1 << 30 && m < (int64_t)1 << 30 && N < ((int64_t)1 << 31) - 65536, CP_EINVAL,     // 32-bit entry positions; kernels look ahead by up to 16 Ki entries
                   "dimensions exceed the 32-bit link-array layout");
        CP_REQUIRE(cp_device_count() > 0, CP_EHIP, "no HIP device visible: libchainpart has no CPU fallback");
        CP_HIP(hipSetDevice(device));
        std::unique_ptr<cp_csr_s> A(new cp_csr_s());
        A->device = device; A->m = m; A->n = n; A->N = N;
        CP_HIP(hipStreamCreate(&A->stream));
        A->own_stream = true;
        csr_upload(A.get(), colptr, rowval, on_device);
        *out = A.release();
        return CP_OK;
    });
}

int32_t cp_csr_create(int64_t m, int64_t n, int64_t N, const int64_t *colptr, const int64_t *rowval, int32_t device, cp_csr_t *out)
{
    if (colptr && n >= 0 && (colptr[0] != 1 || colptr[n] != N + 1)) { set_error("colptr must be 1-based with colptr[n+1] == nnz+1"); return CP_EINVAL; }
    return csr_create_impl(m, n, N, colptr, rowval, device, false, out);
}

int32_t cp_csr_create_device(int64_t m, int64_t n, int64_t N, const int64_t *colptr_device, const int64_t *rowval_device,
                             int32_t device, cp_csr_t *out)
{
    return csr_create_impl(m, n, N, colptr_device, rowval_device, device, true, out);
}

int32_t cp_csr_destroy(cp_csr_t A)
{
    if (!A) return CP_OK;
    (void)hipSetDevice(A->device);
    if (A->stream) (void)hipStreamSynchronize(A->stream);
    delete A;                                        // (the destructor frees the DP scratch and the handle's own stream)
    return CP_OK;
}

int32_t cp_adjoint(cp_csr_t A, cp_csr_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out, CP_EINVAL, "null argument");
        CP_HIP(hipSetDevice(A->device));
        std::unique_ptr<cp_csr_s> T(new cp_csr_s());
        T->device = A->device;
        CP_HIP(hipStreamCreate(&T->stream));
        T->own_stream = true;
        csr_adjoint(A, T.get());
        *out = T.release();
        return CP_OK;
    });
}

int32_t cp_csr_download(cp_csr_t A, int64_t *dims_out, int64_t *colptr_out, int64_t *rowval_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A, CP_EINVAL, "null argument");
        if (dims_out) { dims_out[0] = A->m; dims_out[1] = A->n; dims_out[2] = A->N; }
        if (!colptr_out) return CP_OK;
        CP_REQUIRE(rowval_out || A->N == 0, CP_EINVAL, "rowval_out is null");
        CP_HIP(hipSetDevice(A->device));
        csr_download(A, colptr_out, rowval_out);
        return CP_OK;
    });
}

int32_t cp_csr_reset_cache(cp_csr_t A)
{
    if (!A) return CP_EINVAL;
    return guarded([&]() -> int32_t { CP_HIP(hipStreamSynchronize(A->stream)); drop_cache(A); return CP_OK; });
}

int32_t cp_set_stream(cp_csr_t A, void *hip_stream)
{
    if (!A) return CP_EINVAL;
    if (A->own_stream && A->stream) { (void)hipStreamSynchronize(A->stream); (void)hipStreamDestroy(A->stream); }
    A->stream = (hipStream_t)hip_stream;
    A->own_stream = false;
    return CP_OK;
}

int32_t cp_get_stat(const char *name, int64_t *out)
{
    if (!name || !out) return CP_EINVAL;
    for (const auto &c : g_stats) if (!strcmp(name, c.name)) { *out = *c.var; return CP_OK; }
    return CP_EINVAL;
}

int32_t cp_test_round_scans(const int32_t *a, int64_t na, int64_t na_max, const int32_t *b, int64_t nb, int64_t nb_max, int32_t two, int64_t cap_t,
                            int64_t cap_nt, int32_t err_in, int32_t reps, int64_t *offs_out, int64_t *toffs_out, int64_t *res)
{
    if (!offs_out || !toffs_out || !res || (na > 0 && !a) || (nb > 0 && !b)) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        dp_round_scans_test(a, na, na_max, b, nb, nb_max, two, cap_t, cap_nt, err_in, reps, offs_out, toffs_out, res);
        return CP_OK;
    });
}

int32_t cp_test_list_alloc(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int32_t bs, int64_t cap_t, int64_t cap_nt, int64_t o_cap,
                           int32_t err_in, int32_t reps, int64_t fit_ntask, int64_t fit_n, int64_t fit_own_min, int64_t *offs_out, int32_t *slot_a,
                           int64_t *toffs_out, int32_t *slot_b, int32_t *ioffs_out, int64_t *res)
{
    if (!offs_out || !toffs_out || !slot_a || !slot_b || !ioffs_out || !res || (na > 0 && !a) || (nb > 0 && !b)) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        dp_list_alloc_test(a, na, b, nb, bs, cap_t, cap_nt, o_cap, err_in, reps, fit_ntask, fit_n, fit_own_min, offs_out, slot_a, toffs_out, slot_b, ioffs_out, res);
        return CP_OK;
    });
}

int32_t cp_test_fix_merge(const cp_model_t *model, int64_t ntask, const int64_t *toffs, const int64_t *part_v, const int32_t *part_p, const int32_t *part_nn,
                          const int32_t *part_nl, const int32_t *tile_s, const int32_t *tile_s2, const int32_t *anchor, const int32_t *anchor2,
                          const int32_t *row, const int32_t *plane, int64_t n, int32_t reps, int32_t *p_out, int32_t *nn_out, int32_t *nl_out, int64_t *res)
{
    if (!model || !toffs || !part_v || !part_p || !part_nn || !tile_s || !anchor || !row || !plane || !p_out || !nn_out || !res) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        dp_fix_merge_test(model, ntask, toffs, part_v, part_p, part_nn, part_nl, tile_s, tile_s2, anchor, anchor2, row, plane, n, reps, p_out, nn_out, nl_out, res);
        return CP_OK;
    });
}

int32_t cp_test_own_pair(int64_t nt, int64_t wave, int64_t *res)
{
    if (!res) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        dp_own_pair_test(nt, wave, res);
        return CP_OK;
    });
}

int32_t cp_test_own_split(cp_csr_t A, int32_t *vpos_out, int32_t *vsa_out, int32_t *vnext_out, int64_t *res)
{
    if (!A || !vpos_out || !vsa_out || !vnext_out || !res) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        CP_HIP(hipSetDevice(A->device));
        dp_own_split_test(A, vpos_out, vsa_out, vnext_out, res);
        return CP_OK;
    });
}

int32_t cp_test_own_pack(cp_csr_t A, int32_t *vpk_out, int32_t *vbase_out, int64_t *res)
{
    if (!A || !vpk_out || !vbase_out || !res) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        CP_HIP(hipSetDevice(A->device));
        dp_own_pack_test(A, vpk_out, vbase_out, res);
        return CP_OK;
    });
}

int32_t cp_reset_stream(cp_csr_t A)
{
    if (!A) return CP_EINVAL;
    return guarded([&]() -> int32_t {
        if (A->stream || !A->own_stream) (void)hipStreamSynchronize(A->stream);      // (a borrowed stream may be the null stream)
        if (A->own_stream) return CP_OK;
        CP_HIP(hipSetDevice(A->device));
        hipStream_t s = nullptr;
        CP_HIP(hipStreamCreate(&s));
        A->stream = s; A->own_stream = true;
        return CP_OK;
    });
}

int32_t cp_set_option(const char *name, int64_t value)
{
    if (!name) return CP_EINVAL;
    if (!strcmp(name, "stat_reset")) { stats_reset(true); return CP_OK; }
    if (!strcmp(name, "prof_only")) { g_prof_only = (int)value; return CP_OK; }      // (the one option that is not an int64_t)
    for (const Opt &o : g_options) {
        if (strcmp(name, o.name)) continue;
        *o.var = opt_value(o, value);
        if (o.var == &g_opt_pool && !value) dev_pool_trim();
        if (o.var == &g_opt_poison && value) stats_reset(false);
        return CP_OK;
    }
    set_error("unknown option");
    return CP_EINVAL;
}

int32_t cp_prof_enable(int32_t on) { g_prof_on = on != 0; return CP_OK; }
int32_t cp_prof_reset(void)
{
    for (auto &p : g_prof) { p.launches = 0; p.ms = 0; p.alg_bytes = 0; }
    return CP_OK;
}
int32_t cp_prof_get(int32_t slot, const char **name, int64_t *launches, double *total_ms, double *alg_bytes)
{
    if (slot >= 0 && slot < PROF_NSLOTS) {
        if (name) *name = g_prof[slot].name;
        if (launches) *launches = g_prof[slot].launches;
        if (total_ms) *total_ms = g_prof[slot].ms;
        if (alg_bytes) *alg_bytes = g_prof[slot].alg_bytes;
    }
    return PROF_NSLOTS;
}

int32_t cp_partition_equi(int64_t n, int64_t K, int64_t *spl_out)
{
    if (K < 1 || n < 0 || !spl_out) return CP_EINVAL;
    for (int64_t k = 0; k <= K; k++) spl_out[k] = k * (n / K) + ((n % K) < k ? (n % K) : k) + 1;   // EquiPartitioner.jl:7
    return CP_OK;
}

int32_t cp_pack_equi(int64_t n, int64_t w, int64_t *spl_out, int64_t *K_out)
{
    if (w < 1 || n < 0 || !spl_out || !K_out) return CP_EINVAL;
    int64_t K = 0;
    for (int64_t j = 1; j <= n; j += w) spl_out[K++] = j;                                           // EquiPartitioner.jl:20
    spl_out[K] = n + 1;
    *K_out = K;
    return CP_OK;
}

int32_t cp_partition_dynamic(cp_csr_t A, int64_t K, int32_t combine, int32_t order, const cp_model_t *model,
                             const cp_rowpart_t *Pi, const cp_model_t *weight, int64_t wmax_i64, double wmax_f64, int64_t *spl_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl_out && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        CP_REQUIRE(combine == CP_COMBINE_SUM || combine == CP_COMBINE_MAX, CP_EINVAL, "bad combine");
        CP_HIP(hipSetDevice(A->device));
        bool constrained = weight && weight->kind != CP_MODEL_FEASIBLE;
        if (model->kind == CP_MODEL_PRIMARY || model->kind == CP_MODEL_SECONDARY) {
            CP_REQUIRE(!constrained, CP_EUNSUPPORTED, "ConstrainedCost over a plaid connectivity model has no device path");
            return with_cost_type(model->dtype, [&](auto tag) { return run_plaid_dynamic<decltype(tag)>(A, K, combine, order, model, Pi, spl_out); });
        }
        if (model_is_cut(model->kind)) {                                        // plaid_cut.hip: the prefix-min scan or the candidate sweep
            CP_REQUIRE(!constrained, CP_EUNSUPPORTED, "ConstrainedCost over a plaid edge-cut model has no device path");
            return with_cost_type(model->dtype, [&](auto tag) {
                using TC = decltype(tag);
                return run_cut_dynamic<TC>(A, K, combine, order, model, Pi, spl_out, nullptr, (TC *)nullptr);
            });
        }
        // the envelope cost: the valley search or the candidate sweep of envelope.hip through the K-layer driver; splitter order only
        // (the chunker loop calls the oracle with two arguments, for which the reference has no method), no constrained form
        CP_REQUIRE(!(constrained && model_is_env(weight->kind)), CP_EUNSUPPORTED, "AffineEnvelopeModel has no device path as the weight of a ConstrainedCost");
        if (model_is_env(model->kind)) {
            CP_REQUIRE(!constrained, CP_EUNSUPPORTED, "ConstrainedCost over an AffineEnvelopeModel has no device path");
            CP_REQUIRE(order == CP_ORDER_SPLITTER, CP_EUNSUPPORTED,
                       "AffineEnvelopeModel: the chunker loop order calls ocl(j, j'), for which the envelope oracle has no method; splitter order only");
            return run_dynamic(A, K, combine, order, model, spl_out);
        }
        // the symmetric family: the O(n^2) sweep over the wavelet counters (dp_driver.hip); no constrained form
        CP_REQUIRE(!(constrained && model_is_sym(model->kind)), CP_EUNSUPPORTED, "ConstrainedCost over a symmetric cost model has no device path");
        if (constrained) {
            CP_REQUIRE(weight->kind == CP_MODEL_VERTEX_COUNT || (weight->kind == CP_MODEL_WORK && !weight->alpha_k), CP_EINVAL,
                       "weight must be VertexCount or an AffineWorkModel");
            const ConstrainedRoute route = constrained_route(A, K, combine, model, weight, wmax_i64, wmax_f64);
            if (route.kind != ConstrainedRoute::OneWave)                        // the scalable paths of dp_driver.hip
                return run_dynamic_windowed(A, K, combine, order, model, route, weight, wmax_i64, wmax_f64, spl_out);
            return with_cost_type(model->dtype, [&](auto tag) {
                return run_dyn_constrained<decltype(tag)>(A, K, combine, order, model, Pi, weight, wmax_i64, wmax_f64, spl_out);
            });
        }
        CP_REQUIRE(dp_takes_kind(model->kind, DP_KINDS_STRIPE), CP_EUNSUPPORTED, "model kind has no device DP path yet");
        return run_dynamic(A, K, combine, order, model, spl_out);
    });
}

int32_t cp_dynamic_tables(cp_csr_t A, int64_t K, int32_t combine, const cp_model_t *model, const cp_rowpart_t *Pi,
                          int64_t *ptr_out, int64_t *cst_i64, double *cst_f64)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && ptr_out && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        CP_REQUIRE(combine == CP_COMBINE_SUM || combine == CP_COMBINE_MAX, CP_EINVAL, "bad combine");
        if (model_is_cut(model->kind) || model->kind == CP_MODEL_PRIMARY || model->kind == CP_MODEL_SECONDARY) {      // (the only kinds here that look at Pi)
            CP_HIP(hipSetDevice(A->device));
            std::vector<int64_t> spl((size_t)K + 1);
            const bool cut = model_is_cut(model->kind);
            return with_cost_type(model->dtype, [&](auto tag) {
                using TC = decltype(tag);
                if (cut) return run_cut_dynamic<TC>(A, K, combine, CP_ORDER_SPLITTER, model, Pi, spl.data(), ptr_out, pick<TC>(cst_i64, cst_f64));
                return run_plaid_dynamic<TC>(A, K, combine, CP_ORDER_SPLITTER, model, Pi, spl.data(), ptr_out, pick<TC>(cst_i64, cst_f64));
            });
        }
        CP_REQUIRE(dp_takes_kind(model->kind, DP_KINDS_TABLES), CP_EUNSUPPORTED, "model kind has no device DP path");
        CP_HIP(hipSetDevice(A->device));
        std::vector<int64_t> spl((size_t)K + 1);
        DpTables tabs;
        tabs.ptr_tab = ptr_out; tabs.cst_i64 = cst_i64; tabs.cst_f64 = cst_f64;
        return run_dynamic(A, K, combine, CP_ORDER_SPLITTER, model, spl.data(), tabs);
    });
}

int32_t cp_dynamic_tables_constrained_combine(cp_csr_t A, int64_t K, int32_t combine, const cp_model_t *model, const cp_model_t *weight,
                                              int64_t wmax_i64, double wmax_f64, int64_t *win_lo, int64_t *win_hi, int64_t *ptr_out,
                                              int64_t *cst_i64, double *cst_f64)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && ptr_out && win_lo && win_hi && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        CP_REQUIRE(combine == CP_COMBINE_SUM || combine == CP_COMBINE_MAX, CP_EINVAL, "bad combine");
        CP_REFUSE_ENV(model, "the constrained DP");
        CP_REFUSE_ENV(weight, "the constrained DP (as the weight)");
        CP_REQUIRE(!weight || weight->kind == CP_MODEL_VERTEX_COUNT || (weight->kind == CP_MODEL_WORK && !weight->alpha_k), CP_EINVAL,
                   "weight must be VertexCount or an AffineWorkModel");
        const ConstrainedRoute route = constrained_route(A, K, combine, model, weight, wmax_i64, wmax_f64);      // (null weight: the width wmax_i64)
        CP_REQUIRE(route.kind != ConstrainedRoute::OneWave, CP_EUNSUPPORTED, "outside the windowed scalable path");
        CP_HIP(hipSetDevice(A->device));
        std::vector<int64_t> spl((size_t)K + 1);
        DpTables tabs;
        tabs.ptr_tab = ptr_out; tabs.cst_i64 = cst_i64; tabs.cst_f64 = cst_f64; tabs.win_lo = win_lo; tabs.win_hi = win_hi;
        return run_dynamic_windowed(A, K, combine, CP_ORDER_SPLITTER, model, route, weight, wmax_i64, wmax_f64, spl.data(), tabs);
    });
}

int32_t cp_dynamic_tables_constrained(cp_csr_t A, int64_t K, const cp_model_t *model, int64_t wmax, int64_t *win_lo, int64_t *win_hi,
                                      int64_t *ptr_out, int64_t *cst_i64, double *cst_f64)
{
    return cp_dynamic_tables_constrained_combine(A, K, CP_COMBINE_SUM, model, nullptr, wmax, (double)wmax, win_lo, win_hi, ptr_out, cst_i64, cst_f64);
}

int32_t cp_oracle_eval(cp_csr_t A, const cp_model_t *model, const cp_rowpart_t *Pi, int32_t hint, int64_t nq,
                       const int64_t *j, const int64_t *jp, const int64_t *k, int64_t *out_i64, double *out_f64)
{
    (void)hint;
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model_known(model) && (nq == 0 || (j && jp)), CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(A->device));
        return with_cost_type(model->dtype, [&](auto tag) {
            using TC = decltype(tag);
            TC *out = pick<TC>(out_i64, out_f64);
            if (model->kind == CP_MODEL_PRIMARY || model->kind == CP_MODEL_SECONDARY) return run_plaid_eval<TC>(A, model, Pi, nq, j, jp, k, out);
            // the block model: one wave per query over the quotient pattern (blockcost.hip) where that route applies, else the
            // stateful step oracle, evaluated in query order by one wave (seq.hip)
            if (model->kind == CP_MODEL_BLOCK)
                return run_block_eval<TC>(A, model, Pi, nq, j, jp, out) ? CP_OK : run_seq_eval<TC>(A, model, Pi, nq, j, jp, k, out);
            if (model_is_cut(model->kind)) return run_cut_eval<TC>(A, model, Pi, nq, j, jp, k, out);
            if (model_is_sym(model->kind)) return run_sym_eval<TC>(A, model, nq, j, jp, k, out);
            if (model_is_env(model->kind)) return run_env_eval<TC>(A, model, nq, j, jp, k, out);      // (Pi accepted and ignored: Costs.jl:5-7)
            return run_oracle_eval<TC>(A, model, nq, j, jp, k, out);
        });
    });
}

int32_t cp_oracle_step(cp_csr_t A, const cp_model_t *model, const cp_rowpart_t *Pi, int64_t nq, const int32_t *move_j, const int64_t *j,
                       const int32_t *move_jp, const int64_t *jp, const int64_t *k, int64_t *out_i64, double *out_f64)
{
    if (nq > 0 && (!move_j || !move_jp || !j || !jp)) { set_error("null argument"); return CP_EINVAL; }
    for (int64_t t = 0; t < nq; t++) {
        for (int side = 0; side < 2; side++) {
            const int32_t mv = side ? move_jp[t] : move_j[t];
            const int64_t *x = side ? jp : j;
            if (mv < CP_MOVE_SAME || mv > CP_MOVE_JUMP) { set_error("Step: unknown move code"); return CP_EINVAL; }
            if (t == 0 || mv == CP_MOVE_JUMP) continue;
            const int64_t want = mv == CP_MOVE_SAME ? x[t - 1] : mv == CP_MOVE_NEXT ? x[t - 1] + 1 : x[t - 1] - 1;
            if (x[t] != want) { set_error("Step: a Same / Next / Prev move does not match the previous position"); return CP_EINVAL; }
        }
    }
    return cp_oracle_eval(A, model, Pi, CP_HINT_STEP, nq, j, jp, k, out_i64, out_f64);
}

int32_t cp_objective(cp_csr_t A, int64_t K, const int64_t *spl, const cp_model_t *model, const cp_rowpart_t *Pi,
                     int32_t combine, int64_t *out_i64, double *out_f64)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        if (model->kind == CP_MODEL_SECONDARY) {
            // SecondaryConnectivityCosts.jl:103-108: the primary objective of the adjoint with the two partitions swapped
            CP_REQUIRE(Pi && Pi->spl && Pi->K == K, CP_EINVAL, "the secondary objective needs a SplitPartition Pi with K parts");
            cp_csr_t T = nullptr;
            int32_t rc = cp_adjoint(A, &T);
            if (rc != CP_OK) return rc;
            cp_model_t pm = *model; pm.kind = CP_MODEL_PRIMARY;
            cp_rowpart_t rp; rp.K = K; rp.asg = nullptr; rp.spl = spl;
            rc = cp_objective(T, K, Pi->spl, &pm, &rp, combine, out_i64, out_f64);
            cp_csr_destroy(T);
            return rc;
        }
        std::vector<int64_t> j((size_t)K), jp((size_t)K), kk((size_t)K);
        for (int64_t k = 0; k < K; k++) { j[k] = spl[k]; jp[k] = spl[k + 1]; kk[k] = k + 1; }
        return with_cost_type(model->dtype, [&](auto tag) -> int32_t {
            using TC = decltype(tag);
            std::vector<TC> v((size_t)K);
            int32_t rc = oracle_eval_into<TC>(A, model, Pi, K, j.data(), jp.data(), kk.data(), v.data());
            if (rc != CP_OK) return rc;
            TC acc = combine == CP_COMBINE_SUM ? (TC)0 : max_identity(tag);             // (Int64 sums wrap: cadd)
            for (int64_t k = 0; k < K; k++) acc = combine == CP_COMBINE_SUM ? cadd(acc, v[k]) : (acc > v[k] ? acc : v[k]);
            *pick<TC>(out_i64, out_f64) = acc;
            return CP_OK;
        });
    });
}

int32_t cp_bound_stripe(cp_csr_t A, int64_t K, const cp_model_t *model, int64_t *lo_i64, int64_t *hi_i64, double *lo_f64, double *hi_f64)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        return with_cost_type(model->dtype, [&](auto tag) -> int32_t {
            using TC = decltype(tag);
            const int64_t n = A->n, N = A->N;
            auto P = [&](int i) { return model_param<TC>(model, i); };
            TC *lo = pick<TC>(lo_i64, lo_f64), *hi = pick<TC>(hi_i64, hi_f64);
            if (model->kind == CP_MODEL_WORK) {                                        // WorkCosts.jl:39-51
                const TC a = P(0), bv = P(1), bp = P(2);
                *lo = a + fld(bv * (TC)n + bp * (TC)N, K);
                if (bv >= 0 && bp >= 0) *hi = a + bv * (TC)n + bp * (TC)N;
                else if (bv <= 0 && bp <= 0) *hi = a;
                else { set_error("bound_stripe: mixed-sign work model"); return CP_EINVAL; }
                also_f64(lo, hi, lo_f64, hi_f64);
                return CP_OK;
            }
            if (model->kind == CP_MODEL_PRIMARY) {                                     // PrimaryConnectivityCosts.jl:43-51
                CP_REQUIRE(!(P(1) < 0 || P(2) < 0 || P(3) < 0 || P(4) < 0), CP_EINVAL, "bound_stripe asserts beta >= 0");
                cp_model_t c = *model; c.kind = CP_MODEL_CONNECTIVITY; c.alpha_k = nullptr; c.n_alpha_k = 0;
                TC *cp = pick<TC>(c.p_i64, c.p_f64);
                int64_t di, dh; double df, dg;
                cp[CP_P_NET] = std::max(P(3), P(4)); cp[4] = 0;
                int32_t rc = cp_bound_stripe(A, K, &c, &di, hi_i64, &df, hi_f64);
                if (rc != CP_OK) return rc;
                cp[CP_P_NET] = std::min(P(3), P(4));
                return cp_bound_stripe(A, K, &c, lo_i64, &dh, lo_f64, &dg);
            }
            if (model->kind == CP_MODEL_PRIMARY_EDGE_CUT) {                            // PrimaryEdgeCutCosts.jl:28-39
                int32_t rc = cut_bound_stripe<TC>(A, K, nullptr, model, false, lo, hi);
                if (rc == CP_OK) also_f64(lo, hi, lo_f64, hi_f64);
                return rc;
            }
            if (model_is_env(model->kind)) {                                           // EnvelopeCosts.jl:43-53
                int32_t rc = env_bound_stripe<TC>(A, K, model, lo, hi);
                if (rc == CP_OK) also_f64(lo, hi, lo_f64, hi_f64);
                return rc;
            }
            const bool mono = model->kind == CP_MODEL_MONO_SYM_CONNECTIVITY;
            if (mono) {                                                                // MonotonizedSymmetricConnectivityCosts.jl:50-66
                CP_REQUIRE(A->m == A->n, CP_EINVAL, "bound_stripe asserts m == n");
                CP_REQUIRE(P(1) >= 0 && P(2) >= 0 && P(3) >= 0, CP_EINVAL, "bound_stripe asserts beta >= 0");      // (a NaN fails it too)
            }
            if ((model->kind == CP_MODEL_CONNECTIVITY || mono) && model->alpha_k && model->n_alpha_k > 0) {
                // per-part alpha = the reference tests' FunkyConnectivityModel / FunkyMonotonizedSymmetricConnectivityModel; its
                // bound_stripe (test_Partitioners.jl:36-41) is
                // (minimum, maximum) of (minimum(alpha), maximum(alpha), maximum_k ocl(1, n+1, k))
                CP_REQUIRE(model->n_alpha_k >= K, CP_EINVAL, "bound_stripe: fewer per-part alphas than parts");
                std::vector<int64_t> one((size_t)K, 1), np1((size_t)K, n + 1), ks((size_t)K);
                for (int64_t k = 0; k < K; k++) ks[(size_t)k] = k + 1;
                std::vector<TC> v((size_t)K);
                int32_t rc = oracle_eval_into<TC>(A, model, nullptr, K, one.data(), np1.data(), ks.data(), v.data());
                if (rc != CP_OK) return rc;
                const TC *al = (const TC *)model->alpha_k;
                TC amin = al[0], amax = al[0], fmax = v[0];
                for (int64_t k = 1; k < K; k++) { amin = std::min(amin, al[k]); amax = std::max(amax, al[k]); fmax = std::max(fmax, v[(size_t)k]); }
                *lo = std::min(amin, std::min(amax, fmax)); *hi = std::max(amin, std::max(amax, fmax));
                also_f64(lo, hi, lo_f64, hi_f64);
                return CP_OK;
            }
            if (model->kind == CP_MODEL_CONNECTIVITY || mono) {
                TC chi = 0;
                if (mono) {
                    // the model form: c_hi = alpha + b_vertex*n + b_over_pin*sum(max(deg - Delta_pins, 0)) + b_dia_net*m, left to right
                    SymHost H;
                    CP_HIP(hipSetDevice(A->device));
                    sym_prepare(A, model, H, false);
                    chi = cadd(cadd(cadd(P(0), cmulc(n, P(CP_P_VERTEX))), cmulc(H.over_total, P(CP_P_OVER_PIN))), cmulc(A->m, P(CP_P_DIA_NET)));
                } else {                                                               // ConnectivityCosts.jl:25-35
                    CP_REQUIRE(P(1) >= 0 && P(2) >= 0 && P(3) >= 0, CP_EINVAL, "bound_stripe asserts beta >= 0");
                    int64_t one = 1, np1 = n + 1;
                    int32_t rc = oracle_eval_into<TC>(A, model, nullptr, 1, &one, &np1, nullptr, &chi);
                    if (rc != CP_OK) return rc;
                }
                *hi = chi; *lo = P(0) + fld(chi - P(0), K);
                also_f64(lo, hi, lo_f64, hi_f64);
                return CP_OK;
            }
            set_error("bound_stripe has no method for this model (the reference raises MethodError)");
            return CP_EUNSUPPORTED;
        });
    });
}

// bound_stripe(A, K, Pi, mdl): Costs.jl:17-19 drops Pi for every model but the secondary one
// (SecondaryConnectivityCosts.jl:21-31 == :42-61: per part of Pi, c_lo = max work cost, c_hi = max work cost + nets * b_remote)
int32_t cp_bound_stripe_pi(cp_csr_t A, int64_t K, const cp_rowpart_t *Pi, const cp_model_t *model, int64_t *lo_i64, int64_t *hi_i64,
                           double *lo_f64, double *hi_f64)
{
    if (model && model->kind == CP_MODEL_SECONDARY_EDGE_CUT)                           // the model form, SecondaryEdgeCutCosts.jl:20-28
        return guarded([&]() -> int32_t {
            CP_REQUIRE(A && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
            return with_cost_type(model->dtype, [&](auto tag) -> int32_t {
                using TC = decltype(tag);
                TC *lo = pick<TC>(lo_i64, lo_f64), *hi = pick<TC>(hi_i64, hi_f64);
                int32_t rc = cut_bound_stripe<TC>(A, K, Pi, model, false, lo, hi);
                if (rc == CP_OK) also_f64(lo, hi, lo_f64, hi_f64);
                return rc;
            });
        });
    if (!model || model->kind != CP_MODEL_SECONDARY) return cp_bound_stripe(A, K, model, lo_i64, hi_i64, lo_f64, hi_f64);
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model_known(model) && K >= 1 && Pi && Pi->spl, CP_EINVAL, "bad argument");
        return with_cost_type(model->dtype, [&](auto tag) -> int32_t {
            using TC = decltype(tag);
            auto P = [&](int i) { return model_param<TC>(model, i); };
            CP_REQUIRE(!(P(1) < 0 || P(2) < 0 || P(3) < 0 || P(4) < 0), CP_EINVAL, "bound_stripe asserts beta >= 0");
            // the two bounds are the secondary cost with all nets local resp. all nets remote: evaluate the oracle on the empty and the
            // full column range of every part with (b_local, b_remote) = (0, 0) resp. (b_remote, b_remote)
            int64_t Kp = Pi->K;
            std::vector<int64_t> one((size_t)Kp, 1), ks((size_t)Kp);
            for (int64_t k = 0; k < Kp; k++) ks[(size_t)k] = k + 1;
            cp_model_t lo_m = *model, hi_m = *model;
            TC *pl = pick<TC>(lo_m.p_i64, lo_m.p_f64), *ph = pick<TC>(hi_m.p_i64, hi_m.p_f64);
            pl[3] = 0; pl[4] = 0; ph[3] = P(4);
            lo_m.alpha_k = nullptr; lo_m.n_alpha_k = 0; hi_m.alpha_k = nullptr; hi_m.n_alpha_k = 0;
            std::vector<TC> a((size_t)Kp), b((size_t)Kp);
            int32_t rc = oracle_eval_into<TC>(A, &lo_m, Pi, Kp, one.data(), one.data(), ks.data(), a.data());
            if (rc != CP_OK) return rc;
            rc = oracle_eval_into<TC>(A, &hi_m, Pi, Kp, one.data(), one.data(), ks.data(), b.data());
            if (rc != CP_OK) return rc;
            TC *lo = pick<TC>(lo_i64, lo_f64), *hi = pick<TC>(hi_i64, hi_f64);
            *lo = 0; *hi = 0;                                              // "c_lo = 0; c_hi = 0" (:44-45)
            for (int64_t k = 0; k < Kp; k++) { *lo = std::max(*lo, a[(size_t)k]); *hi = std::max(*hi, b[(size_t)k]); }
            also_f64(lo, hi, lo_f64, hi_f64);
            return CP_OK;
        });
    });
}

int32_t cp_link_array(cp_csr_t A, int64_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(A->device));
        ensure_links(A);
        std::vector<int32_t> h((size_t)(A->N > 0 ? A->N : 1));
        CP_HIP(hipMemcpyAsync(h.data(), A->prev.p, sizeof(int32_t) * (size_t)A->N, hipMemcpyDeviceToHost, A->stream));
        CP_HIP(hipStreamSynchronize(A->stream));
        for (int64_t q = 0; q < A->N; q++) out[q] = (A->n + 1) - ((int64_t)h[q] + 1);   // idx'[q] = (n+1) - hst[i]
        return CP_OK;
    });
}

// ---- row-tiled DP across ranks (multi-GPU): see include/chainpart.h; the handle and its layers: dp.hpp, dp_driver.hip
int32_t cp_dp_begin(cp_csr_t A, int64_t K, int32_t combine, int32_t order, const cp_model_t *model, int64_t row_lo, int64_t row_hi,
                    cp_dp_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out && model_known(model) && K >= 1, CP_EINVAL, "bad argument");
        CP_REQUIRE(row_lo >= 1 && row_hi >= row_lo && row_hi <= A->n + 2, CP_EINVAL, "row tile must satisfy 1 <= row_lo <= row_hi <= n+2");
        CP_REFUSE_ENV(model, "the row-tiled DP");
        CP_REQUIRE(dp_takes_kind(model->kind, DP_KINDS_TILED), CP_EUNSUPPORTED, "model kind has no device DP path");
        CP_HIP(hipSetDevice(A->device));
        return dp_begin(A, K, combine, order, model, row_lo, row_hi, out);
    });
}

int32_t cp_dp_layer(cp_dp_t dp, int64_t k, const void *cst_prev_device, void *cst_cur_device)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(dp && cst_cur_device && k >= 1, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(dp->A->device));
        return dp->step_layer(k, cst_prev_device, cst_cur_device);
    });
}

int32_t cp_dp_ptr_at(cp_dp_t dp, int64_t k, int64_t jp, int64_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(dp && out && k >= 1 && jp >= 1 && jp <= dp->A->n + 1, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(dp->A->device));
        CP_REQUIRE(k <= dp->K, CP_EINVAL, "bad layer");
        *out = 0;
        if (k == 1) { *out = 1; return CP_OK; }                 // ptr[:, 1] == 1 on every rank
        int64_t r = jp - 1;
        if (r < dp->lay_lo[(size_t)k] || r > dp->lay_hi[(size_t)k]) return CP_OK;      // another rank owns this row
        int32_t v = 0;
        CP_HIP(hipMemcpyAsync(&v, dp->ptr.p + (size_t)(k - 1) * (size_t)(dp->A->n + 1) + (size_t)r, sizeof(int32_t), hipMemcpyDeviceToHost, dp->A->stream));
        CP_HIP(hipStreamSynchronize(dp->A->stream));
        *out = (int64_t)v + 1;
        return CP_OK;
    });
}

int32_t cp_dp_set_rows(cp_dp_t dp, int64_t row_lo, int64_t row_hi)
{
    if (!dp || row_lo < 1 || row_hi < row_lo || row_hi > dp->A->n + 2) return CP_EINVAL;
    dp->rlo = row_lo - 1; dp->rhi = row_hi - 2;
    return CP_OK;
}

int32_t cp_dp_set_window(cp_dp_t dp, int64_t wmax)
{
    if (!dp || wmax < 0) return CP_EINVAL;
    dp->wwin = wmax;
    return CP_OK;
}

int32_t cp_dp_ptr_row(cp_dp_t dp, int64_t k, int64_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(dp && out && k >= 1, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(dp->A->device));
        CP_REQUIRE(k <= dp->K, CP_EINVAL, "bad layer");
        const int64_t n = dp->A->n, rlo = dp->lay_lo[(size_t)k], rhi = dp->lay_hi[(size_t)k];
        if (k == 1) { for (int64_t r = 0; r <= n; r++) out[r] = 1; return CP_OK; }
        std::vector<int32_t> h((size_t)n + 1);
        CP_HIP(hipMemcpyAsync(h.data(), dp->ptr.p + (size_t)(k - 1) * (size_t)(n + 1), sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, dp->A->stream));
        CP_HIP(hipStreamSynchronize(dp->A->stream));
        for (int64_t r = 0; r <= n; r++) out[r] = (r < rlo || r > rhi) ? 0 : (int64_t)h[(size_t)r] + 1;
        return CP_OK;
    });
}

int32_t cp_dp_block_tables(cp_dp_t dp, int32_t *nplanes_out, int64_t *opt_out, int64_t *nets_out, int64_t *selfnets_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(dp && opt_out && nets_out, CP_EINVAL, "bad argument");
        CP_HIP(hipSetDevice(dp->A->device));
        return dp->block_tables(nplanes_out, opt_out, nets_out, selfnets_out);
    });
}

int32_t cp_dp_destroy(cp_dp_t dp)
{
    if (!dp) return CP_OK;
    (void)hipSetDevice(dp->A->device);
    delete dp;
    return CP_OK;
}

}  // extern "C"
