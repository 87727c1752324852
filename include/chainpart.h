/*
 * chainpart.h -- C ABI of libchainpart.so, the MI355X (gfx950) engine for the contiguous
 * partitioning hot path of ChainPartitioners.jl.
 *
 * The reference has no FFI layer (it is pure Julia; the boundary is multiple dispatch).
 * These are the entry points a `ccall` shim binds to replace the reference methods named
 * beside each declaration (paths under /root/reference/src).  INTEGRATION.md shows the shim.
 *
 * Conventions
 *   - plain pointers and sizes only; all index VALUES 1-based exactly as Julia stores them;
 *     arrays are caller-owned host memory unless the name says _device;
 *   - every function returns a CP_* status (chainpart_types.h); cp_last_error() gives text;
 *   - calls are synchronous (return after the stream is idle); handles are opaque,
 *     single-owner, not thread-safe, freed by the matching *_destroy;
 *   - there is NO CPU fallback: without a HIP device every compute entry returns CP_EHIP.
 */
#ifndef CHAINPART_H
#define CHAINPART_H

#include "chainpart_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cp_csr_s *cp_csr_t;        /* device-resident sparsity pattern + link arrays */
typedef struct cp_count_s *cp_count_t;    /* device-resident counting structure */

const char *cp_last_error(void);
int32_t cp_version(void);
/* number of visible HIP devices (0 if none); does not initialise a context */
int32_t cp_device_count(void);

/* ---- residency of A.colptr / A.rowval in HBM (SparseMatrixCSC fields; the reference reads
 * them in every oracle constructor, e.g. SparseColorArrays.jl:101-118) ---- */
int32_t cp_csr_create(int64_t m, int64_t n, int64_t N, const int64_t *colptr, const int64_t *rowval,
                      int32_t device, cp_csr_t *out);
/* same, but colptr/rowval already live in device memory (1-based int64, as Julia would upload them) */
int32_t cp_csr_create_device(int64_t m, int64_t n, int64_t N, const int64_t *colptr_device,
                             const int64_t *rowval_device, int32_t device, cp_csr_t *out);
int32_t cp_csr_destroy(cp_csr_t csr);
/* adjointpattern(A) (util.jl:67-95): the transposed pattern (n x m, rows of every column ascending) as a NEW
 * device-resident handle -- the counting sort the reference runs is the (row, column) order the link-array build
 * already produces.  First block of SURVEY 8(f)-4 (the 2-D callers partition A and its adjoint alternately). */
int32_t cp_adjoint(cp_csr_t csr, cp_csr_t *out);
/* copy a handle's pattern back to the host in Julia's layout: colptr int64[n+1], rowval int64[nnz], 1-based;
 * dims_out = {m, n, nnz} (call with NULL arrays to query the sizes first) */
int32_t cp_csr_download(cp_csr_t csr, int64_t *dims_out, int64_t *colptr_out, int64_t *rowval_out);
/* drop cached derived structures (link arrays, counters) so the next call rebuilds them:
 * lets a benchmark time "one partition_stripe call including oracle construction" */
int32_t cp_csr_reset_cache(cp_csr_t csr);
/* permute_plaid(A, CuthillMcKeePermuter(reverse, assumesymmetry, checksymmetry); adj_A)  CuthillMcKeePermuter.jl:7-265: the exact
 * queue of the reference's symrcm / rctrcm, built on the device level by level (csrc/rcm.hip).  mode 0: the symmetric walk if the
 * pattern is square and equal to its adjoint, else the bipartite walk over the m + n rows and columns; 1: the symmetric walk without
 * the test (assumesymmetry; m != n is CP_EINVAL -- the reference would read out of bounds); 2: the bipartite walk.  adj: a handle of
 * the adjoint if the caller holds one (shape checked, CP_EINVAL), else NULL.  rowprm_out (m) / colprm_out (n): perm(sigma), perm(tau),
 * 1-based; on the symmetric walk both receive the same vector.  reverse != 0: each reversed.  The bipartite walk keeps 32-bit ids:
 * m + n or 2 nnz at 2^31 or beyond is CP_EUNSUPPORTED.  A pattern whose columns hold an index twice is refused with CP_EINVAL when
 * the queue would overflow.  stats_out: NULL or 6 values {1 symmetric / 2 bipartite walk, trees, levels expanded, of them by grid
 * kernels, launches of the one-workgroup walker, readbacks}; see the option "rcm_narrow". */
int32_t cp_rcm(cp_csr_t csr, cp_csr_t adj_or_null, int32_t mode, int32_t reverse, int64_t *rowprm_out /* m */, int64_t *colprm_out /* n */,
               int64_t *stats_out /* 6 or NULL */);
/* A[rowprm, colprm] (PermutingPartitioner.jl:12, :21): out[i', j'] = A[rowprm[i'], colprm[j']] as a NEW device-resident handle, the
 * rows of every column ascending.  rowprm (m) / colprm (n): 1-based host arrays, NULL for the identity; each is checked on the device
 * to be a permutation (CP_EINVAL, nothing is read out of range). */
int32_t cp_csr_permute(cp_csr_t csr, const int64_t *rowprm /* m or NULL */, const int64_t *colprm /* n or NULL */, cp_csr_t *out);
/* The quotient pattern of A under a SplitPartition Pi of its rows: the rows of every part merged, Pi->K x n, one entry (k, c) per part k
 * with a nonzero in column c, as a NEW device-resident handle (the parts of every column ascending).  The 2-D block cost is a weighted
 * net count on it (BlockCosts.jl:19-152; csrc/blockcost.hip).  Pi->spl must run from 1 to m + 1 (CP_EINVAL; a Map- or DomainPartition,
 * spl == NULL, too); a repeated boundary is an empty part, an empty row of the result. */
int32_t cp_csr_quotient(cp_csr_t csr, const cp_rowpart_t *Pi, cp_csr_t *out);

/* ---- counting structures ----
 * dominancecount(hint, A)   SparsePrefixMatrices.jl:438-458   kind CP_COUNT_DOM : C[i,j]
 * netcount(hint, A)         SparseColorArrays.jl:57-58,101-125 kind CP_COUNT_NET : net[j,j']
 * selfnetcount(hint, A)     SparseColorArrays.jl:165-229       kind CP_COUNT_SELFNET
 * One exact device structure (wavelet bit-vectors) serves every hint: query results are
 * integers independent of the structure. */
#define CP_COUNT_DOM     0
#define CP_COUNT_NET     1
#define CP_COUNT_SELFNET 2
/* dianetcount(hint, A)      SparseColorArrays.jl:65-99   kind CP_COUNT_DIANET  : nets of A[:, j:j'-1] with the diagonal added
 * selfpincount(hint, A)     SparseColorArrays.jl:268-318 kind CP_COUNT_SELFPIN : nnz(A[j:j'-1, j:j'-1])
 * both need a square pattern (CP_EINVAL otherwise); dianet refuses nnz + n >= 2^31 - 1 with CP_EUNSUPPORTED */
#define CP_COUNT_DIANET  3
#define CP_COUNT_SELFPIN 4
int32_t cp_count_build(cp_csr_t csr, int32_t kind, int32_t hint, cp_count_t *out);
int32_t cp_count_query(cp_count_t h, int64_t nq, const int64_t *a, const int64_t *b, int64_t *out);
int32_t cp_count_destroy(cp_count_t h);
/* the NetCount link array idx'[q] = (n+1) - hst[i] (SparseColorArrays.jl:106-113), for tests */
int32_t cp_link_array(cp_csr_t csr, int64_t *out /* N */);

/* ---- rowenvelope(A)  EnvelopeMatrices.jl:10-57 ----
 * env[j, j'] = (least first row, greatest last row) of the columns j : j'-1, (m + 1, 0) for a range without entries.  The handle is
 * a cp_count_t of kind CP_COUNT_ENVELOPE over the reference's implicit tree, H = cllog2(n), built on the device level by level and kept
 * in the matrix handle's cache (cp_csr_reset_cache drops it; the next call rebuilds it).  n == 0 is CP_EINVAL (cllog2(0)).  The matrix
 * handle must outlive it.  cp_envelope_query walks the tree bottom-up as getindex does, 1 <= j <= j' <= n + 1.  cp_envelope_tree copies the
 * nodes out in the reference's order.  cp_count_query refuses the kind; cp_count_destroy frees it as cp_envelope_destroy does. */
#define CP_COUNT_ENVELOPE 5
int32_t cp_envelope_build(cp_csr_t csr, cp_count_t *out);
int32_t cp_envelope_query(cp_count_t h, int64_t nq, const int64_t *j, const int64_t *jp, int64_t *lo_out, int64_t *hi_out);
int32_t cp_envelope_tree(cp_count_t h, int64_t *dims_out /* 3: H, m, n */,
                         int64_t *tree_out /* 2*(2^(H+1)-1): (lo, hi) pairs in the reference's node order; NULL: dims only */);
int32_t cp_envelope_destroy(cp_count_t h);

/* ---- weighted dominance (used by no cost oracle of the path, kept for the reference's AbstractMatrix API) ----
 * dominancesum(hint, A)                 SparsePrefixMatrices.jl:1-250   S[i, j] = sum(A[1:i-1, 1:j-1])  (test_SparsePrefixMatrices.jl:15)
 * rookcount!(hint, N, idx) / rooksum!(hint, N, idx, val)  :825-1273   the same over ONE point (idx[j], j) per column
 * val: nnz (rook: N) 8-byte weights in the pattern's entry order -- CP_I64: Int / UInt words, summed with wrap-around exactly as
 * Julia does; CP_F64: Float64 (a prefix-sum structure like the reference's `scn`: equal up to rounding, not bit for bit).
 * One query returns the count (rows < i among the entries of the columns < j) and the weighted sum. */
typedef struct cp_wsum_s *cp_wsum_t;
int32_t cp_domsum_build(cp_csr_t csr, int32_t dtype, const void *val, cp_wsum_t *out);
int32_t cp_rook_build(int64_t N, const int64_t *idx, int32_t dtype, const void *val /* NULL: counts only */, int32_t device, cp_wsum_t *out);
int32_t cp_wsum_query(cp_wsum_t h, int64_t nq, const int64_t *i, const int64_t *j, int64_t *count_out /* may be NULL */,
                      int64_t *sum_i64, double *sum_f64);
int32_t cp_wsum_destroy(cp_wsum_t h);

/* partwise(A, Pi) PartwiseCounts.jl:1-60 */
int32_t cp_partwise(cp_csr_t csr, int64_t K, const int64_t *asg, int64_t *nprime_out,
                    int64_t *pios_out /* K+1 */, int64_t *prm_out /* <= N */,
                    int64_t *pos_out /* <= N+1 */, int64_t *idx_out /* N */);

/* ---- cost oracles ----
 * ocl(j, j', k...) for a batch  (WorkCosts.jl:30-35, ConnectivityCosts.jl:58-64,
 * HyperedgeCutCosts.jl:44-51, BlockCosts.jl:66-142); k may be NULL */
int32_t cp_oracle_eval(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi, int32_t hint,
                       int64_t nq, const int64_t *j, const int64_t *jp, const int64_t *k,
                       int64_t *out_i64, double *out_f64);
/* Step(ocl)(move_j(j), move_j'(j'), Same(k)) along a walk of nq calls (Costs.jl:174-195; the specialised methods
 * ConnectivityCosts.jl:66-76, HyperedgeCutCosts.jl:53-64, SparseColorArrays.jl:127-152, 231-256): move codes CP_MOVE_*.
 * A move is the caller's promise about the previous call's position (Same: equal, Next: +1, Prev: -1, Jump: anything); the
 * reference's stepwise structures rely on it, the device counters are random-access and do not -- so the promise is CHECKED
 * (CP_EINVAL on a broken one; the first call may carry any move) and the value is ocl(j, j', k), which is what every Step
 * method of the reference returns (Costs.jl:195). */
int32_t cp_oracle_step(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi, int64_t nq,
                       const int32_t *move_j, const int64_t *j, const int32_t *move_jp, const int64_t *jp,
                       const int64_t *k, int64_t *out_i64, double *out_f64);
/* bound_stripe(A, K, mdl)  WorkCosts.jl:37-51, ConnectivityCosts.jl:22-35 */
int32_t cp_bound_stripe(cp_csr_t csr, int64_t K, const cp_model_t *model,
                        int64_t *lo_i64, int64_t *hi_i64, double *lo_f64, double *hi_f64);
/* bound_stripe(A, K, Pi, mdl) (Costs.jl:17-19): Pi only matters to CP_MODEL_SECONDARY (SecondaryConnectivityCosts.jl:21-31) */
int32_t cp_bound_stripe_pi(cp_csr_t csr, int64_t K, const cp_rowpart_t *Pi, const cp_model_t *model,
                           int64_t *lo_i64, int64_t *hi_i64, double *lo_f64, double *hi_f64);
/* total_value / bottleneck_value  Costs.jl:26-66 */
int32_t cp_objective(cp_csr_t csr, int64_t K, const int64_t *spl, const cp_model_t *model,
                     const cp_rowpart_t *Pi, int32_t combine, int64_t *out_i64, double *out_f64);

/* ---- partitioners ---- */
/* partition_stripe(A, K, Dynamic{Total,Bottleneck}{Splitter,Chunker}(f | ConstrainedCost(f,w,w_max)), [Pi])
 * DynamicSplitter.jl:15-50 (order SPLITTER), :52-87 (order CHUNKER), :206-314 (constrained);
 * Reference{Total,Bottleneck}Splitter (ReferenceSplitter.jl:1-13) are the same entry.  A model whose totals can round (Float64
 * above 2^53) or wrap (Int64 at 2^60 and beyond) has no fast path: above the brute_max_n option it is CP_EUNSUPPORTED, never a guess.
 * Constrained, total cost: width weights (VertexCount, AffineWorkModel(alpha, c, 0)) take the windowed O(K n log^2 n) path; any other
 * AffineWorkModel weight with b_v, b_p >= 0 and no per-part alpha (pins per part, work per part) the two-staircase divide and conquer
 * of csrc/dp_total_budget.hip -- Work / Connectivity / HyperedgeCut models of the inverse-Monge class with exact totals, either
 * element type, both loop orders, any n (option "budget_total"); everything else the one-wave literal kernel. */
int32_t cp_partition_dynamic(cp_csr_t csr, int64_t K, int32_t combine, int32_t order,
                             const cp_model_t *model, const cp_rowpart_t *Pi,
                             const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                             int64_t *spl_out /* K+1 */);
/* pack_stripe(A, DynamicTotalChunker(f | ConstrainedCost(f,w,w_max)), [Pi])  DynamicChunker.jl:15-75 */
int32_t cp_pack_dynamic(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi,
                        const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                        int64_t *spl_out /* n+1 */, int64_t *K_out);
/* the tables DynamicChunker.jl:20-56 builds before unravel_chunks!: cst[j'] and spl[j'] (the smallest minimising j) at index j' - 1,
 * spl_tab[0] = 0, from whichever path cp_pack_dynamic takes.  cst_i64 / cst_f64 (n+1): the one of the model's element type. */
int32_t cp_pack_dynamic_tables(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi,
                               const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                               int64_t *spl_tab /* n+1 */, int64_t *cst_i64 /* n+1 */, double *cst_f64 /* n+1 */);
/* partition_stripe(A, K, [Flip]BisectCostBottleneckSplitter(f, eps))  BisectCostBottleneckSplitter.jl:6-127 */
int32_t cp_partition_bisect_cost(cp_csr_t csr, int64_t K, const cp_model_t *model, double eps,
                                 int32_t flip, int64_t *spl_out /* K+1 */);
/* B independent BisectCostBottleneckSplitter partitions of ONE pattern in one launch (BisectCostBottleneckSplitter.jl:6-63 per request
 * b: K[b], models[b] (Work or Connectivity, one element type for the batch), eps[b], flip[b] (NULL: 0)): the probe chain of a single
 * partition is sequential and fills one wave; a sweep over K / eps / model constants fills the chip and shares the counting
 * structure.  Row b of spl_out (ld >= max K + 1 entries per row) holds the K[b] + 1 split indices of request b -- exactly what
 * cp_partition_bisect_cost returns for it. */
int32_t cp_partition_bisect_cost_batch(cp_csr_t csr, int64_t B, const int64_t *K, const cp_model_t *models, const double *eps,
                                       const int32_t *flip, int64_t ld, int64_t *spl_out);
/* the same two with the row partition the plaid cost models need: partition_stripe(A, K, method, Pi)
 * (CP_MODEL_PRIMARY / CP_MODEL_SECONDARY; Pi is ignored by every other model, Costs.jl:5-7) */
int32_t cp_partition_bisect_cost_pi(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                    int32_t flip, int64_t *spl_out /* K+1 */);
int32_t cp_partition_bisect_index_pi(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, int32_t flip,
                                     int64_t *spl_out /* K+1 */);
/* pack_stripe(A, ConcaveTotalChunker(f | ConstrainedCost(f,w,w_max)), [Pi]) ConcaveTotalChunker.jl:9-24, chunk_concave! :57-114;
 * partition_stripe(A, K, ConcaveTotalSplitter(..), [Pi]) :26-55 and the ConstrainedCost method :140-180.
 * The candidate-deque algorithm is exact for concave (Monge) costs, e.g. CP_MODEL_POWER_WORK with gamma >= 1. */
int32_t cp_pack_concave(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi,
                        const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                        int64_t *spl_out /* n+1 */, int64_t *K_out);
int32_t cp_partition_concave(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi,
                             const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                             int64_t *spl_out /* K+1 */);
/* partition_stripe(A, K, [Flip]BisectIndexBottleneckSplitter(f))  BisectIndexBottleneckSplitter.jl:5-83, :85-166
 * (exact bottleneck: bisection over the split index of every part in turn) */
int32_t cp_partition_bisect_index(cp_csr_t csr, int64_t K, const cp_model_t *model, int32_t flip,
                                  int64_t *spl_out /* K+1 */);
/* partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractConnectivityModel, eps))
 * LazyBisectCostBottleneckSplitter.jl:140-258 (forward-scan probes over the link array).
 * Models that are not connectivity models return CP_EINVAL (the reference's generic method asserts, :486-501). */
int32_t cp_partition_lazy_bisect_cost(cp_csr_t csr, int64_t K, const cp_model_t *model, double eps,
                                      int64_t *spl_out /* K+1 */);
/* ... and with f an AffineMonotonizedSymmetricConnectivityModel (CP_MODEL_MONO_SYM_CONNECTIVITY, :260-388): the same probe over
 * the pattern with its diagonal added.  This form also reports the number of probes the bisection ran (nprobes_out may be NULL). */
int32_t cp_partition_lazy_bisect_cost_probes(cp_csr_t csr, int64_t K, const cp_model_t *model, double eps,
                                             int64_t *spl_out /* K+1 */, int64_t *nprobes_out);
/* partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractPrimaryConnectivityModel, eps), Pi)
 * LazyBisectCostBottleneckSplitter.jl:390-483: with CP_MODEL_PRIMARY the probe counts the local and remote nets of the open part
 * from the link array and the owner of every entry's row, and a column that closes a part is recounted for the part it opens.
 * Pi (asg or spl; any partition of the rows) is required and Pi->K <= K; CP_EINVAL otherwise, and for a negative beta (the bound
 * asserts).  The bounds are the model form's (Pi dropped, Costs.jl:17-19), with per-part alpha those of test_Partitioners.jl:43-48.
 * Every other model kind: cp_partition_lazy_bisect_cost_probes, Pi is not looked at.  nprobes_out (one value) may be NULL. */
int32_t cp_partition_lazy_bisect_cost_pi(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                         int64_t *spl_out /* K+1 */, int64_t *nprobes_out);
/* partition_stripe(A, K, LazyFlipBisectCostBottleneckSplitter(f, eps), [Pi])  LazyBisectCostBottleneckSplitter.jl:72-138, for
 * decreasing costs: a probe closes a part behind the first column that makes its cost small enough; the whole bisection is one
 * launch that streams the link array (csrc/lazy_flip.hip).  Model kinds:
 *   CP_MODEL_CONNECTIVITY, CP_MODEL_COLBLOCK (per-part alpha included)        Pi is not looked at
 *   CP_MODEL_PRIMARY      Pi (asg or spl) required, Pi->K <= K                 CP_EINVAL otherwise
 *   CP_MODEL_SECONDARY    Pi->spl required, Pi->K == K                         CP_EINVAL otherwise
 * every other kind: CP_EUNSUPPORTED, naming it.  The bounds are those of cp_partition_bisect_cost_pi (a negative beta of a model
 * without per-part alpha: CP_EINVAL, the bound asserts); a primary model with per-part alpha takes those of
 * test_Partitioners.jl:43-48.  nnz >= 2^31 - 16384: CP_EUNSUPPORTED.  nprobes_out (one value) may be NULL. */
int32_t cp_partition_lazy_flip_bisect_cost(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                           int64_t *spl_out /* K+1 */, int64_t *nprobes_out);
/* pack_stripe(A, ConvexTotalChunker(..), [Pi]) / partition_stripe(A, K, ConvexTotalSplitter(..), [Pi])
 * ConvexTotalChunker.jl:9-265 */
int32_t cp_pack_convex(cp_csr_t csr, const cp_model_t *model, const cp_rowpart_t *Pi,
                       const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                       int64_t *spl_out /* n+1 */, int64_t *K_out);
/* B independent pack_stripe(A, ConvexTotalChunker(ConstrainedCost(models[b], VertexCount(), wmax[b]))) calls on ONE pattern in one
 * launch (ConvexTotalChunker.jl:141-168, 211-265 per request): the stack algorithm is a dependent chain that occupies one wave
 * whatever the size of the matrix; a sweep over the cost constants / width limits occupies one wave per request, and the requests
 * share the net counter and the window table of net counts.  Requests: ColumnBlock / Connectivity / Work models (one element type,
 * no per-part alpha), 1 <= wmax[b] <= 15.  Row b of spl_out (ld entries per row; n + 1 always suffices) holds the K_out[b] + 1 chunk
 * boundaries of request b -- exactly what cp_pack_convex returns for it. */
int32_t cp_pack_convex_batch(cp_csr_t csr, int64_t B, const cp_model_t *models, const int64_t *wmax, int64_t ld, int64_t *spl_out, int64_t *K_out);
int32_t cp_partition_convex(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi,
                            const cp_model_t *weight, int64_t wmax_i64, double wmax_f64,
                            int64_t *spl_out /* K+1 */);
/* pack_stripe(A, StrictChunker(w_max))  StrictChunker.jl:5-54: a part holds copies of its first column, at most w_max of them
 * (w_max < 1: no width limit -- the reference's `w != w_max` never fires).  Computed as a column-against-left-neighbour comparison, a
 * max-scan and a compaction instead of the reference's sweep; the split vector is the sweep's.  n < 1 is CP_EINVAL (the reference
 * reads colptr[2]).  spl_out: n+1 slots, K_out[0] + 1 of them hold the split vector (the rest are unspecified); K_out: one element. */
int32_t cp_pack_strict(cp_csr_t csr, int64_t w_max, int64_t *spl_out /* n+1 */, int64_t *K_out);
/* pack_stripe(A, OverlapChunker(rho, w_max); n_nets)  OverlapChunker.jl:6-75: column j' joins the part that starts at column j unless
 * j' - j == w_max or Float64(|col j' and col j|) < rho * Float64(min(c, |col j'|)), evaluated in Float64 as written (:57), where c is
 * the length of the matrix's FIRST column throughout -- the reference never refreshes it at a split (:58-63) and its output depends on
 * that.  Computed as next[j] for every start j at once and the orbit of column 1 by pointer doubling; the split vector is the sweep's.
 * n_nets_out: NULL, or n slots of which the first K_out[0] receive the number of distinct rows of each part (n_nets[], :59, :67).
 * n < 1 is CP_EINVAL.  The work is sum_j (next[j] - j) column intersections, at most n * w_max; without a width limit a run of L
 * mutually overlapping columns costs about L^2 / 2 (cp_get_stat "overlap_isect" counts them). */
int32_t cp_pack_overlap(cp_csr_t csr, double rho, int64_t w_max, int64_t *spl_out /* n+1 */, int64_t *K_out, int64_t *n_nets_out /* n or NULL */);
/* partition_stripe(A, K, MagneticPartitioner(), Pi)  MagneticPartitioner.jl:3-20: column j with d entries takes the part of the row
 * of its entry number u_j mod d (0-based), a column without entries the part 1 + u_j mod K.  The reference draws u_j from Julia's
 * global RNG; here draws (n values, each >= 0) are an input, or NULL: u_j = draw(seed, 1, j), the SplitMix64 counter hash of
 * csrc/map_part.hip shifted right by one bit.  Pi (asg, m entries, or spl): any partition of the rows, required; its values are
 * checked on the device to lie in 1 .. Pi->K and the draws to be non-negative (CP_EINVAL, nothing is read out of range).
 * asg_out: the n entries of MapPartition(K, asg). */
int32_t cp_partition_magnetic(cp_csr_t csr, int64_t K, const cp_rowpart_t *Pi, int64_t seed, const int64_t *draws /* n or NULL */,
                              int64_t *asg_out /* n */);
/* partition_stripe(A, K, GreedyBottleneckPartitioner(mdl), Pi)  MagneticPartitioner.jl:26-177 (both methods: they compute the same
 * numbers), mdl a CP_MODEL_SECONDARY model of either element type, per-part alpha included; any other kind is CP_EUNSUPPORTED.
 * The columns are visited in `order` (a permutation of 1 .. n standing for the reference's randperm(n)), or with NULL in ascending
 * (draw(seed, 2, j), j).  A column takes the part of largest current cost among the parts of its rows -- the first such entry in
 * column order -- and part 1 if it has no entries; the chosen part gains a local net, loses a remote one and its cost is recomputed
 * from its four counts.  The counts of the parts come from A's own columns: no adjoint is needed.  Preconditions, all checked on the
 * device before the walk (CP_EINVAL, nothing is read out of range): Pi->K == K, every Pi value in 1 .. K, order a permutation.
 * asg_out: n entries; order_out: NULL or n entries, the order that was walked; cst_i64 / cst_f64 (K, either may be NULL): the final
 * part costs in the one of the model's element type.  The walk is one wave; see the option "greedy_lds_parts". */
int32_t cp_partition_greedy_bottleneck(cp_csr_t csr, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, int64_t seed,
                                       const int64_t *order /* n or NULL */, int64_t *asg_out /* n */, int64_t *order_out /* n or NULL */,
                                       int64_t *cst_i64 /* K */, double *cst_f64 /* K */);
/* EquiSplitter / EquiChunker  EquiPartitioner.jl:3-22 (closed forms, host arithmetic) */
int32_t cp_partition_equi(int64_t n, int64_t K, int64_t *spl_out /* K+1 */);
int32_t cp_pack_equi(int64_t n, int64_t w, int64_t *spl_out /* cld(n,w)+1 */, int64_t *K_out);

/* full (n+1) x K tables of the splitter-order DP, column-major like the reference's cst/ptr
 * (DynamicSplitter.jl:23-24), for table-level parity tests.  Layer K holds row n+1 only.  Pi is read by the four plaid kinds (8 / 9 and
 * 13 / 14), on whichever of their paths runs. */
int32_t cp_dynamic_tables(cp_csr_t csr, int64_t K, int32_t combine, const cp_model_t *model,
                          const cp_rowpart_t *Pi, int64_t *ptr_out, int64_t *cst_i64, double *cst_f64);

/* the same window on the ConstrainedCost splitter with the width weight (DynamicSplitter.jl:206-258,
 * DynamicTotalSplitter(ConstrainedCost(f, VertexCount(), w_max))): win_lo / win_hi receive j'_lo[k] / j'_hi[k] of
 * column_constraints (:144-172), the tables are written densely ((n+1) x K column-major; a cell outside its window holds what
 * the reference's WindowConstrainedMatrix returns for it, 0 / typemax, :127-134).  Infeasible windows: CP_INFEASIBLE.
 * Only the models the O(K n log^2 n) path takes (else CP_EUNSUPPORTED). */
int32_t cp_dynamic_tables_constrained(cp_csr_t csr, int64_t K, const cp_model_t *model, int64_t wmax,
                                      int64_t *win_lo /* K */, int64_t *win_hi /* K */,
                                      int64_t *ptr_out, int64_t *cst_i64, double *cst_f64);
/* ... with the combine op and the weight given (NULL: VertexCount).  CP_COMBINE_MAX is DynamicBottleneckSplitter(ConstrainedCost(f,
 * w, w_max)) (DynamicSplitter.jl:206-258 with g = max) on the valley search with candidate limits: Int64 cost models; width
 * weights (VertexCount, AffineWorkModel(alpha, c, 0)) or any AffineWorkModel weight with b_v, b_p >= 0 (pins per part).
 * CP_COMBINE_SUM takes width weights (the windowed path) and, through csrc/dp_total_budget.hip, any AffineWorkModel weight with
 * b_v, b_p >= 0 and no per-part alpha under the gate named at cp_partition_dynamic, cost models of either element type.  w_max in
 * the weight's element type, as in cp_partition_dynamic. */
int32_t cp_dynamic_tables_constrained_combine(cp_csr_t csr, int64_t K, int32_t combine, const cp_model_t *model, const cp_model_t *weight,
                                              int64_t wmax_i64, double wmax_f64, int64_t *win_lo /* K */, int64_t *win_hi /* K */,
                                              int64_t *ptr_out, int64_t *cst_i64, double *cst_f64);

/* ---- row-tiled DP: one process per GPU, the layer's cost vector is completed by the caller's collective ----
 * The rows j' of every DP layer (DynamicSplitter.jl:33-46: all cst[j',k] of a layer depend only on layer k-1) are
 * tiled contiguously over the ranks.  Rank g calls cp_dp_begin with its tile [row_lo, row_hi) (1-based, half-open,
 * tiles cover 1..n+1), then for k = 1..K: cp_dp_layer(dp, k, prev, cur) -- layer 1 is computed in full by every rank;
 * for k >= 2 it fills cur[row_lo-1 .. row_hi-2] from the COMPLETE previous layer `prev` -- followed by an all_gather of
 * the tile slices (torch.distributed / RCCL over xGMI) so that `cur` is complete everywhere.  cst buffers are
 * caller-owned device arrays of n+1 cost elements (int64 or double like the model).  unravel_splits
 * (DynamicSplitter.jl:89-99) asks the owner of each row: cp_dp_ptr_at returns ptr[j',k] (1-based) on the owning rank
 * and 0 elsewhere, so a MAX all_reduce of one integer per layer walks the chain. */
typedef struct cp_dp_s *cp_dp_t;
int32_t cp_dp_begin(cp_csr_t csr, int64_t K, int32_t combine, int32_t order, const cp_model_t *model,
                    int64_t row_lo, int64_t row_hi, cp_dp_t *out);
int32_t cp_dp_layer(cp_dp_t dp, int64_t k, const void *cst_prev_device, void *cst_cur_device);
int32_t cp_dp_ptr_at(cp_dp_t dp, int64_t k, int64_t jp, int64_t *out);
/* table-level windows for parity tests: the whole ptr[:, k] row of this rank's tile (0 outside the tile), and -- on the
 * O(n log^2 n) path -- the per-block state the last cp_dp_layer(k >= 2) left behind: for bit plane b < nplanes and row
 * j' = r + 1 with bit b of r set, opt_out[b*(n+1) + r] = the LARGEST j minimising cst_prev[j] + f(j, j', k) over the
 * row's Fenwick block j - 1 in [r_b - 2^b, r_b) (r_b = r with the bits below b cleared), nets_out / selfnets_out the counts
 * of that part; 0 where bit b is clear.  These are the candidates the layer's final combine merges into
 * cst[j', k] / ptr[j', k] (DynamicSplitter.jl:36-43); arrays hold 31 * (n+1) entries (selfnets_out may be NULL). */
int32_t cp_dp_ptr_row(cp_dp_t dp, int64_t k, int64_t *out /* n+1 */);
/* layers k >= 2 computed after this call take their candidates from the width window j' - w_max <= j <= j' (the candidate
 * range of the ConstrainedCost splitter with a VertexCount weight, DynamicSplitter.jl:233-246); 0 restores the full range.
 * The layer windows j'_lo / j'_hi are the caller's business (the row tile, and a huge cost outside the previous window). */
int32_t cp_dp_set_window(cp_dp_t dp, int64_t wmax);
/* moves this rank's row tile [row_lo, row_hi) for the layers computed from now on (the constrained DP tiles every layer's own
 * window j'_lo[k] .. j'_hi[k] over the ranks); cp_dp_ptr_at / cp_dp_ptr_row answer with the tile each layer was computed with */
int32_t cp_dp_set_rows(cp_dp_t dp, int64_t row_lo, int64_t row_hi);
int32_t cp_dp_block_tables(cp_dp_t dp, int32_t *nplanes_out, int64_t *opt_out, int64_t *nets_out, int64_t *selfnets_out);
int32_t cp_dp_destroy(cp_dp_t dp);

/* ---- execution control / measurement ---- */
/* run subsequent launches of this csr on an existing hipStream_t (e.g. torch's current stream) */
int32_t cp_set_stream(cp_csr_t csr, void *hip_stream);
/* back to a stream of the handle's own (waits for the borrowed one first): a handle must not stay bound to a caller's stream
 * that may be destroyed before the handle is (chainpartitioners.jl_amd/distributed.py restores it when the tiled run returns) */
int32_t cp_reset_stream(cp_csr_t csr);
/* diagnostics counters of the library (tests): "spec_redo" -- DP layers enqueued from the previous layer's counts that had to be
 * run again with exact counts; "poison_hits" -- with cp_set_option("poison", 1): plane cells read that the layer had not written
 * (each such layer must be one of the redone ones; the library checks it and fails with CP_EINTERNAL otherwise).  Both are reset
 * when "poison" is switched on.  "fix_trips" -- own-tiled DP tasks whose block merge took more than one trip; "fix_edges" -- bits
 * 0 / 1 / 2: a task of 1 / 16 / 17 tiles was merged (both sides of the lane / block split); both count the layers that stand, not
 * attempts that were redone.  "fix_items" -- the (task, trip) work items those merges were handed: one per 2 048 tiles, or part of
 * them, of every task of more than 16 tiles, in every attempt of a layer (a round dropped by its verdict lists none) and in
 * cp_test_fix_merge.  "own_split_tiles" -- own tiles that streamed only their plane's variable link entries ("own_split"), in
 * the layers that stand.  "own_pair_waves" / "own_pair_lone" -- waves of the own-tile stream that ran two tiles / one because the run
 * order ended ("own_pair"), in the layers that stand.  "own_pack_tiles" -- split tiles, those of the gap rounds included, that read the packed words
 * ("own_pack"), in the layers that stand; "own_pack_wide" -- 1 while the pattern of the last layer with split tiles has an in-block
 * offset beyond 16 bits and runs on the wide arrays.  "overlap_isect" -- the column intersections cp_pack_overlap computed.
 * "round_alloc_rounds" -- DP rounds whose task set-up reserved the lists' offsets itself ("round_alloc"), in every attempt of a layer;
 * "cr_consume_rounds" / "cr_clear_launches" -- right passes that add a row's counts chunk by chunk and ran without / with the clearing
 * launch in front ("cr_consume").  "env_valley_layers" -- DP layers of the envelope model (kind 15) the valley search ran; the
 * candidate sweep counts none.  "env_dc_layers" -- its DP layers >= 2 under the total objective that the divide and conquer over the
 * cut column ran (a layer of one row counts).  "budget_layers" -- DP layers >= 2 of the total objective under a pin or work budget that
 * csrc/dp_total_budget.hip ran (its profile slot is "dp_budget").  "sym_total_layers" -- DP layers >= 2 of the total objective of a
 * symmetric model (kinds 10 - 12) that the divide and conquer of csrc/sym_total.hip ran (its profile slot is "dp_sym_total"; a layer of
 * one row counts).  "plaid_total_layers" / "plaid_scan_layers" -- DP layers >= 2 of the total objective of the primary / secondary plaid
 * connectivity model (kinds 8 / 9) that the rectangle engine / the prefix-min scan of csrc/plaid_total.hip ran (profile slot
 * "dp_plaid_total" for both; the candidate sweep keeps "dp_brute" and counts none).  All of these are reset when "poison" is switched on and by cp_set_option("stat_reset", 1); reading
 * changes nothing. */
int32_t cp_get_stat(const char *name, int64_t *out);
/* Test entry: the launch that ends the counting phase of a DP round, on host arrays.  Exclusive scans of a[0 .. na) and (two != 0)
 * b[0 .. nb) in ONE launch whose grid is sized for na_max >= na / nb_max >= nb elements while the counts are read on the device;
 * then the round's verdict: totals beyond cap_t / cap_nt, or err_in != 0, drop the round.  reps >= 1 launches in a row on one
 * workspace.  offs_out: na + 1 values (the last: the total), toffs_out: nb + 1; res: {T, NT, nlong, nown, ntile = ceil(T / 256), err}
 * as the round's later kernels read them -- after a dropped round {0, 0, 0, 0, 0, 1}. */
int32_t cp_test_round_scans(const int32_t *a, int64_t na, int64_t na_max, const int32_t *b, int64_t nb, int64_t nb_max, int32_t two,
                            int64_t cap_t, int64_t cap_nt, int32_t err_in, int32_t reps, int64_t *offs_out, int64_t *toffs_out, int64_t *res);
/* Test entry: the allocation that replaces those scans with "round_alloc" 1, on host arrays.  Lane i of blocks of bs lanes (a
 * multiple of 64 up to 1024; one block more appends nothing) appends a[i] units to the first list (i < na) and b[i] tiles to the
 * second (i < nb); every block reserves its slots and its range of units with one atomic per list, and the last block to finish
 * closes the lists and gives the verdict of cp_test_round_scans (o_cap <= nb: slots of the second list; a count beyond it drops
 * the round too).  reps launches in a row on one record.  offs_out: na + 1 offsets by slot (the last: the total), slot_a[i]: the
 * slot of lane i; toffs_out (nb + 1), slot_b likewise; ioffs_out[slot]: the first merge item of the slot's task (ceil(tiles / 2048)
 * items for every task of more than 16 tiles).  res: {T, NT, nlong, nown, ntile, err, items, the ticket, the two packed words
 * or-ed (both 0 between launches), 1 if a round of fit_ntask tasks on fit_n columns with "own_min" fit_own_min may take this path}. */
int32_t cp_test_list_alloc(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int32_t bs, int64_t cap_t, int64_t cap_nt, int64_t o_cap,
                           int32_t err_in, int32_t reps, int64_t fit_ntask, int64_t fit_n, int64_t fit_own_min, int64_t *offs_out, int32_t *slot_a,
                           int64_t *toffs_out, int32_t *slot_b, int32_t *ioffs_out, int64_t *res);
/* Test entry: the launch that merges the tile partials of a DP round's own-tiled tasks, on host arrays.  Task t of ntask owns the
 * tiles toffs[t] .. toffs[t + 1) (toffs[0] == 0, at least one tile each); tile k has the partial winner {part_v[k]: the 8 bytes of
 * its cost in the model's element type, part_p[k]: its column, < 0 for a tile without a candidate, part_nn[k], part_nl[k]: its
 * counts inside the tile} and made tile_s[k] / tile_s2[k] counts; anchor[t] / anchor2[t] were made before the task's first tile.
 * The counts before a tile are added to its winner through the model (Work, Connectivity or HyperedgeCut; the second-count arrays
 * are read for HyperedgeCut only and may be NULL otherwise), the smallest cost wins, among equals the largest column.  The winner
 * of task t goes through the plane cell of (plane[t] in 0 .. 3, row[t] in 1 .. n; distinct cells) into p_out / nn_out / nl_out[t].
 * reps launches (1 .. 16) in a row on one workspace.  res: {items listed, tasks folded from more than one trip, the "fix_edges" bits,
 * tasks whose ticket was left nonzero} of the last launch; every launch adds its items to "fix_items". */
int32_t cp_test_fix_merge(const cp_model_t *model, int64_t ntask, const int64_t *toffs, const int64_t *part_v, const int32_t *part_p,
                          const int32_t *part_nn, const int32_t *part_nl, const int32_t *tile_s, const int32_t *tile_s2, const int32_t *anchor,
                          const int32_t *anchor2, const int32_t *row, const int32_t *plane, int64_t n, int32_t reps, int32_t *p_out,
                          int32_t *nn_out, int32_t *nl_out, int64_t *res);
/* Test entry: the link entries of the pattern split by bit plane, as the own tiles of the total-cost DP stream them ("own_split").
 * With nbits = the bits of n, nb = max(0, nbits - 8) planes b = 8 .. nbits - 1 (index b - 8) and, for an entry of column p (0-based)
 * whose row next occurs in column x (n: nowhere), h = the highest bit in which p and x differ: vnext_out -- the x of the entries with
 * h == b, plane by plane, column by column, in entry order (room for nnz values); vpos_out[(b - 8) (n + 1) + p], p = 0 .. n -- where
 * column p's entries of plane b start in it; vsa_out[(b - 8) (n + 1) + p] -- the entries of the columns < p with h > b.
 * res: {nb, entries in vnext_out}. */
int32_t cp_test_own_split(cp_csr_t csr, int32_t *vpos_out, int32_t *vsa_out, int32_t *vnext_out, int64_t *res);
/* Test entry (host only, no device): the slots of the run order that wave `wave` of the own-tile stream takes among nt tiles with
 * "own_pair" 1.  res: {1 if the wave has work, else 0; its first slot 2 wave; its second slot 2 wave + 1, or the first one again
 * where the order ends there (a lone wave: it stores one tile)}. */
int32_t cp_test_own_pair(int64_t nt, int64_t wave, int64_t *res);
/* Test entry: the arrays of cp_test_own_split as the own tiles read them with "own_pack" 1.  With c0 = p - p % 256 and k = p / 256,
 * blocks = ceil((n + 1) / 256): vpk_out[(b - 8) (n + 1) + p] = ((vpos[b][p] - vpos[b][c0]) & 0xffff) | (vsa[b][p] - vsa[b][c0]) << 16
 * (as the bits of an unsigned word; the low 16 bits of either offset where it is larger); vbase_out, pairs of 32-bit words: entry (b - 8) (blocks + 1) + k =
 * {vpos[b][256 k], vsa[b][256 k]} for k < blocks, and {the end of plane b's entries in vnext, 0} for k = blocks.
 * res: {nb, blocks, 1 if both offsets fit 16 bits everywhere (the pattern runs packed) else 0, the largest offset of vpos, of vsa}. */
int32_t cp_test_own_pack(cp_csr_t csr, int32_t *vpk_out, int32_t *vbase_out, int64_t *res);
/* Library-wide tunables and test switches; results never depend on them (tests/test_gpu_dynamic.py runs every one against the
 * oracle).  "force_brute" 1: the general O(K n^2) device DP even where the O(K n log^2 n) scheme applies; "brute_max_n": its size
 * limit.  "env_dc_min_n" (default 256, the measured crossover with the candidate sweep): the smallest n at which the total objective of
 * the envelope model (kind 15) in splitter order takes the divide and conquer over the cut column -- exact for Int64 models while
 * K max|alpha| + n |b_vertex| + N |b_pin| + K m |b_net| < 2^60 and for Float64 models with integral parameters while it is < 2^51, any
 * sign of the betas; below it, and for every other model of the kind, the candidate sweep up to "brute_max_n".  Layer driver of the O(K n log^2 n) scheme: "short_t"/"short_e" (tasks finished during setup),
 * "own_min" (shortest task with tiles of its own), "own_blk" (1, default: those tiles sit at absolute 256-column blocks and are
 * streamed in block order; 0: tiles counted from each task's head, in task order), "own_split" (1, default: outside the first round
 * and the gap rounds the own tiles of the planes >= 8 stream only the link entries whose count depends on the row, see
 * cp_test_own_split; 0: whole columns), "own_pair" (1, default: outside the gap rounds and the hyperedge costs a wave of the own-tile
 * stream takes two tiles of the run order, see cp_test_own_pair; 0: one), "own_pack" (1, default: while "own_split" and "own_blk" are 1
 * and the pattern's offsets fit, those tiles read a column's start and prefix sum as one 32-bit word, see cp_test_own_pack; 0: two words),
 * "round_alloc" (1, default: the task set-up of a round reserves its lists' offsets with their slots and ends with the round's verdict, see
 * cp_test_list_alloc; 0: the scan launch of cp_test_round_scans), "cr_consume" (1, default: in layers over all rows the set-up leaves the
 * right-pass counters zero as it reads them and the clearing launch runs only while they may be dirty; 0: in front of every such pass), "gap_tau"/"gap_min" (gap passes: rounds and task lengths; -1: none), "gap_nr" (64-row chunks per wave of the gap finish: 1 or 2), "pool" (1, default: freed device blocks of 1 MB and more are kept for reuse by the next call; 0: returned to HIP at once, and the pool is emptied),
 * "ra_cache" (round A from counts cached per partition), "nospec" 1 (one host sync per round instead of sizing a layer from the
 * previous one), "rpass_ch"/"rpass_small_tau"/"rpass_cap" (right-part passes: columns per wave, last
 * lane-per-row round, lane-private share of a row in per cent of the mean), "setup_bs" (lanes per block of the task setup), "force_max" (a round whose flattened
 * stage served at most this many tasks gives them tiles of their own from the next layer on), "leaf" (1: the rounds tau < 6 of a
 * layer are one leaf pass, csrc/dp_total_leaf.hip; 0: divide-and-conquer rounds down to tau = 0), "block_tables" (1: the leaf pass also
 * stores every per-block winner, needed by cp_dp_block_tables), "poison" (1: test mode of cp_get_stat above), "fixed_point" (1: layers
 * after one that reproduced its input row are copied), "bn_wave" (bottleneck DP walk: 0 lane per chunk of "bn_chunk" rows, 1 wave
 * per run of "bn_run" rows in lockstep, 2 = default: searched crossings for Int64 costs), "bn_slack" (columns of the start bracket), "lws" (1,
 * default: cp_pack_dynamic past the scan -- any width, a monotone work budget, no constraint -- runs the on-line divide and conquer of
 * csrc/chunk_lws.hip; 0: the one-wave kernel), "lws_leaf" (its rows per leaf wave: 256, 512, 1024 or 2048), "budget_total" (1, default:
 * the total-cost DP under a pin or work budget runs the two-staircase divide and conquer of csrc/dp_total_budget.hip; 0: the one-wave
 * kernel), "budget_scan_cells" / "budget_scan_cols" (that path scans a full rectangle whole while it has at most this many cells and
 * columns: 2^20 / 1024; at least 1), "budget_stair_cols" (... and the partial rows of a block of fewer columns than this: 1024),
 * "sym_total" (1, default: the total objective of a symmetric model inside its gate -- b_dia_net >= 0; b_local_net >= 0 and b_remote_net >=
 * b_local_net; b_self_pin <= b_cut_pin; integer-valued parameters and exact totals -- runs the divide and conquer of csrc/sym_total.hip at
 * any n; 0: the candidate sweep, n <= "brute_max_n"), "sym_total_min_n" (the smallest n that path takes while the
 * sweep is allowed, the measured crossover: 10240; where n > "brute_max_n" it runs from n = 1024 on instead of refusing), "sym_total_batch" (1,
 * default: the rectangles of one depth of its column tree share one launch sequence; 0: one sequence per rectangle), "sym_total_scan_cells" /
 * "sym_total_scan_cols" / "sym_total_stair_cols" (that path's limits, as the three budget options: 2^20 / 1024 / 1024; at least 1),
 * "plaid_total" (1, default: the total objective of the plaid connectivity pair in splitter order runs csrc/plaid_total.hip at any n --
 * the primary model with b_local_net >= 0 and b_remote_net >= 0 on the rectangle engine, the secondary model on the prefix-min scan, both
 * with integer-valued parameters and exact totals; 0: the candidate sweep, n <= "brute_max_n"), "plaid_total_min_n" / "plaid_scan_min_n"
 * (the smallest n the primary / the secondary path takes while the sweep is allowed: 1024 both, the first measured size; where n >
 * "brute_max_n" the primary runs from n = 1024 on and the secondary at any n instead of refusing), "plaid_total_scan_cells" /
 * "plaid_total_scan_cols" / "plaid_total_stair_cols" (the primary path's limits, as the three budget options: 2^20 / 1024 / 1024; at least 1),
 * "rcm_narrow" (cp_rcm: BFS levels of at most this many
 * vertices are walked by one workgroup, level after level in one launch; 0: every level by grid kernels; a value beyond the walker's
 * capacity of 1024 vertices: whenever the level fits), "greedy_lds_parts" (cp_partition_greedy_bottleneck: the walk keeps the part costs and counts in
 * LDS while K is at most this, default and largest value 2048; 0: always in global memory), "prof_only" slot (events on one profile slot only), "dbg"
 * (diagnostic bit mask: the bits are named in csrc/dp.hpp, enum DbgBit, and tabulated in DESIGN.md section 4e).  Unknown names
 * return CP_EINVAL. */
int32_t cp_set_option(const char *name, int64_t value);
/* built-in per-kernel HIP-event timing of the named hot kernels on the launch stream */
int32_t cp_prof_enable(int32_t on);
int32_t cp_prof_reset(void);
/* slot-wise totals: name, launches, total ms, algorithmic bytes; returns number of slots */
int32_t cp_prof_get(int32_t slot, const char **name, int64_t *launches, double *total_ms, double *alg_bytes);

#ifdef __cplusplus
}
#endif
#endif
