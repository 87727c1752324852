// blockcost.hpp -- BlockComponentCostModel without the stateful step oracle (blockcost.hip): the quotient pattern of the rows
// under a SplitPartition, the window table the (min,+) chunk scan reads, the stateless batch evaluation, and the gate of both.
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include <memory>

namespace cpk {

extern int64_t g_opt_blockcost_par;            // cp_set_option("blockcost_par"): 1 (default) the routes below; 0 the one-wave kernels of seq.hip
extern int64_t g_blockcost_scan_packs;         // chunker calls that ran table + scan for a block model (cp_get_stat("blockcost_scan_packs"))
extern int64_t g_blockcost_wave_evals;         // queries k_block_eval answered (cp_get_stat("blockcost_wave_evals"))

// Q = A with the rows of every part of Pi merged: Pi->K x A->n, one entry (k, c) per part k with a nonzero in column c, the parts
// of a column ascending.  Q: a fresh handle whose device and stream the caller has set; the work runs on A's stream, which is
// synchronised on return.  Pi must be a split of the rows (CP_EINVAL, in the words of seq_oracle); empty parts are legal.
void block_quotient(cp_csr_s *A, const cp_rowpart_t *Pi, cp_csr_s *Q);

// Do the table, the scan and the wave evaluation compute what block_call computes?  (blockcost.hip has the bound.)  Pi: the split Q
// was built from, already checked by block_quotient.
bool blockcost_exact(const cp_model_t *mdl, const cp_rowpart_t *Pi, const cp_csr_s *Q);

// The quotient pattern with its link arrays built and, entry by entry, the number of rows of the entry's part.
struct BlockQ {
    std::unique_ptr<cp_csr_s> Q;
    DBuf<int32_t> qu;
};
// ... for a model inside the gate; null outside it (the caller stays on the one-wave kernels)
std::unique_ptr<BlockQ> block_quotient_exact(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi);

// F[j' * (Wc + 1) + d] = cost(j' - d, j') for 0 <= d <= min(Wc, j' - 1), the layout of k_window_table; F: (n + 2) * (Wc + 1) entries,
// which the caller has held against block_table_fits (the size seq_window_table allows its tables)
inline bool block_table_fits(int64_t n, int64_t Wc) { return Wc >= 1 && (double)(n + 2) * (double)(Wc + 1) <= 6e8; }
template <typename TC>
void block_window_table(cp_csr_s *A, const BlockQ &B, const cp_model_t *mdl, const DevModel<TC> &M, int64_t Wc, DBuf<TC> &F);

// cp_oracle_eval for a block model, one wave per query.  false: not taken (the option, force_brute, a query outside
// 1 <= j <= j' <= n + 1, or a model outside the gate) -- the caller goes to run_seq_eval, which also words the errors.
template <typename TC>
bool run_block_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp, TC *out);

}  // namespace cpk
