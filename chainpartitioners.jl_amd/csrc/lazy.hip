// lazy.hip -- partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f, eps), [Pi])
// (LazyBisectCostBottleneckSplitter.jl:140-483 of the reference) as ONE kernel launch: the forward probe over the
// chunk stream of lazy.hpp, one kernel template with three modes.
//
// The reference bisects on the cost c; a probe is one forward scan over the columns that closes a part IN FRONT OF the first column
// whose cost exceeds c; that column opens the next part on its own.  Its cached array cch[q] (previous column holding the row of
// nonzero q, :153-170) is exactly the link array `prev` that ensure_links builds, so the flag of the stream is prev[q] < part start
// and the net count of a column range is a flag count.
//   LB_CONN     AbstractConnectivityModel (:140-258).  probe_init and probe read the same data here; they differ only in the
//               reference's control flow at k == K (:171, :180 vs :208-211), which is kept (`first`).
//   LB_PINS     AbstractMonotonizedSymmetricConnectivityModel (:260-388): the same probe over the derived pattern D of sym.hpp.  Its
//               cch / dia arrays together are D's link array, `deg(j') + (dia[j'] < j')` is the length of D's column, and the pin
//               count comes from a prefix array of its own (overpos) instead of pos.
//   LB_PRIMARY  AbstractPrimaryConnectivityModel under a row partition Pi (:390-483).  The reference's probe keeps hst (last column
//               of every row), and per part of Pi the pair lcl / drt (entries of the current column owned by that part).  In the
//               link-array form, with eown[q] = owner[row[q]] and the open part k starting at column j:
//                 n_local_net = #{q in columns [j, j'] : prev[q] < j and eown[q] == k},   x_comm = the same with eown[q] != k
//               so eown streams beside prev and the flags split into two masks.  The counts a split at column j' restarts from are
//               lcl[k] = #{q in column j' : eown[q] == k} for the NEW k and deg(j') - lcl[k] (:447-454) -- every entry of column j'
//               has prev[q] < j', so this is the same count.  They depend on k, so the split loop (:440-455) recounts the column in
//               each of its iterations: a column too expensive as part k (its rows remote) may fit as part k + 1.  This method
//               has no probe_init.
#include "lazy.hpp"
#include "sym.hpp"
#include "envelope.hpp"

namespace cpk {

enum { LB_CONN = 0, LB_PINS = 1, LB_PRIMARY = 2 };

// eown[q] = owner[row[q]]; the 16 entries behind N are written too (lz_load_flags reads into them)
__global__ void __launch_bounds__(256) k_lazy_eown(int64_t N, int64_t Npad, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                                                   int32_t *__restrict__ eown)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < Npad) eown[q] = q < N ? owner[row[q]] : 0;
}

// pin: LB_PINS only; eown: LB_PRIMARY only
template <typename TC, int MODE>
__global__ void __launch_bounds__(LZ_T) k_lazy_bisect(DevModel<TC> M, int64_t n, int64_t N, int64_t K, const int32_t *__restrict__ pos,
                                                      const int32_t *__restrict__ pin, const int32_t *__restrict__ prev,
                                                      const int32_t *__restrict__ eown, double c_lo, double c_hi, double eps,
                                                      int64_t *__restrict__ spl, int64_t *__restrict__ spl_hi,
                                                      int64_t *__restrict__ nprobes)
{
    constexpr bool PRI = MODE == LB_PRIMARY;
    __shared__ LazyShared<PRI> S;
    int tid = threadIdx.x;
    // cost as part k of nv columns with np pins and the counts (a, b) = (nets, -) or (local nets, remote nets)
    auto cost = [&](int64_t k, int64_t nv, int64_t np, int64_t a, int64_t b) -> TC {
        if constexpr (PRI) return lz_primary(M, dm_alpha(M, k), nv, np, a, b);
        else return lf_conn(M, dm_alpha(M, k), nv, np, a);
    };
    LazyBisection B(c_lo, c_hi, eps, n, K, spl, spl_hi);               // :146-150 / :398-402
    for (int64_t k = 1; k <= K; k++) {                                 // :233-235 / :467-469  c_lo = max(c_lo, f(0, 0, 0, k))
        double v = (double)cost(k, 0, 0, 0, 0);
        B.c_lo = B.c_lo < v ? v : B.c_lo;
    }
    bool first = !PRI;                                                 // the first probe is probe_init (the primary method has none)
    double c;
    while (B.next(c)) {                                                // :237-247, :249-257 / :471-480
        bool res = true;
        int64_t k = 1;
        int32_t j0 = 0;                                                // 0-based first column of the open part
        int32_t col = 0;                                               // next column to close
        int32_t qs = 0;                                                // next link entry to read
        int32_t cnt0 = 0, cr0 = 0;                                     // nets (primary: local, remote) of [j0, col) plus the flagged entries in [pos[col], qs)
        while (col < n) {
            // ---- one chunk of link entries [qs, qe)
            int32_t qa, qe;
            uint32_t m0, m1;
            lz_load_flags<PRI ? LZ_NEW_OWN : LZ_NEW>(prev, eown, qs, N, j0, k, qa, qe, m0, m1);
            lz_publish(S, m0, m1);
            // ---- close the columns that end inside the chunk, 1024 at a time
            bool restarted = false;
            bool checks = !first || k < K;                             // probe_init stops checking once k == K (:171)
            while (col < n) {
                int32_t c_me = col + tid;
                int32_t e = (c_me < n) ? pos[c_me + 1] : INT32_MAX;
                bool complete = c_me < n && e <= qe;
                bool exceed = false;
                if (complete && checks) {
                    uint32_t pr = lz_prefix(S, e - qa);
                    int64_t np = MODE == LB_PINS ? pin[c_me + 1] - pin[j0] : e - pos[j0];
                    TC v = cost(k, (int64_t)(c_me - j0 + 1), np, (int64_t)cnt0 + (int64_t)(PRI ? pr & 0xffffu : pr), (int64_t)cr0 + (int64_t)(pr >> 16));
                    exceed = !lz_le(v, c);
                }
                LazyBatch bt = lz_batch_reduce(S, exceed, complete);   // first exceeding column of this batch
                if (bt.first != INT32_MAX) {
                    // ---- split in front of column cx (:208-219 / :440-455): the column opens the next part on its own
                    int32_t cx = col + bt.first;
                    int32_t qb = pos[cx], deg = pos[cx + 1] - qb;
                    int32_t dpin = MODE == LB_PINS ? pin[cx + 1] - pin[cx] : deg;
                    int32_t nloc = deg;                                // entries of the column that count first (primary: the local ones)
                    bool fail = false;
                    while (true) {
                        if (!first && k == K) { fail = true; break; }  // :209-211 / :441-443
                        if (tid == 0) spl[k] = (int64_t)cx + 1;
                        j0 = cx;
                        k += 1;
                        if constexpr (PRI) {
                            // lcl[k] of the column for the new k (:451-454), block-strided: the column may be longer than a chunk
                            int32_t kn = k > INT32_MAX ? -1 : (int32_t)k, mc = 0;
                            for (int32_t q = qb + tid; q < qb + deg; q += LZ_T) mc += eown[q] == kn;
                            nloc = lz_block_sum(S, mc);
                        }
                        bool again = (!first || k < K) && !lz_le(cost(k, (int64_t)1, (int64_t)dpin, (int64_t)nloc, (int64_t)(deg - nloc)), c);
                        if (!again) break;
                    }
                    if (fail) { res = false; col = (int32_t)n; restarted = true; break; }
                    col = cx + 1;
                    qs = pos[cx + 1];
                    cnt0 = nloc; cr0 = deg - nloc;
                    restarted = true;
                    break;
                }
                col += bt.ncomp;
                if (bt.ncomp < LZ_T) break;                            // the next column ends beyond the chunk
            }
            if (!restarted) {
                cnt0 += (int32_t)(PRI ? S.total & 0xffffu : S.total);  // everything flagged in [qs, qe) belongs to [j0, col]
                cr0 += (int32_t)(S.total >> 16);
                qs = qe;
            }
            __syncthreads();
        }
        if (res) {
            if (first) {                                               // :180  res = k < K || f(...) <= c
                int64_t nv = n - j0, np = (n > 0 ? (MODE == LB_PINS ? (int64_t)pin[n] - pin[j0] : (int64_t)pos[n] - pos[j0]) : 0);
                res = k < K || lz_le(cost(K, nv, np, (int64_t)cnt0, (int64_t)0), c);
            }
            if (tid == 0) for (int64_t t = k; t <= K; t++) spl[t] = n + 1;    // :181-184 / :221-224 / :457-460
        }
        if (!B.close(res, c)) break;
        first = false;
    }
    B.finish(nprobes);
}

template <typename TC>
int32_t run_lazy(cp_csr_s *A, int64_t K, const cp_model_t *mdl, double c_lo, double c_hi, double eps, int64_t *spl_out, int64_t *nprobes_out)
{
    hipStream_t s = A->stream;
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    ensure_links(A);
    const bool sym = mdl->kind == CP_MODEL_MONO_SYM_CONNECTIVITY;
    SymHost SH;
    SymWork *SW = nullptr;
    if (sym) {
        sym_prepare(A, mdl, SH);
        SW = sym_work_get(A);
        lazy_require_int32("LazyBisectCost", SW->Nd, "nnz + n");
        HM.d.kind = CP_MODEL_CONNECTIVITY;      // alpha + nv*b_vertex + pins*b_over_pin + nets*b_dia_net: the connectivity formula, slot for slot
    }
    return lazy_run(A, K, spl_out, nprobes_out, [&](int64_t *d_spl, int64_t *d_hi, int64_t *d_np) {
        const int32_t *nil = nullptr;
        if (sym)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect<TC, LB_PINS>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, SW->Nd, K, SW->dpos32.p, SH.pin32,
                               SW->dprev.p, nil, c_lo, c_hi, eps, d_spl, d_hi, d_np);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect<TC, LB_CONN>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, nil,
                               A->prev.p, nil, c_lo, c_hi, eps, d_spl, d_hi, d_np);
    });
}

template <typename TC>
int32_t run_lazy_plaid(cp_csr_s *A, int64_t K, const cp_model_t *mdl, const cp_rowpart_t *Pi, double c_lo, double c_hi, double eps,
                       int64_t *spl_out, int64_t *nprobes_out)
{
    hipStream_t s = A->stream;
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    ensure_links(A);
    PlaidPart R;
    upload_part(A, Pi, false, R);
    const int64_t Npad = lazy_padded(A->N);
    DBuf<int32_t> eown((size_t)Npad);
    hipLaunchKernelGGL(k_lazy_eown, dim3((unsigned)cdiv(Npad, 256)), dim3(256), 0, s, A->N, Npad, A->row.p, R.owner.p, eown.p);
    CP_HIP(hipGetLastError());
    return lazy_run(A, K, spl_out, nprobes_out, [&](int64_t *d_spl, int64_t *d_hi, int64_t *d_np) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect<TC, LB_PRIMARY>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p,
                           (const int32_t *)nullptr, A->prev.p, eown.p, c_lo, c_hi, eps, d_spl, d_hi, d_np);
    });
}

}  // namespace cpk

using namespace cpk;

// partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractPrimaryConnectivityModel, eps), Pi)
// (LazyBisectCostBottleneckSplitter.jl:390-483); every other kind: cp_partition_lazy_bisect_cost_probes, Pi is not looked at
extern "C" int32_t cp_partition_lazy_bisect_cost_pi(cp_csr_t A, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                                    int64_t *spl_out, int64_t *nprobes_out)
{
    if (!model || model->kind != CP_MODEL_PRIMARY) return cp_partition_lazy_bisect_cost_probes(A, K, model, eps, spl_out, nprobes_out);
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl_out && K >= 1, CP_EINVAL, "bad argument");
        lazy_require_rowpart("LazyBisectCost", Pi, K, true);
        CP_HIP(hipSetDevice(A->device));
        double lf, hf;
        if (model->alpha_k && model->n_alpha_k > 0) {
            int32_t rc = with_cost_type(model->dtype, [&](auto tag) { return lazy_plaid_funky_bound<decltype(tag)>(A, K, model, Pi, &lf, &hf); });
            if (rc != CP_OK) return rc;
        } else {
            int64_t li, hi;
            int32_t rc = cp_bound_stripe(A, K, model, &li, &hi, &lf, &hf);    // :465, the model form: Pi is dropped (Costs.jl:17-19)
            if (rc != CP_OK) return rc;
        }
        lazy_require_int32("LazyBisectCost", A->N, "nnz");
        return with_cost_type(model->dtype, [&](auto tag) { return run_lazy_plaid<decltype(tag)>(A, K, model, Pi, lf, hf, eps, spl_out, nprobes_out); });
    });
}

// the same call, also returning the number of probes the bisection ran (tests, tools/bench_symmetric.py)
extern "C" int32_t cp_partition_lazy_bisect_cost_probes(cp_csr_t A, int64_t K, const cp_model_t *model, double eps, int64_t *spl_out, int64_t *nprobes_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model && spl_out && K >= 1, CP_EINVAL, "bad argument");
        CP_REFUSE_ENV(model, "LazyBisectCost");
        // only AbstractConnectivityModel reaches the specialised method; other models hit the generic one whose g() asserts
        // false for them (LazyBisectCostBottleneckSplitter.jl:486-501)
        CP_REQUIRE(model->kind == CP_MODEL_CONNECTIVITY || model->kind == CP_MODEL_COLBLOCK || model->kind == CP_MODEL_MONO_SYM_CONNECTIVITY, CP_EINVAL,
                   "LazyBisectCost: the reference asserts on models that are not connectivity models");
        CP_HIP(hipSetDevice(A->device));
        int64_t li, hi; double lf, hf;
        int32_t rc = cp_bound_stripe(A, K, model, &li, &hi, &lf, &hf);        // :231
        if (rc != CP_OK) return rc;
        lazy_require_int32("LazyBisectCost", A->N, "nnz");
        return with_cost_type(model->dtype, [&](auto tag) { return run_lazy<decltype(tag)>(A, K, model, lf, hf, eps, spl_out, nprobes_out); });
    });
}

extern "C" int32_t cp_partition_lazy_bisect_cost(cp_csr_t A, int64_t K, const cp_model_t *model, double eps, int64_t *spl_out)
{
    return cp_partition_lazy_bisect_cost_probes(A, K, model, eps, spl_out, nullptr);
}
