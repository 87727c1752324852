// lazy_flip.hip -- partition_stripe(A, K, LazyFlipBisectCostBottleneckSplitter(f, eps), [Pi])
// (LazyBisectCostBottleneckSplitter.jl:72-138 of the reference) as ONE kernel launch, for decreasing costs: the connectivity
// family (per-part alpha included), the primary model under a row partition and the secondary model under a row split.
//
// The reference bisects on the cost c between bound_stripe's bounds as they are (no "c_lo = max(c_lo, f(1, 1, k))" step, unlike
// :55-57).  A probe first gives away leading empty parts while f(1, 1, k) <= c (:99-106), then walks j' = 2 .. n + 1 and closes part k
// BEHIND the first column that makes f(j, j', k) <= c; the new part starts empty at j', and f(j', j', k) is tested for every following
// k before another column is read (:108-120).  Reaching k == K on a cheap enough range is success; running out of columns is failure.
// The loop tests every j' in order, so "the first column whose inclusive prefix cost is <= c" is literal for any sign pattern.
//
// The probe runs over the chunk stream of lazy.hpp, like lazy.hip's forward probe; it stays a kernel of its own because it closes
// behind the first fitting column where the forward probe closes in front of the first exceeding one, and has the empty-part loops
// where that one has probe_init.  One kernel template, three modes:
//   connectivity  flag prev[q] < j0                                  cost f(nv, np, #flags)
//   primary       flags (prev[q] < j0) x (eown[q] == k), two counts    cost f(nv, np, #local, #remote)        (as lazy.hip's LB_PRIMARY)
//   secondary     flag e2[q] == k                                     cost f(|Pi_k|, pins(Pi_k), l, d_k - l)  (SecondaryConnectivityCosts.jl:82-89)
// e2[q] is the owner of entry q's row if q is the first entry of its column owned by that part and 0 otherwise (rows ascend inside a
// column and the parts of a split are contiguous: a comparison with the neighbouring entry), so l, the number of columns of [j, j')
// holding a row of part k, is the flag count since pos[j0], and d_k is the count over all columns.
#include "lazy.hpp"
#include "envelope.hpp"

namespace cpk {

enum { LF_CONN = 0, LF_PRIMARY = 1, LF_SECONDARY = 2 };

// e2 of the file comment, padded like eown, and dk[k - 1] = #{q : e2[q] == k} (zeroed by the caller); one atomic per wave and owner
__global__ void __launch_bounds__(256) k_lazy_e2(int64_t N, int64_t Npad, const int64_t *__restrict__ pos, const int32_t *__restrict__ col,
                                                 const int32_t *__restrict__ row, const int32_t *__restrict__ owner, int32_t *__restrict__ e2,
                                                 unsigned long long *__restrict__ dk)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int lane = threadIdx.x & 63;
    int32_t o = 0;
    if (q < N) {
        int32_t me = owner[row[q]];
        bool first = q == pos[col[q]] || owner[row[q - 1]] != me;
        o = first ? me : 0;
    }
    if (q < Npad) e2[q] = o;
    unsigned long long act = __ballot(o != 0);
    while (act) {                                                      // wave-uniform
        int src = __ffsll((long long)act) - 1;
        int32_t o0 = __shfl(o, src);
        unsigned long long same = __ballot(o == o0);
        if (lane == src) atomicAdd(dk + (o0 - 1), (unsigned long long)__popcll(same));
        act &= ~same;
    }
}

template <typename TC, int MODE>
__global__ void __launch_bounds__(LZ_T) k_lazy_flip(DevModel<TC> M, int64_t n, int64_t N, int64_t K, const int32_t *__restrict__ pos,
                                                    const int32_t *__restrict__ lnk, const int32_t *__restrict__ eown,
                                                    const int64_t *__restrict__ pspl, const int64_t *__restrict__ tpos,
                                                    const unsigned long long *__restrict__ dk, double c_lo, double c_hi, double eps,
                                                    int64_t *__restrict__ spl, int64_t *__restrict__ spl_hi, int64_t *__restrict__ nprobes)
{
    // lnk: prev (connectivity, primary) or e2 (secondary); eown: primary only; pspl / tpos / dk: secondary only
    constexpr bool PRI = MODE == LF_PRIMARY;
    constexpr int FLAGS = MODE == LF_SECONDARY ? LZ_OWNER : PRI ? LZ_NEW_OWN : LZ_NEW;
    __shared__ LazyShared<PRI> S;
    int tid = threadIdx.x;
    // the constants of part k (secondary: |Pi_k|, its pins, d_k; read once per k) and the cost of the empty range as part k
    int64_t nvk = 0, npk = 0, dkk = 0;
    auto empty_cost = [&](int64_t k) -> TC {
        if constexpr (MODE == LF_SECONDARY) {
            int64_t s0 = pspl[k - 1] - 1, s1 = pspl[k] - 1;
            nvk = s1 - s0; npk = tpos[s1] - tpos[s0]; dkk = (int64_t)dk[k - 1];
            return lz_primary(M, dm_alpha(M, k), nvk, npk, (int64_t)0, dkk);
        } else if constexpr (PRI) {
            return lz_primary(M, dm_alpha(M, k), (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0);
        } else {
            return lf_conn(M, dm_alpha(M, k), (int64_t)0, (int64_t)0, (int64_t)0);
        }
    };
    if constexpr (MODE == LF_SECONDARY) {
        // (c_lo, c_hi) = bound_stripe(A, K, Pi, ocl) ./ 1  (:125; SecondaryConnectivityCosts.jl:42-61) from the constants the probe reads
        // anyway: cp_bound_stripe_pi's values (it takes them from two oracle sweeps over the whole pattern, most of a call's time)
        TC lo = 0, hi = 0;
        for (int64_t k = 1; k <= K; k++) {
            int64_t s0 = pspl[k - 1] - 1, s1 = pspl[k] - 1;
            TC work = cadd(cadd(M.p[CP_P_ALPHA], cmulc(s1 - s0, M.p[CP_P_VERTEX])), cmulc(tpos[s1] - tpos[s0], M.p[CP_P_PIN]));
            TC full = cadd(work, cmulc((int64_t)dk[k - 1], M.p[CP_P_REMOTE_NET]));
            lo = work > lo ? work : lo;
            hi = full > hi ? full : hi;
        }
        c_lo = (double)lo; c_hi = (double)hi;
    }
    LazyBisection B(c_lo, c_hi, eps, n, K, spl, spl_hi);               // :87-91
    double c;
    while (B.next(c)) {                                                // :127-135
        bool res = false;
        int64_t k = 1;
        int32_t j0 = 0;                                                // 0-based first column of the open part
        int32_t col = 0;                                               // next column to test: j' = col + 2
        int32_t qs = 0;                                                // next link entry to read
        int32_t cnt0 = 0, cr0 = 0;                                     // flagged entries in [pos[j0], qs) (primary: local, remote)
        while (lz_le(empty_cost(k), c)) {                              // :99-106  leading empty parts
            if (k == K) { res = true; break; }
            if (tid == 0) spl[k] = 1;
            k += 1;
        }
        while (!res && col < n) {                                      // :108-120
            // ---- one chunk of link entries [qs, qe)
            int32_t qa, qe;
            uint32_t m0, m1;
            lz_load_flags<FLAGS>(lnk, eown, qs, N, j0, k, qa, qe, m0, m1);
            lz_publish(S, m0, m1);
            // ---- test the columns that end inside the chunk, 1024 at a time
            bool restarted = false;
            while (col < n) {
                int32_t c_me = col + tid;
                int32_t e = (c_me < n) ? pos[c_me + 1] : INT32_MAX;
                bool complete = c_me < n && e <= qe;
                bool fits = false;
                if (complete) {
                    uint32_t pr = lz_prefix(S, e - qa);
                    TC v;
                    if constexpr (MODE == LF_SECONDARY) {
                        int64_t l = (int64_t)cnt0 + (int64_t)pr;
                        v = lz_primary(M, dm_alpha(M, k), nvk, npk, l, dkk - l);
                    } else if constexpr (PRI) {
                        v = lz_primary(M, dm_alpha(M, k), (int64_t)(c_me - j0 + 1), (int64_t)(e - pos[j0]), (int64_t)cnt0 + (int64_t)(pr & 0xffffu),
                                       (int64_t)cr0 + (int64_t)(pr >> 16));
                    } else {
                        v = lf_conn(M, dm_alpha(M, k), (int64_t)(c_me - j0 + 1), (int64_t)(e - pos[j0]), (int64_t)cnt0 + (int64_t)pr);
                    }
                    fits = lz_le(v, c);
                }
                LazyBatch bt = lz_batch_reduce(S, fits, complete);     // first column of this batch that is cheap enough
                if (bt.first != INT32_MAX) {
                    // ---- close part k behind column cx (j' = cx + 2), then empty parts while f(j', j', k) <= c  (:110-118)
                    int32_t cx = col + bt.first;
                    while (true) {
                        if (k == K) { res = true; break; }
                        if (tid == 0) spl[k] = (int64_t)cx + 2;
                        k += 1;
                        if (!lz_le(empty_cost(k), c)) break;
                    }
                    j0 = cx + 1;
                    col = cx + 1;
                    qs = pos[cx + 1];
                    cnt0 = 0; cr0 = 0;
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
        if (res && tid == 0) spl[K] = n + 1;                           // :101, :112
        if (!B.close(res, c)) break;
    }
    B.finish(nprobes);
}

template <typename TC>
int32_t run_lazy_flip(cp_csr_s *A, int64_t K, const cp_model_t *mdl, const cp_rowpart_t *Pi, double c_lo, double c_hi, double eps,
                      int64_t *spl_out, int64_t *nprobes_out)
{
    hipStream_t s = A->stream;
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    ensure_links(A);
    const bool pri = mdl->kind == CP_MODEL_PRIMARY, sec = mdl->kind == CP_MODEL_SECONDARY;
    PlaidPart R;
    DBuf<int32_t> own;                                                 // eown (primary) or e2 (secondary)
    DBuf<unsigned long long> dk;
    if (pri || sec) {
        upload_part(A, Pi, sec, R);
        const int64_t Npad = lazy_padded(A->N);
        own.alloc((size_t)Npad);
        if (pri) {
            hipLaunchKernelGGL(k_lazy_eown, dim3((unsigned)cdiv(Npad, 256)), dim3(256), 0, s, A->N, Npad, A->row.p, R.owner.p, own.p);
        } else {
            dk.alloc((size_t)K);
            CP_HIP(hipMemsetAsync(dk.p, 0, dk.bytes(), s));
            hipLaunchKernelGGL(k_lazy_e2, dim3((unsigned)cdiv(Npad, 256)), dim3(256), 0, s, A->N, Npad, A->pos.p, A->col.p, A->row.p, R.owner.p,
                               own.p, dk.p);
        }
        CP_HIP(hipGetLastError());
    }
    return lazy_run(A, K, spl_out, nprobes_out, [&](int64_t *d_spl, int64_t *d_hi, int64_t *d_np) {
        const int64_t *nil = nullptr;
        if (sec)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_flip<TC, LF_SECONDARY>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, own.p,
                               (const int32_t *)nullptr, R.spl.p, A->tpos.p, dk.p, c_lo, c_hi, eps, d_spl, d_hi, d_np);
        else if (pri)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_flip<TC, LF_PRIMARY>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, A->prev.p,
                               own.p, nil, nil, (const unsigned long long *)nullptr, c_lo, c_hi, eps, d_spl, d_hi, d_np);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_flip<TC, LF_CONN>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, A->prev.p,
                               (const int32_t *)nullptr, nil, nil, (const unsigned long long *)nullptr, c_lo, c_hi, eps, d_spl, d_hi, d_np);
    });
}

}  // namespace cpk

using namespace cpk;

extern "C" int32_t cp_partition_lazy_flip_bisect_cost(cp_csr_t A, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                                      int64_t *spl_out, int64_t *nprobes_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model && spl_out && K >= 1, CP_EINVAL, "bad argument");
        CP_REFUSE_ENV(model, "LazyFlipBisectCost");
        const int32_t kind = model->kind;
        const bool pri = kind == CP_MODEL_PRIMARY, sec = kind == CP_MODEL_SECONDARY;
        if (!(kind == CP_MODEL_CONNECTIVITY || kind == CP_MODEL_COLBLOCK || pri || sec)) {
            const char *name = kind == CP_MODEL_WORK ? "work" : kind == CP_MODEL_POWER_WORK ? "power work" : kind == CP_MODEL_HYPEREDGE_CUT ? "hyperedge cut"
                             : kind == CP_MODEL_BLOCK ? "block" : kind == CP_MODEL_SYM_CONNECTIVITY ? "symmetric connectivity"
                             : kind == CP_MODEL_MONO_SYM_CONNECTIVITY ? "monotonized symmetric connectivity" : kind == CP_MODEL_SYM_EDGE_CUT ? "symmetric edge cut"
                             : kind == CP_MODEL_PRIMARY_EDGE_CUT ? "primary edge cut" : kind == CP_MODEL_SECONDARY_EDGE_CUT ? "secondary edge cut" : "this";
            set_error(std::string("LazyFlipBisectCost has no device path for the ") + name + " model (kind " + std::to_string(kind) + ")");
            return CP_EUNSUPPORTED;
        }
        if (pri || sec) lazy_require_rowpart("LazyFlipBisectCost", Pi, K, pri);
        // the reference's secondary oracle indexes Pi.spl[k + 1] for k up to K (SecondaryConnectivityCosts.jl:84-87)
        if (sec) CP_REQUIRE(Pi->spl && Pi->K == K, CP_EINVAL, "LazyFlipBisectCost: the secondary model needs a SplitPartition of the rows with exactly K parts");
        CP_HIP(hipSetDevice(A->device));
        // (c_lo, c_hi) = bound_stripe(A, K, args..., ocl) ./ 1  (:125): what the Bisect entries take for the same model
        double lf = 0, hf = 0;
        int32_t rc = CP_OK;
        if (sec) {
            // cp_bound_stripe_pi's values, computed by the kernel from |Pi_k|, pins(Pi_k) and d_k; its assertion stays here
            const bool neg = with_cost_type(model->dtype, [&](auto tag) {
                using TC = decltype(tag);
                return model_param<TC>(model, 1) < 0 || model_param<TC>(model, 2) < 0 || model_param<TC>(model, 3) < 0 || model_param<TC>(model, 4) < 0;
            });
            CP_REQUIRE(!neg, CP_EINVAL, "bound_stripe asserts beta >= 0");
        } else if (pri && model->alpha_k && model->n_alpha_k > 0) {
            rc = with_cost_type(model->dtype, [&](auto tag) { return lazy_plaid_funky_bound<decltype(tag)>(A, K, model, Pi, &lf, &hf); });
        } else {
            int64_t li, hi;
            rc = cp_bound_stripe_pi(A, K, Pi, model, &li, &hi, &lf, &hf);
        }
        if (rc != CP_OK) return rc;
        lazy_require_int32("LazyFlipBisectCost", A->N, "nnz");
        return with_cost_type(model->dtype, [&](auto tag) { return run_lazy_flip<decltype(tag)>(A, K, model, pri || sec ? Pi : nullptr, lf, hf, eps, spl_out, nprobes_out); });
    });
}
