// lazy.hip -- partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractConnectivityModel, eps))
// (/root/reference/src/LazyBisectCostBottleneckSplitter.jl:140-258) as ONE kernel launch.
//
// The reference bisects on the cost c; a probe is one forward scan over the columns that closes a part at the
// first column whose cost exceeds c.  Its cached array cch[q] (previous column holding the row of nonzero q,
// :153-170) is exactly the link array `prev` that ensure_links builds, so probe_init and probe read the same data
// here; they differ only in the reference's control flow at k == K (:171, :180 vs :208-211), which is kept.
//
// One workgroup of 1024 lanes streams the link array in 16 Ki-entry chunks: 16 entries per lane, flags
// (prev[q] < part start) packed into a 16-bit mask, one block-wide scan of the per-lane counts; the count of a
// column is the prefix at its last entry; the first exceeding column of the chunk is a block-wide minimum.  After
// a split the stream restarts behind the split column with the new threshold.  All control state is block-uniform.
//
// The specialisation for AbstractMonotonizedSymmetricConnectivityModel (:260-388) is the same probe over the derived pattern D
// of sym.hpp: its cch / dia arrays together are D's link array, `deg(j') + (dia[j'] < j')` is the length of D's column, and the
// pin count comes from a prefix array of its own (overpos).  The body (lazy_body.inc) is shared by the two kernels; SEP selects
// that second prefix, and without it the body is the connectivity probe unchanged.
#include "csr.hpp"
#include "model.hpp"
#include "sym.hpp"

namespace cpk {

__device__ __forceinline__ bool lz_le(int64_t v, double c)
{
    if (c != c) return false;
    if (c >= 9223372036854775808.0) return true;
    if (c < -9223372036854775808.0) return false;
    return v <= (int64_t)floor(c);
}
__device__ __forceinline__ bool lz_le(double v, double c) { return v <= c; }

constexpr int LZ_T = 1024;             // lanes
constexpr int LZ_E = 16;               // link entries per lane and chunk
constexpr int LZ_CH = LZ_T * LZ_E;

struct LazyShared {
    int32_t tbase[LZ_T];               // exclusive prefix of the per-lane flag counts
    uint16_t tmask[LZ_T];              // flags of the lane's 16 entries
    int32_t wsum[LZ_T / 64];
    int32_t red[LZ_T / 64];
    int32_t total;
};

// #flagged entries in [qa, qa + i)
__device__ __forceinline__ int32_t lz_prefix(const LazyShared &S, int32_t i)
{
    if (i >= LZ_CH) return S.total;
    int t = i >> 4, r = i & 15;
    return S.tbase[t] + __popc((uint32_t)S.tmask[t] & ((1u << r) - 1u));
}

template <typename TC>
__global__ void __launch_bounds__(LZ_T) k_lazy_bisect(DevModel<TC> M, int64_t n, int64_t N, int64_t K, const int32_t *__restrict__ pos,
                                                      const int32_t *__restrict__ prev, double c_lo, double c_hi, double eps,
                                                      int64_t *__restrict__ spl, int64_t *__restrict__ spl_hi,
                                                      int64_t *__restrict__ nprobes)
{
    __shared__ LazyShared S;
    constexpr bool SEP = false;
    const int32_t *pin = nullptr;
#include "lazy_body.inc"
}

// the same probe with the pin count read from `pin` (the symmetric specialisation: pos / prev are D's)
template <typename TC>
__global__ void __launch_bounds__(LZ_T) k_lazy_bisect_pins(DevModel<TC> M, int64_t n, int64_t N, int64_t K, const int32_t *__restrict__ pos,
                                                           const int32_t *__restrict__ pin, const int32_t *__restrict__ prev, double c_lo,
                                                           double c_hi, double eps, int64_t *__restrict__ spl, int64_t *__restrict__ spl_hi,
                                                           int64_t *__restrict__ nprobes)
{
    __shared__ LazyShared S;
    constexpr bool SEP = true;
#include "lazy_body.inc"
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
        CP_REQUIRE(SW->Nd < ((int64_t)1 << 31) - LZ_CH, CP_EUNSUPPORTED, "LazyBisectCost needs nnz + n < 2^31");
        HM.d.kind = CP_MODEL_CONNECTIVITY;      // alpha + nv*b_vertex + pins*b_over_pin + nets*b_dia_net: the connectivity formula, slot for slot
    }
    DBuf<int64_t> buf((size_t)(2 * (K + 1) + 1));
    int64_t *d_spl = buf.p, *d_hi = buf.p + (K + 1), *d_np = buf.p + 2 * (K + 1);
    {
        ProfScope ps(PROF_BISECT, s, 0.0);
        if (sym)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect_pins<TC>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, SW->Nd, K, SW->dpos32.p, SH.pin32,
                               SW->dprev.p, c_lo, c_hi, eps, d_spl, d_hi, d_np);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect<TC>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, A->prev.p,
                               c_lo, c_hi, eps, d_spl, d_hi, d_np);
    }
    CP_HIP(hipGetLastError());
    int64_t np_host = 0;
    CP_HIP(hipMemcpyAsync(spl_out, d_hi, sizeof(int64_t) * (size_t)(K + 1), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(&np_host, d_np, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    CP_REQUIRE(np_host >= 0, CP_EINVAL, "cost bisection cannot terminate on these bounds (the reference loops forever: non-positive costs)");
    if (nprobes_out) *nprobes_out = np_host;
    return CP_OK;
}

}  // namespace cpk

using namespace cpk;

// the same call, also returning the number of probes the bisection ran (tests, tools/bench_symmetric.py)
extern "C" int32_t cp_partition_lazy_bisect_cost_probes(cp_csr_t A, int64_t K, const cp_model_t *model, double eps, int64_t *spl_out, int64_t *nprobes_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model && spl_out && K >= 1, CP_EINVAL, "bad argument");
        // only AbstractConnectivityModel reaches the specialised method; other models hit the generic one whose g() asserts
        // false for them (LazyBisectCostBottleneckSplitter.jl:486-501)
        CP_REQUIRE(model->kind == CP_MODEL_CONNECTIVITY || model->kind == CP_MODEL_COLBLOCK || model->kind == CP_MODEL_MONO_SYM_CONNECTIVITY, CP_EINVAL,
                   "LazyBisectCost: the reference asserts on models that are not connectivity models");
        CP_HIP(hipSetDevice(A->device));
        int64_t li, hi; double lf, hf;
        int32_t rc = cp_bound_stripe(A, K, model, &li, &hi, &lf, &hf);        // :231
        if (rc != CP_OK) return rc;
        CP_REQUIRE(A->N < ((int64_t)1 << 31) - LZ_CH, CP_EUNSUPPORTED, "LazyBisectCost needs nnz < 2^31");
        return with_cost_type(model->dtype, [&](auto tag) { return run_lazy<decltype(tag)>(A, K, model, lf, hf, eps, spl_out, nprobes_out); });
    });
}

extern "C" int32_t cp_partition_lazy_bisect_cost(cp_csr_t A, int64_t K, const cp_model_t *model, double eps, int64_t *spl_out)
{
    return cp_partition_lazy_bisect_cost_probes(A, K, model, eps, spl_out, nullptr);
}
