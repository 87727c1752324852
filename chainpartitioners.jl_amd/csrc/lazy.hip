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
// (The chunk geometry, the shared prefix tables and lz_le are in lazy.hpp, shared with lazy_flip.hip.)
//
// The specialisation for AbstractMonotonizedSymmetricConnectivityModel (:260-388) is the same probe over the derived pattern D
// of sym.hpp: its cch / dia arrays together are D's link array, `deg(j') + (dia[j'] < j')` is the length of D's column, and the
// pin count comes from a prefix array of its own (overpos).  The body (lazy_body.inc) is shared by the two kernels; SEP selects
// that second prefix, and without it the body is the connectivity probe unchanged.
//
// The specialisation for AbstractPrimaryConnectivityModel under a row partition Pi (:390-483) is a kernel of its own further
// down (k_lazy_bisect_plaid): the same stream with the owner of every entry's row beside it.
#include "lazy.hpp"
#include "sym.hpp"

namespace cpk {

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

// ---------------------------------------------------------------- AbstractPrimaryConnectivityModel under a row partition (:390-483)
// The reference's probe keeps hst (last column of every row), and per part of Pi the pair lcl / drt (entries of the current column
// owned by that part).  In the link-array form, with eown[q] = owner[row[q]] and the open part k starting at column j:
//   n_local_net = #{q in columns [j, j'] : prev[q] < j and eown[q] == k},   x_comm = the same with eown[q] != k
// and the counts a split at column j' restarts from are lcl[k] = #{q in column j' : eown[q] == k} for the NEW k and deg(j') - lcl[k]
// (:447-454) -- every entry of column j' has prev[q] < j', so this is the same count.  They depend on k, so the split loop (:440-455)
// recounts the column in each of its iterations: a column too expensive as part k (its rows remote) may fit as part k + 1.
// The stream is k_lazy_bisect's with a second int32 stream (eown) beside prev and two flag masks per lane; the two per-lane counts
// travel through one block scan packed into a 32-bit word (a chunk holds at most 2^14 flags of either kind).
// (LazyPlaidShared, its lz_prefix and lz_primary: lazy.hpp)
// eown[q] = owner[row[q]]; the 16 entries behind N are written too (the probe's 16-byte loads reach into them)
__global__ void __launch_bounds__(256) k_lazy_eown(int64_t N, int64_t Npad, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                                                   int32_t *__restrict__ eown)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < Npad) eown[q] = q < N ? owner[row[q]] : 0;
}

template <typename TC>
__global__ void __launch_bounds__(LZ_T) k_lazy_bisect_plaid(DevModel<TC> M, int64_t n, int64_t N, int64_t K, const int32_t *__restrict__ pos,
                                                            const int32_t *__restrict__ prev, const int32_t *__restrict__ eown, double c_lo,
                                                            double c_hi, double eps, int64_t *__restrict__ spl, int64_t *__restrict__ spl_hi,
                                                            int64_t *__restrict__ nprobes)
{
    __shared__ LazyPlaidShared S;
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // spl / spl_hi live in global memory; every store is made by lane 0 only and read back after a barrier
    if (tid == 0) {
        for (int64_t k = 0; k <= K; k++) { spl[k] = 0; spl_hi[k] = n + 1; }
        spl[0] = 1; spl_hi[0] = 1;                                     // :398-402
    }
    for (int64_t k = 1; k <= K; k++) {                                 // :467-469  c_lo = max(c_lo, f(0, 0, 0, 0, k))
        double v = (double)lz_primary(M, dm_alpha(M, k), (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0);
        c_lo = c_lo < v ? v : c_lo;
    }
    int64_t probes = 0;
    bool stuck = false;
    while (c_lo * (1 + eps) < c_hi) {                                  // :471-480
        double c = (c_lo + c_hi) / 2;
        probes++;
        bool res = true;
        int64_t k = 1;
        int32_t j0 = 0;                                                // 0-based first column of the open part
        int32_t col = 0;                                               // next column to close
        int32_t qs = 0;                                                // next link entry to read
        int32_t cl0 = 0, cr0 = 0;                                      // local / remote nets of [j0, col) plus the flagged entries in [pos[col], qs)
        if (tid == 0) spl[0] = 1;
        while (col < n) {
            // ---- one chunk of link entries [qs, qe), loaded as aligned 16-byte pieces of prev and eown
            int32_t qa = qs & ~3;
            int32_t qe = (int32_t)((int64_t)qa + LZ_CH < N ? (int64_t)qa + LZ_CH : N);
            int32_t kk = k > INT32_MAX ? -1 : (int32_t)k;              // (owners are 1 .. Pi.K <= K)
            uint32_t ml = 0, mr = 0;
            {
                int32_t b = qa + tid * LZ_E;
#pragma unroll
                for (int v4 = 0; v4 < LZ_E / 4; v4++) {
                    int32_t x = b + 4 * v4;
                    if (x < qe) {                                      // both arrays are padded by 16 entries
                        int4 v = *reinterpret_cast<const int4 *>(prev + x);
                        int4 o = *reinterpret_cast<const int4 *>(eown + x);
                        uint32_t nw = 0, lc = 0;
                        if (x >= qs && v.x < j0) nw |= 1u;
                        if (x + 1 >= qs && x + 1 < qe && v.y < j0) nw |= 2u;
                        if (x + 2 >= qs && x + 2 < qe && v.z < j0) nw |= 4u;
                        if (x + 3 >= qs && x + 3 < qe && v.w < j0) nw |= 8u;
                        if (o.x == kk) lc |= 1u;
                        if (o.y == kk) lc |= 2u;
                        if (o.z == kk) lc |= 4u;
                        if (o.w == kk) lc |= 8u;
                        ml |= (nw & lc) << (4 * v4);
                        mr |= (nw & ~lc) << (4 * v4);
                    }
                }
            }
            uint32_t mine = (uint32_t)__popc(ml) | ((uint32_t)__popc(mr) << 16), incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { uint32_t pv = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += pv; }
            if (lane == 63) S.wsum[wave] = incl;
            __syncthreads();
            uint32_t wbase = 0;
            for (int w = 0; w < wave; w++) wbase += S.wsum[w];
            S.tbase[tid] = wbase + incl - mine;
            S.tml[tid] = (uint16_t)ml;
            S.tmr[tid] = (uint16_t)mr;
            if (tid == LZ_T - 1) S.total = wbase + incl;
            __syncthreads();
            // ---- close the columns that end inside the chunk, 1024 at a time
            bool restarted = false;
            while (col < n) {
                int32_t c_me = col + tid;
                int32_t e = (c_me < n) ? pos[c_me + 1] : INT32_MAX;
                bool complete = c_me < n && e <= qe;
                bool exceed = false;
                if (complete) {
                    uint32_t pr = lz_prefix(S, e - qa);
                    TC v = lz_primary(M, dm_alpha(M, k), (int64_t)(c_me - j0 + 1), (int64_t)(e - pos[j0]), (int64_t)cl0 + (int64_t)(pr & 0xffffu),
                                      (int64_t)cr0 + (int64_t)(pr >> 16));
                    exceed = !lz_le(v, c);
                }
                // first exceeding column and number of complete columns of this batch
                unsigned long long em = __ballot(exceed), cm = __ballot(complete);
                if (lane == 0) { S.red[wave] = em ? (wave * 64 + __ffsll((long long)em) - 1) : INT32_MAX; S.ncmp[wave] = __popcll(cm); }
                __syncthreads();
                int32_t fx = INT32_MAX, ncomp = 0;
                for (int w = 0; w < LZ_T / 64; w++) { fx = S.red[w] < fx ? S.red[w] : fx; ncomp += S.ncmp[w]; }
                __syncthreads();
                if (fx != INT32_MAX) {
                    // ---- split at column cx (:440-455): the column opens the next part on its own, counted for that part's number
                    int32_t cx = col + fx;
                    int32_t qb = pos[cx], deg = pos[cx + 1] - qb;
                    int32_t nloc = 0;
                    bool fail = false;
                    while (true) {
                        if (k == K) { fail = true; break; }            // :441-443
                        if (tid == 0) spl[k] = (int64_t)cx + 1;
                        j0 = cx;
                        k += 1;
                        // lcl[k] of the column (:451-454), block-strided: the column may be longer than a chunk
                        int32_t kn = k > INT32_MAX ? -1 : (int32_t)k, mc = 0;
                        for (int32_t q = qb + tid; q < qb + deg; q += LZ_T) mc += eown[q] == kn;
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) mc += __shfl_down(mc, o);
                        if (lane == 0) S.red[wave] = mc;
                        __syncthreads();
                        nloc = 0;
                        for (int w = 0; w < LZ_T / 64; w++) nloc += S.red[w];
                        __syncthreads();
                        if (lz_le(lz_primary(M, dm_alpha(M, k), (int64_t)1, (int64_t)deg, (int64_t)nloc, (int64_t)(deg - nloc)), c)) break;
                    }
                    if (fail) { res = false; col = (int32_t)n; restarted = true; break; }
                    col = cx + 1;
                    qs = pos[cx + 1];
                    cl0 = nloc; cr0 = deg - nloc;
                    restarted = true;
                    break;
                }
                col += ncomp;
                if (ncomp < LZ_T) break;                               // the next column ends beyond the chunk
            }
            if (!restarted) {
                cl0 += (int32_t)(S.total & 0xffffu);                   // everything flagged in [qs, qe) belongs to [j0, col]
                cr0 += (int32_t)(S.total >> 16);
                qs = qe;
            }
            __syncthreads();
        }
        if (res && tid == 0) for (int64_t t = k; t <= K; t++) spl[t] = n + 1;      // :457-460
        __syncthreads();
        // no bound moved: the reference would repeat this probe forever (non-positive bounds); block-uniform exit
        if ((res ? c_hi : c_lo) == c || probes > 4096) { stuck = true; break; }
        if (res) {
            c_hi = c;
            for (int64_t t = tid; t <= K; t += LZ_T) spl_hi[t] = spl[t];
        } else {
            c_lo = c;
        }
        __syncthreads();
    }
    if (tid == 0) *nprobes = stuck ? -1 : probes;
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
    const int64_t Npad = (A->N > 0 ? A->N : 1) + 16;
    DBuf<int32_t> eown((size_t)Npad);
    hipLaunchKernelGGL(k_lazy_eown, dim3((unsigned)cdiv(Npad, 256)), dim3(256), 0, s, A->N, Npad, A->row.p, R.owner.p, eown.p);
    CP_HIP(hipGetLastError());
    DBuf<int64_t> buf((size_t)(2 * (K + 1) + 1));
    int64_t *d_spl = buf.p, *d_hi = buf.p + (K + 1), *d_np = buf.p + 2 * (K + 1);
    {
        ProfScope ps(PROF_BISECT, s, 0.0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lazy_bisect_plaid<TC>), dim3(1), dim3(LZ_T), 0, s, HM.d, A->n, A->N, K, A->pos32.p, A->prev.p,
                           eown.p, c_lo, c_hi, eps, d_spl, d_hi, d_np);
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

// partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractPrimaryConnectivityModel, eps), Pi)
// (LazyBisectCostBottleneckSplitter.jl:390-483); every other kind: cp_partition_lazy_bisect_cost_probes, Pi is not looked at
extern "C" int32_t cp_partition_lazy_bisect_cost_pi(cp_csr_t A, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, double eps,
                                                    int64_t *spl_out, int64_t *nprobes_out)
{
    if (!model || model->kind != CP_MODEL_PRIMARY) return cp_partition_lazy_bisect_cost_probes(A, K, model, eps, spl_out, nprobes_out);
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl_out && K >= 1, CP_EINVAL, "bad argument");
        CP_REQUIRE(Pi && (Pi->asg || Pi->spl) && Pi->K >= 1, CP_EINVAL, "this cost model needs a row partition Pi");
        // the reference sizes lcl / drt by K and indexes them with the parts of Pi (:405-406, :426)
        CP_REQUIRE(Pi->K <= K, CP_EINVAL, "LazyBisectCost: the row partition has more parts than K");
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
        CP_REQUIRE(A->N < ((int64_t)1 << 31) - LZ_CH, CP_EUNSUPPORTED, "LazyBisectCost needs nnz < 2^31");
        return with_cost_type(model->dtype, [&](auto tag) { return run_lazy_plaid<decltype(tag)>(A, K, model, Pi, lf, hf, eps, spl_out, nprobes_out); });
    });
}

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
