// lazy.hpp -- the chunk stream of the lazy probes, stated once: lazy.hip (LazyBisectCost) and lazy_flip.hip (LazyFlipBisectCost)
// build their kernels from the stages below.  One workgroup of 1024 lanes reads a link array in chunks of 16 Ki entries, 16 per
// lane; a flag per entry goes into a 16-bit mask, one block scan of the per-lane counts gives every column's count as the prefix
// at its last entry, and the first qualifying column of a batch of 1024 is a block minimum.  After a split the stream restarts
// behind the split column.  The stages, in the order a kernel calls them:
//   LazyBisection     the bisection on the cost c around a probe: spl / spl_hi, the bounds, the exit, the probe count
//   lz_load_flags     chunk window [qa, qe) of the restart point qs and the lane's flag masks of it
//   lz_publish        block scan of the counts; tbase / masks / total into shared memory
//   lz_prefix         the flag count of [qa, qa + i) from those tables
//   lz_batch_reduce   (first hit, number of complete columns) of a batch of columns
// Every stage is called by all 1024 lanes under block-uniform control: the loops around them run on values that are the same in
// every lane (arguments, shared-memory reductions read behind a barrier), which is what lets the stages hold barriers.
// Also here: the comparison with the Float64 bisection value, the narrow cost formulas, the owner stream, the bound of a primary
// model with per-part alpha and the host side every probe shares (argument checks, result buffer, launch scope, error).
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include <string>
#include <type_traits>
#include <vector>

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
constexpr int LZ_W = LZ_T / 64;        // waves

// TWO: a second flag mask per lane; the two counts then travel packed as first | second << 16 (a chunk holds at most 2^14
// flags of a kind, so with one mask the packed word is the plain count)
template <bool TWO>
struct LazyShared {
    uint32_t tbase[LZ_T];              // exclusive prefix of the per-lane flag counts
    uint16_t tmask[TWO ? 2 : 1][LZ_T]; // flags of the lane's 16 entries
    uint32_t wsum[LZ_W];               // lz_publish: inclusive count of every wave
    int32_t wfirst[LZ_W], wcnt[LZ_W];  // lz_batch_reduce / lz_block_sum: per-wave first hit, per-wave count
    uint32_t total;
};

// ---------------------------------------------------------------- chunk window and flag load
// The flag of link entry q, for the open part k that starts at column j0:
enum { LZ_NEW = 0,                     // lnk[q] < j0                                    (lnk = prev: the row is new to the part)
       LZ_NEW_OWN = 1,                 // the same, split by eown[q] == k into two masks  (local, remote)
       LZ_OWNER = 2 };                 // lnk[q] == k                                    (lnk = e2)

// Chunk of the stream that restarts at entry qs: the window [qa, qe) with qa = qs rounded down to a 16-byte piece, and the lane's
// masks of its 16 entries qa + 16 tid ..; entries in front of qs or behind qe carry no flag.  A piece that begins in front of qe
// is loaded whole, so every streamed array needs 16 readable entries behind N: prev (core.hip, ensure_links: Na + 16), dprev
// (sym.hip, ensure_sym_links: Nd + 16) and eown / e2 (Npad = N + 16, written to the end by k_lazy_eown / k_lazy_e2).
template <int FLAGS>
__device__ __forceinline__ void lz_load_flags(const int32_t *__restrict__ lnk, const int32_t *__restrict__ eown, int32_t qs, int64_t N,
                                              int32_t j0, int64_t k, int32_t &qa, int32_t &qe, uint32_t &m0, uint32_t &m1)
{
    qa = qs & ~3;
    qe = (int32_t)((int64_t)qa + LZ_CH < N ? (int64_t)qa + LZ_CH : N);
    const int32_t kk = k > INT32_MAX ? -1 : (int32_t)k;               // (owners are 1 .. Pi.K <= K)
    const int32_t b = qa + (int32_t)threadIdx.x * LZ_E;
    m0 = 0; m1 = 0;
#pragma unroll
    for (int v4 = 0; v4 < LZ_E / 4; v4++) {
        int32_t x = b + 4 * v4;
        if (x < qe) {
            int4 v = *reinterpret_cast<const int4 *>(lnk + x);
            uint32_t in = 0, nw = 0;
            if (x >= qs) in |= 1u;
            if (x + 1 >= qs && x + 1 < qe) in |= 2u;
            if (x + 2 >= qs && x + 2 < qe) in |= 4u;
            if (x + 3 >= qs && x + 3 < qe) in |= 8u;
            if constexpr (FLAGS == LZ_OWNER) {
                if (v.x == kk) nw |= 1u;
                if (v.y == kk) nw |= 2u;
                if (v.z == kk) nw |= 4u;
                if (v.w == kk) nw |= 8u;
            } else {
                if (v.x < j0) nw |= 1u;
                if (v.y < j0) nw |= 2u;
                if (v.z < j0) nw |= 4u;
                if (v.w < j0) nw |= 8u;
            }
            nw &= in;
            if constexpr (FLAGS == LZ_NEW_OWN) {
                int4 o = *reinterpret_cast<const int4 *>(eown + x);
                uint32_t lc = 0;
                if (o.x == kk) lc |= 1u;
                if (o.y == kk) lc |= 2u;
                if (o.z == kk) lc |= 4u;
                if (o.w == kk) lc |= 8u;
                m0 |= (nw & lc) << (4 * v4);
                m1 |= (nw & ~lc) << (4 * v4);
            } else {
                m0 |= nw << (4 * v4);
            }
        }
    }
}

// ---------------------------------------------------------------- publish
template <bool TWO>
__device__ __forceinline__ void lz_publish(LazyShared<TWO> &S, uint32_t m0, uint32_t m1)
{
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t mine = (uint32_t)__popc(m0), incl;
    if constexpr (TWO) mine |= (uint32_t)__popc(m1) << 16;
    incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t pv = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += pv; }
    if (lane == 63) S.wsum[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave; w++) wbase += S.wsum[w];
    S.tbase[tid] = wbase + incl - mine;
    S.tmask[0][tid] = (uint16_t)m0;
    if constexpr (TWO) S.tmask[1][tid] = (uint16_t)m1;
    if (tid == LZ_T - 1) S.total = wbase + incl;
    __syncthreads();
}

// #flagged entries in [qa, qa + i), packed like the counts
template <bool TWO>
__device__ __forceinline__ uint32_t lz_prefix(const LazyShared<TWO> &S, int32_t i)
{
    if (i >= LZ_CH) return S.total;
    int t = i >> 4;
    uint32_t low = (1u << (i & 15)) - 1u;
    uint32_t r = S.tbase[t] + (uint32_t)__popc((uint32_t)S.tmask[0][t] & low);
    if constexpr (TWO) r += (uint32_t)__popc((uint32_t)S.tmask[1][t] & low) << 16;
    return r;
}

// ---------------------------------------------------------------- batch reduce
// Lane t holds column col + t of a batch.  Returns, the same in every lane, the first t with `hit` (INT32_MAX if none) and the
// number of lanes with `complete` (complete columns are a prefix of the batch).  (The count is summed in front of the minimum:
// with the two the other way round k_lazy_flip's primary mode gets 81 VGPRs for the same instructions, a step of occupancy.)
struct LazyBatch { int32_t first, ncomp; };
template <bool TWO>
__device__ __forceinline__ LazyBatch lz_batch_reduce(LazyShared<TWO> &S, bool hit, bool complete)
{
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long hm = __ballot(hit), cm = __ballot(complete);
    if (lane == 0) { S.wfirst[wave] = hm ? (wave * 64 + __ffsll((long long)hm) - 1) : INT32_MAX; S.wcnt[wave] = __popcll(cm); }
    __syncthreads();
    LazyBatch r{INT32_MAX, 0};
    for (int w = 0; w < LZ_W; w++) { r.ncomp += S.wcnt[w]; r.first = S.wfirst[w] < r.first ? S.wfirst[w] : r.first; }
    __syncthreads();
    return r;
}

// block sum of a per-lane count, the same in every lane
template <bool TWO>
__device__ __forceinline__ int32_t lz_block_sum(LazyShared<TWO> &S, int32_t v)
{
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) S.wcnt[wave] = v;
    __syncthreads();
    int32_t r = 0;
    for (int w = 0; w < LZ_W; w++) r += S.wcnt[w];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- bisection frame
// while (B.next(c)) { res = probe at c, lane 0 writing spl; if (!B.close(res, c)) break; }  B.finish(nprobes);
// spl / spl_hi live in global memory.  Every member is block-uniform; spl and *nprobes are stored by lane 0 only and spl is read
// (by all lanes, for the copy to spl_hi) behind the barrier that opens close().
struct LazyBisection {
    double c_lo, c_hi, eps;
    int64_t K;
    int64_t *__restrict__ spl, *__restrict__ spl_hi;
    int64_t probes;
    bool stuck;

    __device__ __forceinline__ LazyBisection(double lo, double hi, double eps_, int64_t n_, int64_t K_, int64_t *spl_, int64_t *spl_hi_)
        : c_lo(lo), c_hi(hi), eps(eps_), K(K_), spl(spl_), spl_hi(spl_hi_), probes(0), stuck(false)
    {
        if (threadIdx.x == 0) {
            for (int64_t k = 0; k <= K; k++) { spl[k] = 0; spl_hi[k] = n_ + 1; }
            spl[0] = 1; spl_hi[0] = 1;
        }
    }
    __device__ __forceinline__ bool next(double &c)
    {
        if (!(c_lo * (1 + eps) < c_hi)) return false;
        c = (c_lo + c_hi) / 2;
        probes++;
        if (threadIdx.x == 0) spl[0] = 1;
        return true;
    }
    // false: the bisection is stuck, leave the loop
    __device__ __forceinline__ bool close(bool res, double c)
    {
        __syncthreads();
        // no bound moved: the reference would repeat this probe forever (non-positive bounds)
        if ((res ? c_hi : c_lo) == c || probes > 4096) { stuck = true; return false; }
        if (res) {
            c_hi = c;
            for (int64_t t = threadIdx.x; t <= K; t += LZ_T) spl_hi[t] = spl[t];
        } else {
            c_lo = c;
        }
        __syncthreads();
        return true;
    }
    __device__ __forceinline__ void finish(int64_t *__restrict__ nprobes) const
    {
        if (threadIdx.x == 0) *nprobes = stuck ? -1 : probes;
    }
};

// ---------------------------------------------------------------- cost formulas
// The probes evaluate the one or two kinds they can meet, not dm_apply: its whole switch sends the Float64 kernels to scratch.
// kinds 2 and 4 of dm_apply, slot for slot
template <typename TC>
__device__ __forceinline__ TC lf_conn(const DevModel<TC> &m, TC alpha, int64_t nv, int64_t np, int64_t nn)
{
    if (m.kind == CP_MODEL_COLBLOCK)
        return cadd(dm_comp(m.ac_const, m.ac_c, m.ac_tab, m.ac_len, m.ac_lo, nv),
                    cmulc(nn, dm_comp(m.bc_const[0], m.bc_c[0], m.bc_tab[0], m.bc_len[0], m.bc_lo[0], nv)));
    return cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])), cmulc(nn, m.p[CP_P_NET]));
}

// kind 8 of dm_apply, slot for slot
template <typename TC>
__device__ __forceinline__ TC lz_primary(const DevModel<TC> &m, TC alpha, int64_t nv, int64_t np, int64_t nl, int64_t nr)
{
    return cadd(cadd(cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN])), cmulc(nl, m.p[CP_P_LOCAL_NET])),
                cmulc(nr, m.p[CP_P_REMOTE_NET]));
}

// lazy.hip: eown[q] = owner[row[q]]; the 16 entries behind N are written too (lz_load_flags reads into them)
__global__ void __launch_bounds__(256) k_lazy_eown(int64_t N, int64_t Npad, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                                                   int32_t *__restrict__ eown);
inline int64_t lazy_padded(int64_t N) { return (N > 0 ? N : 1) + 16; }

// ---------------------------------------------------------------- host side
// `who` is the splitter's name in the message: LazyBisectCost or LazyFlipBisectCost
inline void lazy_require_rowpart(const char *who, const cp_rowpart_t *Pi, int64_t K, bool at_most_K)
{
    CP_REQUIRE(Pi && (Pi->asg || Pi->spl) && Pi->K >= 1, CP_EINVAL, "this cost model needs a row partition Pi");
    // the reference sizes lcl / drt by K and indexes them with the parts of Pi (:405-406, :426)
    if (at_most_K) CP_REQUIRE(Pi->K <= K, CP_EINVAL, std::string(who) + ": the row partition has more parts than K");
}
// the stream indexes with int32 and a window may end LZ_CH behind its start; `what` names N: nnz, or nnz + n for the pattern D
inline void lazy_require_int32(const char *who, int64_t N, const char *what)
{
    CP_REQUIRE(N < ((int64_t)1 << 31) - LZ_CH, CP_EUNSUPPORTED, std::string(who) + " needs " + what + " < 2^31");
}

// The tail of every probe: owns the device buffer spl[K + 1] | spl_hi[K + 1] | nprobes, runs launch(spl, spl_hi, nprobes) (one kernel
// on A->stream) as the PROF_BISECT scope, and returns spl_hi and the probe count.
template <typename Launch>
int32_t lazy_run(cp_csr_s *A, int64_t K, int64_t *spl_out, int64_t *nprobes_out, Launch &&launch)
{
    hipStream_t s = A->stream;
    DBuf<int64_t> buf((size_t)(2 * (K + 1) + 1));
    int64_t *d_spl = buf.p, *d_hi = buf.p + (K + 1), *d_np = buf.p + 2 * (K + 1);
    {
        ProfScope ps(PROF_BISECT, s, 0.0);
        launch(d_spl, d_hi, d_np);
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

// bound_stripe(A, K, Pi, f) of a primary model with per-part alpha, the reference tests' FunkyPrimaryConnectivityModel
// (test_Partitioners.jl:43-48): (minimum, maximum) of (minimum(alpha), maximum(alpha), maximum_k ocl(1, n + 1, k)), k = 1 .. K.
// The oracle takes part numbers up to Pi.K, so Pi is widened to K parts (the added ones own no row).
template <typename TC>
int32_t lazy_plaid_funky_bound(cp_csr_s *A, int64_t K, const cp_model_t *mdl, const cp_rowpart_t *Pi, double *lo, double *hi)
{
    CP_REQUIRE(mdl->n_alpha_k >= K, CP_EINVAL, "bound_stripe: fewer per-part alphas than parts");
    cp_rowpart_t wide;
    std::vector<int64_t> wspl;
    wide.K = K; wide.asg = Pi->asg; wide.spl = nullptr;
    if (!Pi->asg) {
        wspl.assign(Pi->spl, Pi->spl + Pi->K + 1);
        wspl.resize((size_t)K + 1, A->m + 1);
        wide.spl = wspl.data();
    }
    std::vector<int64_t> one((size_t)K, 1), np1((size_t)K, A->n + 1), ks((size_t)K);
    for (int64_t k = 0; k < K; k++) ks[(size_t)k] = k + 1;
    std::vector<TC> v((size_t)K);
    const bool i64 = std::is_same<TC, int64_t>::value;
    int32_t rc = cp_oracle_eval(A, mdl, &wide, CP_HINT_STEP, K, one.data(), np1.data(), ks.data(), i64 ? (int64_t *)v.data() : nullptr,
                                i64 ? nullptr : (double *)v.data());
    if (rc != CP_OK) return rc;
    const TC *al = (const TC *)mdl->alpha_k;
    TC amin = al[0], amax = al[0], fmax = v[0];
    for (int64_t i = 1; i < mdl->n_alpha_k; i++) { amin = std::min(amin, al[i]); amax = std::max(amax, al[i]); }
    for (int64_t k = 1; k < K; k++) fmax = std::max(fmax, v[(size_t)k]);
    *lo = (double)std::min(amin, std::min(amax, fmax)); *hi = (double)std::max(amin, std::max(amax, fmax));
    return CP_OK;
}

}  // namespace cpk
