// map_part.hip -- the two partitioners of the reference that return a MapPartition (src/MagneticPartitioner.jl), on the device:
//   cp_partition_magnetic            MagneticPartitioner.jl:3-20     a column takes the part of one drawn row of its own
//   cp_partition_greedy_bottleneck   MagneticPartitioner.jl:26-177   a column takes the costliest part among its rows' parts, and
//                                                                    that part's cost is lowered before the next column looks
// The reference draws from Julia's global RNG (rand, randperm); here the draws are inputs -- arrays, or the counter hash
//     draw(seed, stream, idx) = SplitMix64(key(seed, stream) + idx * 0x2545F4914F6CDD1D) >> 1      (draws.py states it for the host)
// with stream 1 the Magnetic draws and stream 2 the keys the Greedy visiting order is sorted by; idx is the 1-based column.
//
// Greedy runs in three phases:
//   setup   the counts of every part of Pi (vertices, pins, remote nets) from A's own columns -- no adjoint: the (part, column)
//           pairs of all entries are sorted once, a part's pins are its run of the sorted keys and its nets the distinct keys of
//           that run, found by K binary searches; no atomics, exact for any column length and any K
//   gather  the part of every entry in visiting order as one contiguous stream, and the prefix of the column lengths in that
//           order: every dependent random load is taken off the sequential chain
//   walk    k_greedy_walk: one wave, column after column (column t + 1 sees column t's update).  The lanes read their entries'
//           parts and cst[part], a wave arg-max picks the first entry in column order among the maxima, chunks of 64 entries carry
//           the running best with the reference's strict test, and the chosen part's cost is recomputed from its counts.  The
//           state lives in LDS up to "greedy_lds_parts" parts and in global memory above.
#include "csr.hpp"
#include "model.hpp"
#include "envelope.hpp"
#include <rocprim/rocprim.hpp>

namespace cpk {

constexpr int GREEDY_LDS_MAX = 2048;             // parts whose walk state fits the walker's LDS (24 bytes a part)
int64_t g_opt_greedy_lds_parts = GREEDY_LDS_MAX; // the walk keeps its state in LDS while K <= this (0: always in global memory)

// ------------------------------------------------------------------ draws
__host__ __device__ __forceinline__ uint64_t sm64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t stream_key(int64_t seed, uint64_t stream) { return sm64((uint64_t)seed + stream * 0xD1342543DE82EF95ull); }
__device__ __forceinline__ int64_t draw_at(uint64_t key, int64_t idx) { return (int64_t)(sm64(key + (uint64_t)idx * 0x2545F4914F6CDD1Dull) >> 1); }

// ------------------------------------------------------------------ checks (before anything is indexed by these values)
// asg: 1-based int64 -> owner: 0-based int32; a value outside 1 .. K raises *bad and becomes part 0
__global__ void k_map_owner(const int64_t *__restrict__ asg, int32_t *__restrict__ owner, int64_t m, int64_t K, int32_t *__restrict__ bad)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t a = asg[i];
    if (a < 1 || a > K) { *bad = 1; owner[i] = 0; return; }
    owner[i] = (int32_t)(a - 1);
}
__global__ void k_map_draws_check(const int64_t *__restrict__ draws, int64_t n, int32_t *__restrict__ bad)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && draws[j] < 0) *bad = 1;
}

// ------------------------------------------------------------------ Magnetic
// one lane per column: the draw, the drawn entry's row, that row's part (draws == nullptr: draw(seed, 1, j))
__global__ void k_magnetic(const int64_t *__restrict__ pos, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                           const int64_t *__restrict__ draws, uint64_t key, int64_t n, int64_t K, int64_t *__restrict__ asg)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t u = draws ? draws[j] : draw_at(key, j + 1);
    const int64_t b = pos[j], d = pos[j + 1] - b;
    asg[j] = d == 0 ? 1 + u % K : (int64_t)owner[row[b + u % d]] + 1;
}

// ------------------------------------------------------------------ Greedy: setup
__global__ void k_greedy_keys(uint64_t key, int64_t n, uint64_t *__restrict__ k, uint32_t *__restrict__ v)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) { k[j] = (uint64_t)draw_at(key, j + 1); v[j] = (uint32_t)j; }
}
__global__ void k_greedy_emit_order(const int32_t *__restrict__ ord, int64_t *__restrict__ out, int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = (int64_t)ord[t] + 1;
}
// entry q of column c whose row is owned by part k -> the key k * n + c; one thread per entry, the column by binary search
__global__ void k_greedy_pairs(const int64_t *__restrict__ pos, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                               uint64_t *__restrict__ key, int64_t n, int64_t N)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pos[mid] <= q) lo = mid; else hi = mid;
    }
    key[q] = (uint64_t)owner[row[q]] * (uint64_t)n + (uint64_t)lo;
}
__global__ void k_greedy_owner_keys(const int32_t *__restrict__ owner, uint32_t *__restrict__ key, int64_t m)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) key[i] = (uint32_t)owner[i];
}
__global__ void k_greedy_distinct(const uint64_t *__restrict__ skey, int32_t *__restrict__ flag, int64_t N)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < N) flag[q] = (q == 0 || skey[q] != skey[q - 1]) ? 1 : 0;
}
// first index of the ascending a[0 .. len) with a[i] >= x
template <typename T> __device__ __forceinline__ int64_t lower_bound(const T *__restrict__ a, int64_t len, T x)
{
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// one thread per part: its vertices, pins and remote nets from the sorted keys; cst[k] and the part of it the walk never changes,
//     c0 = alpha_k + nv * b_vertex + np * b_pin,      cst = c0 + nl * b_local_net + nr * b_remote_net      (left to right)
template <typename TC>
__global__ void k_greedy_counts(const uint32_t *__restrict__ sown, int64_t m, const uint64_t *__restrict__ skey, const int64_t *__restrict__ dscan,
                                int64_t n, int64_t N, int64_t K, DevModel<TC> M, TC *__restrict__ c0, TC *__restrict__ cst, int32_t *__restrict__ nl,
                                int32_t *__restrict__ nr)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t nv = lower_bound<uint32_t>(sown, m, (uint32_t)(k + 1)) - lower_bound<uint32_t>(sown, m, (uint32_t)k);
    const int64_t a = lower_bound<uint64_t>(skey, N, (uint64_t)k * (uint64_t)n), b = lower_bound<uint64_t>(skey, N, (uint64_t)(k + 1) * (uint64_t)n);
    const int64_t np = b - a, rem = dscan[b] - dscan[a];
    const TC base = cadd(cadd(dm_alpha(M, k + 1), cmulc(nv, M.p[CP_P_VERTEX])), cmulc(np, M.p[CP_P_PIN]));
    c0[k] = base;
    nl[k] = 0;
    nr[k] = (int32_t)rem;
    cst[k] = cadd(cadd(base, cmulc((int64_t)0, M.p[CP_P_LOCAL_NET])), cmulc(rem, M.p[CP_P_REMOTE_NET]));
}

// ------------------------------------------------------------------ Greedy: gather
__global__ void k_greedy_len(const int64_t *__restrict__ pos, const int32_t *__restrict__ ord, int32_t *__restrict__ len, int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t c = ord[t];
    len[t] = (int32_t)(pos[c + 1] - pos[c]);
}
// entry q of the stream belongs to the t-th visited column (binary search in the prefix gpos): the part of its row
__global__ void k_greedy_stream(const int64_t *__restrict__ pos, const int32_t *__restrict__ row, const int32_t *__restrict__ owner,
                                const int32_t *__restrict__ ord, const int32_t *__restrict__ gpos, int32_t *__restrict__ stream, int64_t n, int64_t N)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (gpos[mid] <= q) lo = mid; else hi = mid;
    }
    stream[q] = owner[row[pos[ord[lo]] + (q - gpos[lo])]];
}

// ------------------------------------------------------------------ Greedy: walk
__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int o)
{
    return ((int64_t)__shfl_xor((int)(v >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(v & 0xffffffffll), o);
}
__device__ __forceinline__ double shfl_xor64(double v, int o) { return __longlong_as_double(shfl_xor64((int64_t)__double_as_longlong(v), o)); }

// One wave.  stream / gpos are the gather's; the state arrays hold K parts each and are read and written in LDS copies when LDS.
// Every quantity a branch depends on (the column's end, the chunk count, the winner) is the same in all lanes.  The loads of the
// chunk after the one in hand are issued before its reduction: a chunk starts where the previous one ends, whatever column it is of.
template <typename TC, bool LDS>
__global__ void __launch_bounds__(64) k_greedy_walk(const int32_t *__restrict__ stream, const int32_t *__restrict__ gpos, const int32_t *__restrict__ ord,
                                                    int32_t n, int32_t N, int32_t K, const TC *__restrict__ c0, TC *g_cst, int32_t *g_nl, int32_t *g_nr,
                                                    TC b_local, TC b_remote, int64_t *__restrict__ asg)
{
    __shared__ TC s_c0[LDS ? GREEDY_LDS_MAX : 1], s_cst[LDS ? GREEDY_LDS_MAX : 1];
    __shared__ int32_t s_nl[LDS ? GREEDY_LDS_MAX : 1], s_nr[LDS ? GREEDY_LDS_MAX : 1];
    const int lane = threadIdx.x;
    if (LDS) {
        for (int32_t k = lane; k < K; k += 64) { s_c0[k] = c0[k]; s_cst[k] = g_cst[k]; s_nl[k] = g_nl[k]; s_nr[k] = g_nr[k]; }
        __syncthreads();
    }
    const TC *bc = LDS ? s_c0 : c0;
    TC *cst = LDS ? s_cst : g_cst;
    int32_t *nl = LDS ? s_nl : g_nl, *nr = LDS ? s_nr : g_nr;
    int32_t start = 0;
    int32_t cur = lane < N ? stream[lane] : 0;
    for (int32_t t0 = 0; t0 < n; t0 += 64) {
        const bool have = t0 + lane < n;
        const int32_t ge = have ? gpos[t0 + lane + 1] : N;          // where the column this lane reports ends in the stream
        const int32_t oc = have ? ord[t0 + lane] : 0;
        int32_t res = 0;
        const int32_t tn = n - t0 < 64 ? n - t0 : 64;
        for (int32_t tt = 0; tt < tn; tt++) {
            const int32_t end = __shfl(ge, tt);
            TC best_c = CostTraits<TC>::typemin();
            int32_t best_k = -1;
            for (;;) {
                const int32_t cnt = end - start < 64 ? end - start : 64;
                const int32_t nstart = start + cnt;
                const int32_t nxt = nstart + lane < N ? stream[nstart + lane] : 0;
                if (cnt > 0) {
                    const bool valid = lane < cnt;
                    TC c = valid ? cst[cur] : CostTraits<TC>::typemin();
                    int32_t i = valid ? lane : 64;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const TC c2 = shfl_xor64(c, o);
                        const int32_t i2 = __shfl_xor(i, o);
                        if (i2 < 64 && (i >= 64 || c2 > c || (c2 == c && i2 < i))) { c = c2; i = i2; }
                    }
                    const int32_t p = __shfl(cur, i);                // (lane 0 is valid: i < 64)
                    if (best_k < 0 || c > best_c) { best_c = c; best_k = p; }
                }
                start = nstart;
                cur = nxt;
                if (start >= end) break;
            }
            if (best_k >= 0) {
                if (lane == 0) {
                    const int32_t l = nl[best_k] + 1, r = nr[best_k] - 1;
                    nl[best_k] = l; nr[best_k] = r;
                    cst[best_k] = cadd(cadd(bc[best_k], cmulc((int64_t)l, b_local)), cmulc((int64_t)r, b_remote));
                }
                __syncthreads();
            }
            if (lane == tt) res = best_k < 0 ? 1 : best_k + 1;
        }
        if (have) asg[oc] = res;
    }
    if (LDS) {
        __syncthreads();
        for (int32_t k = lane; k < K; k += 64) { g_cst[k] = s_cst[k]; g_nl[k] = s_nl[k]; g_nr[k] = s_nr[k]; }
    }
}

// ------------------------------------------------------------------ host
// Pi -> owner (0-based parts, m entries) on the device, every value checked there; Pi->asg (m entries) or, without it, Pi->spl
static void map_owner(cp_csr_s *A, const cp_rowpart_t *Pi, DBuf<int32_t> &owner, hipStream_t s)
{
    CP_REQUIRE(Pi && (Pi->asg || Pi->spl) && Pi->K >= 1, CP_EINVAL, "this partitioner needs a row partition Pi");
    const int64_t m = A->m, K = Pi->K;
    owner.alloc((size_t)(m > 0 ? m : 1));
    if (m <= 0) return;
    std::vector<int64_t> expanded;
    const int64_t *asg = Pi->asg;
    if (!asg) {
        CP_REQUIRE(Pi->spl[0] == 1 && Pi->spl[K] == m + 1, CP_EINVAL, "split vector must run from 1 to m+1");
        expanded.assign((size_t)m, 0);
        for (int64_t k = 1; k <= K; k++) {
            CP_REQUIRE(Pi->spl[k] >= Pi->spl[k - 1] && Pi->spl[k] <= m + 1, CP_EINVAL, "split vector out of range");
            for (int64_t i = Pi->spl[k - 1]; i < Pi->spl[k]; i++) expanded[(size_t)i - 1] = k;
        }
        asg = expanded.data();
    }
    DBuf<int64_t> d((size_t)m);
    DBuf<int32_t> bad(1);
    CP_HIP(hipMemcpyAsync(d.p, asg, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemsetAsync(bad.p, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_map_owner, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, d.p, owner.p, m, K, bad.p);
    CP_HIP(hipGetLastError());
    int32_t hb = 0;
    CP_HIP(hipMemcpyAsync(&hb, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    CP_REQUIRE(!hb, CP_EINVAL, "row owner out of range: Pi.asg must hold values of 1 .. Pi.K");
}

static unsigned key_bits(uint64_t x) { unsigned b = 1; while (b < 64 && ((uint64_t)1 << b) <= x) b++; return b; }

template <typename TC>
static int32_t run_greedy(cp_csr_s *A, int64_t K, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t seed, const int64_t *order,
                          int64_t *asg_out, int64_t *order_out, TC *cst_out)
{
    hipStream_t s = A->stream;
    const int64_t m = A->m, n = A->n, N = A->N;
    DBuf<int32_t> owner, ord((size_t)(n > 0 ? n : 1)), flag(1);
    DBuf<char> tmp;
    map_owner(A, Pi, owner, s);
    // the visiting order: given (checked to be a permutation), or the columns sorted by (draw(seed, 2, j), j)
    if (n > 0 && order) {
        DBuf<int64_t> d((size_t)n);
        DBuf<int32_t> mark((size_t)n);
        CP_HIP(hipMemcpyAsync(d.p, order, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        CP_HIP(hipMemsetAsync(mark.p, 0, mark.bytes(), s));
        CP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(k_perm_check, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, d.p, ord.p, mark.p, n, flag.p);
        CP_HIP(hipGetLastError());
        int32_t hb = 0;
        CP_HIP(hipMemcpyAsync(&hb, flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        CP_REQUIRE(!hb, CP_EINVAL, "cp_partition_greedy_bottleneck: order is not a permutation of 1 .. n");
    } else if (n > 0) {
        DBuf<uint64_t> ka((size_t)n), kb((size_t)n);
        DBuf<uint32_t> va((size_t)n);
        hipLaunchKernelGGL(k_greedy_keys, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, stream_key(seed, 2), n, ka.p, va.p);
        size_t bytes = 0;
        CP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, ka.p, kb.p, va.p, (uint32_t *)ord.p, (size_t)n, 0u, 63u, s));
        tmp.ensure(bytes > 0 ? bytes : 1);
        CP_HIP(rocprim::radix_sort_pairs((void *)tmp.p, bytes, ka.p, kb.p, va.p, (uint32_t *)ord.p, (size_t)n, 0u, 63u, s));
        CP_HIP(hipStreamSynchronize(s));                            // (ka, kb, va go out of scope)
    }
    const size_t Ks = (size_t)K;
    DBuf<TC> c0(Ks), cst(Ks);
    DBuf<int32_t> nl(Ks), nr(Ks);
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    {   // ---- setup
        ProfScope ps(PROF_MAP_SETUP, s, 12.0 * (double)N + 4.0 * (double)m);
        const size_t Ns = (size_t)(N > 0 ? N : 1), ms = (size_t)(m > 0 ? m : 1);
        DBuf<uint64_t> ka(Ns), kb(Ns);
        DBuf<uint32_t> oa(ms), ob(ms);
        DBuf<int32_t> dist(Ns);
        DBuf<int64_t> dscan(Ns + 1), scratch;
        size_t bytes = 0;
        if (m > 0) {
            hipLaunchKernelGGL(k_greedy_owner_keys, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, owner.p, oa.p, m);
            const unsigned eb = key_bits((uint64_t)K);
            CP_HIP(rocprim::radix_sort_keys(nullptr, bytes, oa.p, ob.p, (size_t)m, 0u, eb, s));
            tmp.ensure(bytes > 0 ? bytes : 1);
            CP_HIP(rocprim::radix_sort_keys((void *)tmp.p, bytes, oa.p, ob.p, (size_t)m, 0u, eb, s));
        }
        if (N > 0) {
            hipLaunchKernelGGL(k_greedy_pairs, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, A->pos.p, A->row.p, owner.p, ka.p, n, N);
            const unsigned eb = key_bits((uint64_t)K * (uint64_t)n);
            CP_HIP(rocprim::radix_sort_keys(nullptr, bytes, ka.p, kb.p, (size_t)N, 0u, eb, s));
            tmp.ensure(bytes > 0 ? bytes : 1);
            CP_HIP(rocprim::radix_sort_keys((void *)tmp.p, bytes, ka.p, kb.p, (size_t)N, 0u, eb, s));
            hipLaunchKernelGGL(k_greedy_distinct, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, kb.p, dist.p, N);
        }
        exclusive_scan_i32(dist.p, dscan.p, N > 0 ? N : 0, scratch, s);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_greedy_counts<TC>), dim3((unsigned)cdiv(K, 256)), dim3(256), 0, s, ob.p, m > 0 ? m : 0, kb.p, dscan.p,
                           n, N > 0 ? N : 0, K, HM.d, c0.p, cst.p, nl.p, nr.p);
        CP_HIP(hipGetLastError());
        CP_HIP(hipStreamSynchronize(s));                            // (the scope's buffers are released below)
    }
    DBuf<int32_t> len((size_t)(n > 0 ? n : 1)), gpos((size_t)n + 1), stream((size_t)(N > 0 ? N : 1));
    DBuf<int64_t> dasg((size_t)(n > 0 ? n : 1)), dord((size_t)(n > 0 && order_out ? n : 1)), scratch;
    if (n > 0) {
        {   // ---- gather
            ProfScope ps(PROF_MAP_GATHER, s, 16.0 * (double)N + 12.0 * (double)n);
            hipLaunchKernelGGL(k_greedy_len, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, A->pos.p, ord.p, len.p, n);
            exclusive_scan_i32_i32(len.p, gpos.p, n, scratch, s);
            if (N > 0)
                hipLaunchKernelGGL(k_greedy_stream, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, A->pos.p, A->row.p, owner.p, ord.p, gpos.p, stream.p, n, N);
            CP_HIP(hipGetLastError());
        }
        {   // ---- walk
            ProfScope ps(PROF_MAP_WALK, s, 4.0 * (double)N + 16.0 * (double)n);
            const TC bl = HM.d.p[CP_P_LOCAL_NET], br = HM.d.p[CP_P_REMOTE_NET];
            if (K <= g_opt_greedy_lds_parts && K <= GREEDY_LDS_MAX)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_greedy_walk<TC, true>), dim3(1), dim3(64), 0, s, stream.p, gpos.p, ord.p, (int32_t)n, (int32_t)N,
                                   (int32_t)K, c0.p, cst.p, nl.p, nr.p, bl, br, dasg.p);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_greedy_walk<TC, false>), dim3(1), dim3(64), 0, s, stream.p, gpos.p, ord.p, (int32_t)n, (int32_t)N,
                                   (int32_t)K, c0.p, cst.p, nl.p, nr.p, bl, br, dasg.p);
            CP_HIP(hipGetLastError());
        }
        CP_HIP(hipMemcpyAsync(asg_out, dasg.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (order_out) {
            hipLaunchKernelGGL(k_greedy_emit_order, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, ord.p, dord.p, n);
            CP_HIP(hipGetLastError());
            CP_HIP(hipMemcpyAsync(order_out, dord.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        }
    }
    if (cst_out) CP_HIP(hipMemcpyAsync(cst_out, cst.p, sizeof(TC) * Ks, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    return CP_OK;
}

}  // namespace cpk

using namespace cpk;

extern "C" int32_t cp_partition_magnetic(cp_csr_t A, int64_t K, const cp_rowpart_t *Pi, int64_t seed, const int64_t *draws, int64_t *asg_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && (asg_out || A->n == 0), CP_EINVAL, "null argument");
        CP_REQUIRE(K >= 1, CP_EINVAL, "cp_partition_magnetic: K must be at least 1");
        CP_HIP(hipSetDevice(A->device));
        hipStream_t s = A->stream;
        const int64_t n = A->n;
        DBuf<int32_t> owner;
        map_owner(A, Pi, owner, s);
        if (n <= 0) return CP_OK;
        DBuf<int64_t> dd, dasg((size_t)n);
        if (draws) {
            DBuf<int32_t> bad(1);
            dd.alloc((size_t)n);
            CP_HIP(hipMemcpyAsync(dd.p, draws, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
            CP_HIP(hipMemsetAsync(bad.p, 0, sizeof(int32_t), s));
            hipLaunchKernelGGL(k_map_draws_check, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, dd.p, n, bad.p);
            CP_HIP(hipGetLastError());
            int32_t hb = 0;
            CP_HIP(hipMemcpyAsync(&hb, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            CP_REQUIRE(!hb, CP_EINVAL, "cp_partition_magnetic: a draw is negative");
        }
        {
            ProfScope ps(PROF_MAGNETIC, s, 28.0 * (double)n);
            hipLaunchKernelGGL(k_magnetic, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, A->pos.p, A->row.p, owner.p, draws ? dd.p : (const int64_t *)nullptr,
                               stream_key(seed, 1), n, K, dasg.p);
            CP_HIP(hipGetLastError());
        }
        CP_HIP(hipMemcpyAsync(asg_out, dasg.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        prof_collect();
        return CP_OK;
    });
}

extern "C" int32_t cp_partition_greedy_bottleneck(cp_csr_t A, int64_t K, const cp_model_t *model, const cp_rowpart_t *Pi, int64_t seed,
                                                  const int64_t *order, int64_t *asg_out, int64_t *order_out, int64_t *cst_i64, double *cst_f64)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && model && (asg_out || A->n == 0), CP_EINVAL, "null argument");
        CP_REFUSE_ENV(model, "GreedyBottleneckPartitioner");
        CP_REQUIRE(model->kind == CP_MODEL_SECONDARY && (model->dtype == CP_I64 || model->dtype == CP_F64), CP_EUNSUPPORTED,
                   "cp_partition_greedy_bottleneck: the reference has a method for the secondary connectivity model only");
        CP_REQUIRE(K >= 1 && K < ((int64_t)1 << 31), CP_EINVAL, "cp_partition_greedy_bottleneck: K must be at least 1");
        CP_REQUIRE(Pi && Pi->K == K, CP_EINVAL, "cp_partition_greedy_bottleneck: Pi must be a partition of the rows into K parts");
        CP_HIP(hipSetDevice(A->device));
        return with_cost_type(model->dtype, [&](auto tag) {
            using TC = decltype(tag);
            return run_greedy<TC>(A, K, model, Pi, seed, order, asg_out, order_out, pick<TC>(cst_i64, cst_f64));
        });
    });
}
