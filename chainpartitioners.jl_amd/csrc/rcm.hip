// rcm.hip -- the reordering layer on the device: cp_rcm (symrcm / rctrcm / permute_plaid of the reference's
// src/CuthillMcKeePermuter.jl:7-265) and cp_csr_permute (A[perm(sigma), perm(tau)], src/PermutingPartitioner.jl:12).
//
// The reference walks a queue vertex by vertex and sorts the children of every vertex by degree with a stable insertion sort
// (:60-77).  The children come in ascending index order, so a vertex's place in the queue is fixed by the key
//     (queue position of its parent, degree, index),        parent = the earliest-queued vertex whose column holds it,
// and a new tree starts at the unvisited vertex of least (degree, index) (tests/rcm_model.py holds the two forms against each
// other).  The queue positions of one BFS level are contiguous, so a level is expanded as a whole:
//     mark     every frontier vertex u at position p does atomicMin(par[v], p) for the unvisited v of its column
//     collect  an edge (u, v) with par[v] == p contributes v -- exactly once, a column holds a row at most once
//     order    the collected vertices by (par, degree, v): the keys are unique, the order does not depend on scheduling
//     commit   append to the queue, mark visited (visited is written here only: mark and collect read a stable value)
// Two regimes, chosen per level by the host from the level's size:
//     wide     grid kernels for mark / collect, rocprim radix sorts for the order, one small readback per level
//     narrow   k_rcm_walk: ONE workgroup walks level after level in one launch, the candidates sorted in LDS; it starts the next
//              tree itself when the queue runs dry and returns when the level in hand exceeds its node or edge capacity (that
//              level is left unexpanded, the wide regime takes it) or when the queue is full.  No grid barrier, no co-residency.
#include "csr.hpp"
#include <rocprim/rocprim.hpp>
#include <memory>

namespace cpk {

int64_t g_opt_rcm_narrow = 256;          // levels of at most this many vertices go to the walker (0: never; clamped to WALK_NODES)

constexpr int WALK_T = 256;              // threads of the walker's workgroup
constexpr int WALK_NODES = 1024;         // largest frontier it expands
constexpr int WALK_EDGES = 4096;         // largest number of column entries of a frontier = room for its candidates in LDS
constexpr int WALK_PER = WALK_EDGES / WALK_T;
enum { ST_LO = 0, ST_HI, ST_KSTART, ST_TREES, ST_LEVELS, ST_FLAG, ST_CNT, ST_N };
enum { WALK_DONE = 0, WALK_OVERFLOW = 1, WALK_CORRUPT = 2 };

// ------------------------------------------------------------------ graph construction
__global__ void k_rcm_deg(const int32_t *__restrict__ pos, uint32_t *__restrict__ key, uint32_t *__restrict__ val, int64_t V)
{
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) { key[v] = (uint32_t)(pos[v + 1] - pos[v]); val[v] = (uint32_t)v; }
}

// the (m + n)-vertex bipartite graph: rows 0 .. m-1 with neighbours m + j from the adjoint, columns m .. m+n-1 with neighbours i
__global__ void k_rcm_bip_pos(const int64_t *__restrict__ tpos, const int64_t *__restrict__ apos, int32_t *__restrict__ pos, int64_t m,
                              int64_t n, int64_t N)
{
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > m + n) return;
    pos[v] = (int32_t)(v < m ? tpos[v] : N + apos[v - m]);
}
__global__ void k_rcm_bip_adj(const int32_t *__restrict__ trow, const int32_t *__restrict__ arow, int32_t *__restrict__ adj, int64_t m, int64_t N)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    adj[q] = (int32_t)(m + trow[q]);
    adj[N + q] = arow[q];
}

__global__ void k_rcm_differs(const int64_t *__restrict__ pa, const int64_t *__restrict__ pb, int64_t n1, const int32_t *__restrict__ ra,
                              const int32_t *__restrict__ rb, int64_t N, int32_t *__restrict__ differs)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((i < n1 && pa[i] != pb[i]) || (i < N && ra[i] != rb[i])) *differs = 1;
}

// ------------------------------------------------------------------ tree starts
// the first k >= k0 with ord[k] unvisited, V if there is none (whole workgroup of WALK_T threads; k0 grows by WALK_T per trip)
__device__ __forceinline__ int32_t rcm_find_start(const int32_t *__restrict__ ord, const uint8_t *visited, int32_t k0, int32_t V, int32_t *s_min)
{
    for (int64_t k = k0; ; k += WALK_T) {
        if (threadIdx.x == 0) *s_min = V;
        __syncthreads();
        const int64_t mine = k + threadIdx.x;
        if (mine < V && !visited[ord[mine]]) atomicMin(s_min, (int32_t)mine);
        __syncthreads();
        const int32_t f = *s_min;
        __syncthreads();
        if (f < V || k + WALK_T >= V) return f;
    }
}

// wide regime: the queue is dry at position hi -- start the next tree there
__global__ void __launch_bounds__(WALK_T) k_rcm_start(const int32_t *__restrict__ ord, int32_t *__restrict__ queue, uint8_t *visited,
                                                      int32_t *__restrict__ st, int32_t V, int32_t hi)
{
    __shared__ int32_t s_min;
    const int32_t k = rcm_find_start(ord, visited, st[ST_KSTART], V, &s_min);
    if (threadIdx.x != 0) return;
    if (k >= V || hi >= V) { st[ST_FLAG] = WALK_CORRUPT; return; }
    const int32_t v = ord[k];
    queue[hi] = v;
    visited[v] = 1;
    st[ST_KSTART] = k + 1;
}

// ------------------------------------------------------------------ narrow regime
// largest i in [0, F) with pre[i] <= e (pre[0] == 0 <= e)
__device__ __forceinline__ int32_t rcm_owner(const int32_t *pre, int32_t F, int32_t e)
{
    int32_t lo = 0, hi = F;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup, level after level from the level [lo, hi) of the queue.  Every quantity a branch or a barrier depends on (lo, hi,
// the level's totals, the candidate count) is the same in all threads.  The loop runs at most 2 V + 2 times -- every trip starts a
// tree, appends a vertex or empties the frontier -- and every overflow leaves it: nothing here waits for another workgroup.
// par is only touched with workgroup-scope atomics: a vertex marked in a level is committed in that level, so no other launch ever
// reads what this one wrote there.
__global__ void __launch_bounds__(WALK_T) k_rcm_walk(const int32_t *__restrict__ pos, const int32_t *__restrict__ adj, const int32_t *__restrict__ ord,
                                                     int32_t *queue, uint8_t *visited, uint32_t *par, int32_t *__restrict__ st, int32_t V, int32_t lo,
                                                     int32_t hi, int32_t node_cap)
{
    __shared__ uint64_t skey[WALK_EDGES];
    __shared__ uint32_t sval[WALK_EDGES];
    __shared__ int32_t spre[WALK_NODES + 1], sbase[WALK_NODES];
    __shared__ int32_t s_wsum[WALK_T / 64], s_cnt, s_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t kstart = st[ST_KSTART], trees = 0, levels = 0, flag = WALK_DONE;
    for (int64_t trip = 0; trip < 2 * (int64_t)V + 2 && hi < V; trip++) {
        if (lo == hi) {                                             // the queue ran dry: the next tree starts at ord[k_start ..]'s first unvisited vertex
            const int32_t k = rcm_find_start(ord, visited, kstart, V, &s_min);
            if (k >= V) { flag = WALK_CORRUPT; break; }
            if (tid == 0) { const int32_t v = ord[k]; queue[hi] = v; visited[v] = 1; }
            kstart = k + 1; hi++; trees++;
            __syncthreads();
            continue;
        }
        const int32_t F = hi - lo;
        if (F > node_cap) { flag = WALK_OVERFLOW; break; }
        // column starts and the prefix sum of the column lengths (clamped: only "more than WALK_EDGES" matters beyond it)
        int32_t d[WALK_NODES / WALK_T], sum = 0;
#pragma unroll
        for (int c = 0; c < WALK_NODES / WALK_T; c++) {
            const int32_t i = tid * (WALK_NODES / WALK_T) + c;
            d[c] = 0;
            if (i < F) {
                const int32_t u = queue[lo + i], b = pos[u], len = pos[u + 1] - b;
                sbase[i] = b;
                d[c] = len > WALK_EDGES + 1 ? WALK_EDGES + 1 : len;
            }
            sum += d[c];
        }
        int32_t inc = sum;
        for (int o = 1; o < 64; o <<= 1) { const int32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        int32_t woff = 0, total = 0;
        for (int w = 0; w < WALK_T / 64; w++) { if (w < wave) woff += s_wsum[w]; total += s_wsum[w]; }
        if (total > WALK_EDGES) { flag = WALK_OVERFLOW; break; }
        int32_t run = woff + inc - sum;
#pragma unroll
        for (int c = 0; c < WALK_NODES / WALK_T; c++) {
            const int32_t i = tid * (WALK_NODES / WALK_T) + c;
            if (i < F) spre[i] = run;
            run += d[c];
        }
        if (tid == 0) { spre[F] = total; s_cnt = 0; }
        __syncthreads();
        // mark: entry e of the level belongs to frontier vertex pi[c] at queue position lo + pi[c]
        int32_t vv[WALK_PER], pi[WALK_PER];
#pragma unroll
        for (int c = 0; c < WALK_PER; c++) {
            const int32_t e = tid + c * WALK_T;
            vv[c] = -1;
            if (e < total) {
                const int32_t i = rcm_owner(spre, F, e), v = adj[sbase[i] + (e - spre[i])];
                pi[c] = i;
                if (!visited[v]) {
                    vv[c] = v;
                    __hip_atomic_fetch_min(&par[v], (uint32_t)(lo + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // collect
#pragma unroll
        for (int c = 0; c < WALK_PER; c++) {
            const int32_t v = vv[c];
            if (v >= 0 && __hip_atomic_load(&par[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == (uint32_t)(lo + pi[c])) {
                const int32_t slot = atomicAdd(&s_cnt, 1);          // (at most `total` <= WALK_EDGES of them)
                skey[slot] = ((uint64_t)pi[c] << 31) | (uint64_t)(uint32_t)(pos[v + 1] - pos[v]);
                sval[slot] = (uint32_t)v;
            }
        }
        __syncthreads();
        const int32_t C = s_cnt;
        levels++;
        if (C == 0) { lo = hi; continue; }
        if ((int64_t)hi + C > V) { flag = WALK_CORRUPT; break; }  // (a column that holds an index twice: refuse, never write past the queue)
        if (C <= WALK_T) {                                          // rank sort: one candidate per thread
            if (tid < C) {
                const uint64_t k = skey[tid];
                const uint32_t v = sval[tid];
                int32_t r = 0;
                for (int32_t j = 0; j < C; j++) { const uint64_t kj = skey[j]; r += (kj < k) || (kj == k && sval[j] < v); }
                queue[hi + r] = (int32_t)v;
                visited[v] = 1;
            }
        } else {                                                    // bitonic sort of (key, vertex) over the next power of two
            int32_t P = 512;
            while (P < C) P <<= 1;
            for (int32_t x = C + tid; x < P; x += WALK_T) { skey[x] = ~0ull; sval[x] = ~0u; }
            __syncthreads();
            for (int32_t k = 2; k <= P; k <<= 1)
                for (int32_t j = k >> 1; j > 0; j >>= 1) {
                    for (int32_t x = tid; x < P; x += WALK_T) {
                        const int32_t y = x ^ j;
                        if (y > x) {
                            const uint64_t kx = skey[x], ky = skey[y];
                            const uint32_t vx = sval[x], vy = sval[y];
                            const bool gt = kx > ky || (kx == ky && vx > vy);
                            if (gt == ((x & k) == 0)) { skey[x] = ky; skey[y] = kx; sval[x] = vy; sval[y] = vx; }
                        }
                    }
                    __syncthreads();
                }
            for (int32_t x = tid; x < C; x += WALK_T) { const uint32_t v = sval[x]; queue[hi + x] = (int32_t)v; visited[v] = 1; }
        }
        __syncthreads();
        lo = hi; hi += C;
    }
    if (tid == 0) {
        st[ST_LO] = lo; st[ST_HI] = hi; st[ST_KSTART] = kstart; st[ST_FLAG] = flag;
        st[ST_TREES] += trees; st[ST_LEVELS] += levels;
    }
}

// ------------------------------------------------------------------ wide regime
// one wave per frontier vertex; collect == 0: mark, else: collect into cand[0 .. cap) (the count goes on beyond cap: the host refuses)
__global__ void __launch_bounds__(256) k_rcm_expand(const int32_t *__restrict__ pos, const int32_t *__restrict__ adj, const int32_t *__restrict__ queue,
                                                    const uint8_t *__restrict__ visited, uint32_t *par, int32_t lo, int32_t F, int32_t collect,
                                                    uint32_t *__restrict__ cand, int32_t *st, int32_t cap)
{
    const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= F) return;
    const int lane = threadIdx.x & 63;
    const int32_t u = queue[lo + w], end = pos[u + 1];
    const uint32_t p = (uint32_t)(lo + w);
    for (int64_t base = pos[u]; base < end; base += 64) {
        const int64_t q = base + lane;
        int32_t v = -1;
        if (q < end) { v = adj[q]; if (visited[v]) v = -1; }
        if (!collect) {
            if (v >= 0) atomicMin(&par[v], p);
            continue;
        }
        const bool take = v >= 0 && par[v] == p;
        const unsigned long long mask = __ballot(take);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int32_t slot0 = 0;
        if (lane == leader) slot0 = atomicAdd(&st[ST_CNT], __popcll(mask));
        slot0 = __shfl(slot0, leader);
        const int64_t slot = (int64_t)slot0 + __popcll(mask & ((1ull << lane) - 1ull));
        if (take && slot0 >= 0 && slot < cap) cand[slot] = (uint32_t)v;
    }
}

__global__ void k_rcm_keys(const int32_t *__restrict__ pos, const uint32_t *__restrict__ par, const uint32_t *__restrict__ cand, uint64_t *__restrict__ key,
                           int32_t lo, int32_t cnt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t v = cand[i];
    key[i] = ((uint64_t)(par[v] - (uint32_t)lo) << 31) | (uint64_t)(uint32_t)(pos[v + 1] - pos[v]);
}

__global__ void k_rcm_commit(const uint32_t *__restrict__ sorted, int32_t *__restrict__ queue, uint8_t *__restrict__ visited, int32_t hi, int32_t cnt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t v = sorted[i];
    queue[hi + i] = (int32_t)v;
    visited[v] = 1;
}

// ------------------------------------------------------------------ results
__global__ void k_rcm_emit(const int32_t *__restrict__ queue, int64_t *__restrict__ out, int64_t V, int32_t reverse)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < V) out[reverse ? V - 1 - k : k] = (int64_t)queue[k] + 1;
}
__global__ void k_rcm_isrow(const int32_t *__restrict__ queue, int32_t *__restrict__ flag, int64_t V, int64_t m)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < V) flag[k] = queue[k] < m;
}
// permute_plaid's deal (CuthillMcKeePermuter.jl:237-261): the rows and the columns of the queue, each in queue order, backwards if reverse
__global__ void k_rcm_deal(const int32_t *__restrict__ queue, const int64_t *__restrict__ rrank, int64_t *__restrict__ iprm, int64_t *__restrict__ jprm,
                           int64_t V, int64_t m, int64_t n, int32_t reverse)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    const int64_t v = queue[k], r = rrank[k];
    if (v < m) { if (r < m) iprm[reverse ? m - 1 - r : r] = v + 1; }
    else { const int64_t c = k - r; if (c < n) jprm[reverse ? n - 1 - c : c] = v - m + 1; }
}

struct RcmStats { int64_t path = 0, trees = 0, levels = 0, wide = 0, walks = 0, readbacks = 0; };

template <typename K>
static void rcm_sort_pairs(DBuf<char> &tmp, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t cnt, unsigned end_bit, hipStream_t s)
{
    size_t bytes = 0;
    CP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, cnt, 0u, end_bit, s));
    tmp.ensure(bytes > 0 ? bytes : 1);
    CP_HIP(rocprim::radix_sort_pairs((void *)tmp.p, bytes, kin, kout, vin, vout, cnt, 0u, end_bit, s));
}

static unsigned bits_of(uint64_t x) { unsigned b = 1; while (b < 63 && ((uint64_t)1 << b) <= x) b++; return b; }

// the queue of the graph (pos, adj) with V vertices -> queue[0 .. V), 0-based
static void rcm_run(const int32_t *pos, const int32_t *adj, int32_t V, int32_t *queue, hipStream_t s, RcmStats &out)
{
    if (V <= 0) return;
    const size_t Vs = (size_t)V;
    DBuf<uint32_t> k32a(Vs), k32b(Vs), v32a(Vs), ord(Vs), cand(Vs), cand_s(Vs), sorted(Vs);
    DBuf<uint64_t> k64a(Vs), k64b(Vs);
    DBuf<uint8_t> visited(Vs);
    DBuf<uint32_t> par(Vs);
    DBuf<int32_t> st(ST_N);
    DBuf<char> tmp;
    const unsigned vbits = bits_of((uint64_t)V);
    // ord: one stable sort of the vertices by degree (CuthillMcKeePermuter.jl:14-29)
    hipLaunchKernelGGL(k_rcm_deg, dim3((unsigned)cdiv(V, 256)), dim3(256), 0, s, pos, k32a.p, v32a.p, (int64_t)V);
    rcm_sort_pairs<uint32_t>(tmp, k32a.p, k32b.p, v32a.p, ord.p, Vs, 32u, s);
    CP_HIP(hipMemsetAsync(visited.p, 0, visited.bytes(), s));
    CP_HIP(hipMemsetAsync(par.p, 0xFF, par.bytes(), s));
    CP_HIP(hipMemsetAsync(queue, 0, sizeof(int32_t) * Vs, s));
    CP_HIP(hipMemsetAsync(st.p, 0, st.bytes(), s));
    const int32_t *d_ord = (const int32_t *)ord.p;
    const int32_t lim = (int32_t)(g_opt_rcm_narrow < 0 ? 0 : g_opt_rcm_narrow > WALK_NODES ? WALK_NODES : g_opt_rcm_narrow);
    int32_t h[ST_N] = {0};
    auto readback = [&]() {
        CP_HIP(hipMemcpyAsync(h, st.p, sizeof(h), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        out.readbacks++;
        CP_REQUIRE(h[ST_FLAG] != WALK_CORRUPT, CP_EINVAL, "cp_rcm: malformed pattern (a column holds an index twice)");
    };
    int32_t lo = 0, hi = 0;
    int64_t host_trees = 0;
    bool skip_walk = false;
    while (hi < V) {
        const int32_t F = hi - lo;
        if (lim > 0 && F <= lim && !skip_walk) {
            hipLaunchKernelGGL(k_rcm_walk, dim3(1), dim3(WALK_T), 0, s, pos, adj, d_ord, queue, visited.p, par.p, st.p, V, lo, hi, lim);
            CP_HIP(hipGetLastError());
            readback();
            out.walks++;
            CP_REQUIRE(h[ST_LO] >= lo && h[ST_HI] >= hi && h[ST_LO] <= h[ST_HI] && h[ST_HI] <= V, CP_EINTERNAL, "cp_rcm: the walker left an inconsistent state");
            lo = h[ST_LO]; hi = h[ST_HI];
            CP_REQUIRE(hi >= V || h[ST_FLAG] == WALK_OVERFLOW, CP_EINTERNAL, "cp_rcm: the walker stopped early");
            skip_walk = true;                                       // the level in hand is beyond its capacity: one wide level
            continue;
        }
        skip_walk = false;
        if (F == 0) {
            hipLaunchKernelGGL(k_rcm_start, dim3(1), dim3(WALK_T), 0, s, d_ord, queue, visited.p, st.p, V, hi);
            CP_HIP(hipGetLastError());
            lo = hi; hi++; host_trees++;
            continue;
        }
        CP_HIP(hipMemsetAsync(st.p + ST_CNT, 0, sizeof(int32_t), s));
        const unsigned blocks = (unsigned)cdiv((int64_t)F * 64, 256);
        for (int32_t collect = 0; collect < 2; collect++)
            hipLaunchKernelGGL(k_rcm_expand, dim3(blocks), dim3(256), 0, s, pos, adj, queue, visited.p, par.p, lo, F, collect, cand.p, st.p, V);
        CP_HIP(hipGetLastError());
        readback();
        out.wide++; out.levels++;
        const int32_t cnt = h[ST_CNT];
        CP_REQUIRE(cnt >= 0 && cnt <= V - hi, CP_EINVAL, "cp_rcm: malformed pattern (a column holds an index twice)");
        if (cnt > 0) {
            size_t bytes = 0;
            CP_HIP(rocprim::radix_sort_keys(nullptr, bytes, cand.p, cand_s.p, (size_t)cnt, 0u, vbits, s));
            tmp.ensure(bytes > 0 ? bytes : 1);
            CP_HIP(rocprim::radix_sort_keys((void *)tmp.p, bytes, cand.p, cand_s.p, (size_t)cnt, 0u, vbits, s));
            hipLaunchKernelGGL(k_rcm_keys, dim3((unsigned)cdiv(cnt, 256)), dim3(256), 0, s, pos, par.p, cand_s.p, k64a.p, lo, cnt);
            rcm_sort_pairs<uint64_t>(tmp, k64a.p, k64b.p, cand_s.p, sorted.p, (size_t)cnt, 31u + bits_of((uint64_t)F), s);
            hipLaunchKernelGGL(k_rcm_commit, dim3((unsigned)cdiv(cnt, 256)), dim3(256), 0, s, sorted.p, queue, visited.p, hi, cnt);
            CP_HIP(hipGetLastError());
        }
        lo = hi; hi += cnt;
    }
    readback();                                                     // the walker's counters; a corrupt flag of the last tree start
    out.trees = host_trees + h[ST_TREES];
    out.levels += h[ST_LEVELS];
}

// ------------------------------------------------------------------ A[rowprm, colprm]
// prm: 1-based int64 -> 0-based int32, refused unless every value of 1 .. len occurs once (mark array: no access out of range)
__global__ void k_perm_check(const int64_t *__restrict__ prm, int32_t *__restrict__ out, int32_t *mark, int64_t len, int32_t *__restrict__ bad)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const int64_t p = prm[i];
    if (p < 1 || p > len) { *bad = 1; out[i] = 0; return; }
    if (atomicExch(&mark[p - 1], 1)) *bad = 1;
    out[i] = (int32_t)(p - 1);
}
__global__ void k_gather_len(const int64_t *__restrict__ pos, const int32_t *__restrict__ prm, int32_t *__restrict__ len, int64_t n)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t c = prm ? prm[j] : j;
    len[j] = (int32_t)(pos[c + 1] - pos[c]);
}
// one thread per entry of the result: its column by binary search (as k_fill_col), its source in the gathered column
__global__ void k_gather_rows(const int64_t *__restrict__ apos, const int32_t *__restrict__ arow, const int32_t *__restrict__ prm,
                              const int64_t *__restrict__ bpos, int32_t *__restrict__ brow, int64_t n, int64_t N)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (bpos[mid] <= q) lo = mid; else hi = mid;
    }
    const int64_t c = prm ? prm[lo] : lo;
    brow[q] = arow[apos[c] + (q - bpos[lo])];
}

static void perm_upload(const int64_t *h_prm, int64_t len, DBuf<int32_t> &out, hipStream_t s, const char *what)
{
    const size_t L = (size_t)(len > 0 ? len : 1);
    DBuf<int64_t> d(L);
    DBuf<int32_t> mark(L), bad(1);
    out.alloc(L);
    if (len <= 0) return;
    CP_HIP(hipMemcpyAsync(d.p, h_prm, sizeof(int64_t) * (size_t)len, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemsetAsync(mark.p, 0, mark.bytes(), s));
    CP_HIP(hipMemsetAsync(bad.p, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_perm_check, dim3((unsigned)cdiv(len, 256)), dim3(256), 0, s, d.p, out.p, mark.p, len, bad.p);
    CP_HIP(hipGetLastError());
    int32_t hb = 0;
    CP_HIP(hipMemcpyAsync(&hb, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    CP_REQUIRE(!hb, CP_EINVAL, what);
}

// B = A[:, prm] (prm 0-based on the device, nullptr: the identity) on stream s: lengths -> scan -> copy; the rows stay sorted
static void gather_columns(const cp_csr_s *A, const int32_t *prm, cp_csr_s *B, hipStream_t s)
{
    const int64_t n = A->n, N = A->N;
    B->m = A->m; B->n = n; B->N = N;
    B->pos.alloc((size_t)n + 1);
    B->row.alloc((size_t)(N > 0 ? N : 1));
    DBuf<int32_t> len((size_t)(n > 0 ? n : 1));
    DBuf<int64_t> scratch;
    if (n > 0) hipLaunchKernelGGL(k_gather_len, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, A->pos.p, prm, len.p, n);
    exclusive_scan_i32(len.p, B->pos.p, n, scratch, s);
    if (N > 0 && n > 0)
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, A->pos.p, A->row.p, prm, B->pos.p, B->row.p, n, N);
    CP_HIP(hipGetLastError());
    CP_HIP(hipStreamSynchronize(s));
}

static std::unique_ptr<cp_csr_s> temp_handle(const cp_csr_s *A)
{
    std::unique_ptr<cp_csr_s> T(new cp_csr_s());
    T->device = A->device; T->stream = A->stream; T->own_stream = false;      // (borrowed: the destructor leaves the stream alone)
    return T;
}

}  // namespace cpk

using namespace cpk;

extern "C" int32_t cp_rcm(cp_csr_t A, cp_csr_t adj, int32_t mode, int32_t reverse, int64_t *rowprm_out, int64_t *colprm_out, int64_t *stats_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && rowprm_out && colprm_out, CP_EINVAL, "null argument");
        CP_REQUIRE(mode >= 0 && mode <= 2, CP_EINVAL, "cp_rcm: mode must be 0 (check symmetry), 1 (assume symmetry) or 2 (bipartite)");
        const int64_t m = A->m, n = A->n, N = A->N;
        CP_REQUIRE(mode != 1 || m == n, CP_EINVAL, "cp_rcm: assumesymmetry needs a square pattern");
        CP_REQUIRE(!adj || (adj->m == n && adj->n == m && adj->N == N && adj->device == A->device), CP_EINVAL,
                   "cp_rcm: the adjoint handle does not have the adjoint's shape");
        CP_HIP(hipSetDevice(A->device));
        hipStream_t s = A->stream;
        RcmStats stt;
        std::unique_ptr<cp_csr_s> Town;
        cp_csr_s *T = adj;
        if (mode != 1 && !T) { Town = temp_handle(A); csr_adjoint(A, Town.get()); T = Town.get(); }
        bool sym = mode == 1;
        if (mode == 0 && m == n) {                                  // issymmetric(pattern(A)): A and its adjoint hold the same arrays
            DBuf<int32_t> differs(1);
            CP_HIP(hipMemsetAsync(differs.p, 0, sizeof(int32_t), s));
            const int64_t mx = n + 1 > N ? n + 1 : N;
            hipLaunchKernelGGL(k_rcm_differs, dim3((unsigned)cdiv(mx, 256)), dim3(256), 0, s, A->pos.p, T->pos.p, n + 1, A->row.p, T->row.p, N, differs.p);
            CP_HIP(hipGetLastError());
            int32_t hd = 0;
            CP_HIP(hipMemcpyAsync(&hd, differs.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            sym = !hd;
        }
        if (sym) {
            stt.path = 1;
            DBuf<int32_t> pos((size_t)n + 1), queue((size_t)(n > 0 ? n : 1));
            DBuf<int64_t> prm((size_t)(n > 0 ? n : 1));
            hipLaunchKernelGGL(k_narrow, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, A->pos.p, pos.p, n + 1);
            rcm_run(pos.p, A->row.p, (int32_t)n, queue.p, s, stt);
            if (n > 0) {
                hipLaunchKernelGGL(k_rcm_emit, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, queue.p, prm.p, n, reverse);
                CP_HIP(hipGetLastError());
                CP_HIP(hipMemcpyAsync(rowprm_out, prm.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
                CP_HIP(hipMemcpyAsync(colprm_out, prm.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
            }
        } else {
            stt.path = 2;
            const int64_t V = m + n;
            CP_REQUIRE(V < ((int64_t)1 << 31) && 2 * N < ((int64_t)1 << 31), CP_EUNSUPPORTED,
                       "cp_rcm: the bipartite walk keeps 32-bit vertex and edge ids (m + n and 2 nnz must stay below 2^31)");
            DBuf<int32_t> pos((size_t)V + 1), gadj((size_t)(N > 0 ? 2 * N : 1)), queue((size_t)(V > 0 ? V : 1)), isrow((size_t)(V > 0 ? V : 1));
            DBuf<int64_t> rrank((size_t)V + 1), scratch, iprm((size_t)(m > 0 ? m : 1)), jprm((size_t)(n > 0 ? n : 1));
            hipLaunchKernelGGL(k_rcm_bip_pos, dim3((unsigned)cdiv(V + 1, 256)), dim3(256), 0, s, T->pos.p, A->pos.p, pos.p, m, n, N);
            if (N > 0) hipLaunchKernelGGL(k_rcm_bip_adj, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, T->row.p, A->row.p, gadj.p, m, N);
            CP_HIP(hipGetLastError());
            rcm_run(pos.p, gadj.p, (int32_t)V, queue.p, s, stt);
            if (V > 0) {
                hipLaunchKernelGGL(k_rcm_isrow, dim3((unsigned)cdiv(V, 256)), dim3(256), 0, s, queue.p, isrow.p, V, m);
                exclusive_scan_i32(isrow.p, rrank.p, V, scratch, s);
                hipLaunchKernelGGL(k_rcm_deal, dim3((unsigned)cdiv(V, 256)), dim3(256), 0, s, queue.p, rrank.p, iprm.p, jprm.p, V, m, n, reverse);
                CP_HIP(hipGetLastError());
                if (m > 0) CP_HIP(hipMemcpyAsync(rowprm_out, iprm.p, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, s));
                if (n > 0) CP_HIP(hipMemcpyAsync(colprm_out, jprm.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
            }
        }
        CP_HIP(hipStreamSynchronize(s));
        if (stats_out) {
            stats_out[0] = stt.path; stats_out[1] = stt.trees; stats_out[2] = stt.levels;
            stats_out[3] = stt.wide; stats_out[4] = stt.walks; stats_out[5] = stt.readbacks;
        }
        return CP_OK;
    });
}

extern "C" int32_t cp_csr_permute(cp_csr_t A, const int64_t *rowprm, const int64_t *colprm, cp_csr_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out, CP_EINVAL, "null argument");
        CP_HIP(hipSetDevice(A->device));
        hipStream_t s = A->stream;
        DBuf<int32_t> rp, cq;
        if (rowprm) perm_upload(rowprm, A->m, rp, s, "cp_csr_permute: rowprm is not a permutation of 1 .. m");
        if (colprm) perm_upload(colprm, A->n, cq, s, "cp_csr_permute: colprm is not a permutation of 1 .. n");
        std::unique_ptr<cp_csr_s> B(new cp_csr_s());
        B->device = A->device;
        CP_HIP(hipStreamCreate(&B->stream));
        B->own_stream = true;
        if (!rowprm) {
            gather_columns(A, colprm ? cq.p : nullptr, B.get(), s);
        } else {
            // the rows are the columns of the adjoint: gather there, and the counting-sort transpose back re-sorts every column
            std::unique_ptr<cp_csr_s> C, T1 = temp_handle(A), T2 = temp_handle(A);
            cp_csr_s *src = A;
            if (colprm) { C = temp_handle(A); gather_columns(A, cq.p, C.get(), s); src = C.get(); }
            csr_adjoint(src, T1.get());
            gather_columns(T1.get(), rp.p, T2.get(), s);
            csr_adjoint(T2.get(), B.get());
        }
        *out = B.release();
        return CP_OK;
    });
}
