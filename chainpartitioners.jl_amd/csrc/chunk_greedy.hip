// chunk_greedy.hip -- the greedy chunkers StrictChunker(w_max) and OverlapChunker(rho, w_max) in their parallel forms
// (DESIGN.md section 5c).  The reference writes both as one sweep over the columns (StrictChunker.jl:5-54, OverlapChunker.jl:6-75);
// here
//   strict : neq[j'] = (column j' differs from column j' - 1), start(j') = the last flagged position <= j' (a max-scan), a split
//            falls at j' iff neq[j'] or (j' - start(j')) mod w_max == 0;
//   overlap: whether j' splits depends on the part's first column j and on j' alone, so next[j] = the first j' that fires is
//            computed for EVERY start j at once, and the split vector is the orbit 1 -> next[1] -> ... -> n + 1, marked by pointer
//            doubling over a double-buffered jump array.
// Both end in the same tail: flags -> exclusive scan -> spl (1-based) and K; n_nets[k] on request from the link array prev.
// Columns are 0-based below (column p is the reference's j = p + 1; position n stands for its n + 1).
#include "csr.hpp"
#include "dp.hpp"

namespace cpk {

int64_t g_overlap_isect = 0;

// ------------------------------------------------------------------ strict: neq
// One wave per 64 columns.  The lanes first compare the lengths of their column and its left neighbour; the entries of the 64 columns
// are then streamed 64 at a time (coalesced), every lane finds the column of its entry in the wave's LDS copy of pos and, where the
// lengths agree, compares its row with the row len entries to the left -- the same place in the neighbour column.  So a row index is
// read at most twice, and not at all where the lengths differ.
__global__ void __launch_bounds__(64) k_col_neq(const int64_t *__restrict__ pos, const int32_t *__restrict__ row, int64_t n, int32_t *__restrict__ neq)
{
    __shared__ int32_t srel[65];        // pos of the wave's columns, relative to the first
    __shared__ int32_t slen[64];        // the common length where column and neighbour agree in length (and have entries), else 0
    __shared__ int32_t sflag[64];
    const int lane = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    const int cnt = (int)(n - c0 < 64 ? n - c0 : 64);
    const int64_t base = pos[c0];
    for (int i = lane; i <= cnt; i += 64) srel[i] = (int32_t)(pos[c0 + i] - base);
    if (lane < cnt) {
        const int64_t j = c0 + lane;
        const int64_t len = pos[j + 1] - pos[j], plen = j > 0 ? pos[j] - pos[j - 1] : -1;
        sflag[lane] = len != plen;
        slen[lane] = len == plen ? (int32_t)len : 0;
    }
    __syncthreads();
    const int32_t total = srel[cnt];
    for (int32_t e0 = 0; e0 < total; e0 += 64) {
        const int32_t e = e0 + lane;
        if (e < total) {
            int lo = 0, hi = cnt;                    // the column i with srel[i] <= e < srel[i + 1]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (srel[mid] <= e) lo = mid; else hi = mid; }
            const int32_t L = slen[lo];
            if (L > 0) {
                const int64_t q = base + e;
                if (row[q] != row[q - L]) sflag[lo] = 1;
            }
        }
    }
    __syncthreads();
    if (lane < cnt) neq[c0 + lane] = sflag[lane];
}

// split flags of StrictChunker in place over neq: flag[p] = neq[p] or (w_max >= 1 and (p - start[p]) mod w_max == 0)
__global__ void k_strict_flags(int32_t *__restrict__ flag, const int32_t *__restrict__ start, int64_t n, int64_t w_max)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (!flag[p] && w_max >= 1 && ((p - (int64_t)start[p]) % w_max) == 0) flag[p] = 1;
}

// ------------------------------------------------------------------ overlap: next
// G lanes per start column p; its candidates p + 1, p + 2, ... are taken in order until one fires.  A start column of at most G
// entries is held one entry per lane and a candidate's rows are looked up by rotating it through the group (shuffles); a longer one
// is binary-searched in place (it stays in the L1 while its candidates stream).  cc' = popcount of the group's ballot bits.  The test
// is the reference's Float64 expression as written (OverlapChunker.jl:57): Float64(cc') < rho * Float64(min(c, c')), with c the
// length of the matrix's FIRST column throughout (the reference never refreshes it, :58-63).
template <int G>
__global__ void __launch_bounds__(256) k_overlap_next(const int64_t *__restrict__ pos, const int32_t *__restrict__ row, int64_t n, double rho,
                                                      int64_t w_max, int32_t *__restrict__ next)
{
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = tid / G;
    if (p >= n) return;
    const int t = (int)(tid % G);
    const int shift = (int)((threadIdx.x & 63) / G) * G;
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    const int64_t c = pos[1] - pos[0];
    const int64_t ps = pos[p], Ls = pos[p + 1] - ps;
    const bool in_regs = Ls <= G;
    const int32_t srow = (in_regs && t < Ls) ? row[ps + t] : -1;
    int64_t jp = p + 1;
    for (; jp < n; jp++) {
        if (w_max >= 1 && jp - p == w_max) break;
        const int64_t qs = pos[jp], Lc = pos[jp + 1] - qs;
        int64_t cc = 0;
        for (int64_t b = 0; b < Lc; b += G) {
            const int32_t x = b + t < Lc ? row[qs + b + t] : -2;
            bool f = false;
            if (in_regs) {
                for (int k = 0; k < G; k++) f |= __shfl(srow, (t + k) & (G - 1), G) == x;
            } else if (x >= 0) {
                int64_t lo = 0, hi = Ls;                 // first entry >= x
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (row[ps + mid] < x) lo = mid + 1; else hi = mid; }
                f = lo < Ls && row[ps + lo] == x;
            }
            cc += __popcll((__ballot(f) >> shift) & gmask);
        }
        const int64_t mn = c < Lc ? c : Lc;
        if ((double)cc < rho * (double)mn) break;
    }
    if (t == 0) next[p] = (int32_t)jp;
}

// ------------------------------------------------------------------ overlap: the orbit of column 0
// jump[n] = n; mark[0] = 1; the intersections the kernel above computed for start p: one per candidate short of next[p], and the one
// that fired unless the width did
__global__ void __launch_bounds__(256) k_orbit_init(int32_t *__restrict__ jump, int32_t *__restrict__ mark, int64_t n, int64_t w_max,
                                                    unsigned long long *__restrict__ isect)
{
    __shared__ unsigned long long sh[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long cnt = 0;
    if (p < n) {
        const int64_t nx = jump[p];
        cnt = (unsigned long long)(nx - p - 1) + ((nx < n && nx - p != w_max) ? 1ull : 0ull);
        mark[p] = p == 0;
    } else if (p == n) { jump[n] = (int32_t)n; mark[n] = 0; }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && (sh[0] + sh[1] + sh[2] + sh[3])) atomicAdd(isect, sh[0] + sh[1] + sh[2] + sh[3]);
}

// one doubling round: every marked p marks jin[p]; jout = jin o jin.  jin is only read and jout only written here: in place, a thread
// would read entries that others have already advanced in the same round, and splits would be skipped.  A mark that becomes visible
// during the round belongs to the orbit, so acting on it early is harmless.
__global__ void __launch_bounds__(256) k_orbit_round(const int32_t *__restrict__ jin, int32_t *__restrict__ jout, int32_t *__restrict__ mark, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    const int32_t a = jin[p];
    if (mark[p]) mark[a] = 1;
    jout[p] = jin[a];
}

// ------------------------------------------------------------------ the common tail
// spl[off[p]] = p + 1 for every flagged column, spl[K] = n + 1 (1-based, as the reference stores them)
__global__ void k_compact_splits(const int32_t *__restrict__ flag, const int64_t *__restrict__ off, int64_t n, int64_t *__restrict__ spl)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    if (p == n) spl[off[n]] = n + 1;
    else if (flag[p]) spl[off[p]] = p + 1;
}

// n_nets[k] = the distinct rows of part k = its entries whose row did not occur before in the part: prev[q] < the part's first
// column.  One lane per entry; the lanes of a wave that share a part add their hits with one atomic.
__global__ void __launch_bounds__(256) k_part_nets(const int32_t *__restrict__ col, const int32_t *__restrict__ prev, const int32_t *__restrict__ flag,
                                                   const int64_t *__restrict__ off, const int64_t *__restrict__ spl, int64_t N,
                                                   unsigned long long *__restrict__ nets)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t k = -1;
    bool hit = false;
    if (q < N) {
        const int32_t p = col[q];
        k = off[p] + flag[p] - 1;
        hit = (int64_t)prev[q] < spl[k] - 1;
    }
    const int64_t kl = __shfl_up(k, 1);
    const bool head = lane == 0 || kl != k;
    const unsigned long long hits = __ballot(hit), heads = __ballot(head);
    if (head && k >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int end = above ? __ffsll((long long)above) - 1 : 64;
        const unsigned long long seg = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
        const int cnt = __popcll(hits & seg);
        if (cnt) atomicAdd(&nets[k], (unsigned long long)cnt);
    }
}

// ------------------------------------------------------------------ host
namespace {
struct GreedyRun {
    cp_csr_s *A;
    hipStream_t s;
    int64_t n;
    DBuf<int32_t> flag;          // n + 1: split flags (strict: neq first; overlap: the orbit marks)
    DBuf<int64_t> off, spl, scratch, nets;

    explicit GreedyRun(cp_csr_s *A_) : A(A_), s(A_->stream), n(A_->n), flag((size_t)A_->n + 1), off((size_t)A_->n + 1), spl((size_t)A_->n + 1) {}

    // flags -> spl_out[0 .. K], K_out, n_nets_out[0 .. K) (entries past those are unspecified); the one stream sync of the entry
    int32_t finish(int64_t *spl_out, int64_t *K_out, int64_t *n_nets_out, unsigned long long *isect_dev)
    {
        const int64_t N = A->N;
        if (n_nets_out) ensure_links(A);
        {
            ProfScope ps(PROF_COMPACT, s, 4.0 * (double)n + 16.0 * (double)(n + 1) + (n_nets_out ? 8.0 * (double)N : 0.0));
            exclusive_scan_i32(flag.p, off.p, n, scratch, s);
            hipLaunchKernelGGL(k_compact_splits, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, flag.p, off.p, n, spl.p);
            if (n_nets_out) {
                nets.alloc((size_t)n);
                CP_HIP(hipMemsetAsync(nets.p, 0, nets.bytes(), s));
                if (N > 0)
                    hipLaunchKernelGGL(k_part_nets, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, A->col.p, A->prev.p, flag.p, off.p, spl.p, N,
                                       (unsigned long long *)nets.p);
            }
            CP_HIP(hipGetLastError());
        }
        unsigned long long isect = 0;
        CP_HIP(hipMemcpyAsync(K_out, off.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        CP_HIP(hipMemcpyAsync(spl_out, spl.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, s));
        if (n_nets_out) CP_HIP(hipMemcpyAsync(n_nets_out, nets.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (isect_dev) CP_HIP(hipMemcpyAsync(&isect, isect_dev, sizeof(isect), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        prof_collect();
        g_overlap_isect += (int64_t)isect;
        return CP_OK;
    }
};
}  // namespace

static int32_t run_pack_strict(cp_csr_s *A, int64_t w_max, int64_t *spl_out, int64_t *K_out)
{
    GreedyRun R(A);
    hipStream_t s = R.s;
    const int64_t n = R.n;
    DBuf<int32_t> start((size_t)n);
    {
        ProfScope ps(PROF_COLNEQ, s, 8.0 * (double)(n + 1) + 8.0 * (double)A->N + 4.0 * (double)n);
        hipLaunchKernelGGL(k_col_neq, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, s, A->pos.p, A->row.p, n, R.flag.p);
        CP_HIP(hipGetLastError());
    }
    {
        ProfScope ps(PROF_COMPACT, s, 16.0 * (double)n);
        scan_last_flagged(R.flag.p, start.p, n, R.scratch, s);
        hipLaunchKernelGGL(k_strict_flags, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, R.flag.p, start.p, n, w_max);
        CP_HIP(hipGetLastError());
    }
    return R.finish(spl_out, K_out, nullptr, nullptr);
}

static int32_t run_pack_overlap(cp_csr_s *A, double rho, int64_t w_max, int64_t *spl_out, int64_t *K_out, int64_t *n_nets_out)
{
    GreedyRun R(A);
    hipStream_t s = R.s;
    const int64_t n = R.n;
    DBuf<int32_t> ja((size_t)n + 1), jb((size_t)n + 1);
    DBuf<unsigned long long> isect(1);
    CP_HIP(hipMemsetAsync(isect.p, 0, sizeof(unsigned long long), s));
    {
        // lanes per start: the power of two from 8 to 64 that holds the mean column
        const int64_t mean = n > 0 ? cdiv(A->N, n) : 0;
        const int G = mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
        const dim3 grid((unsigned)cdiv(n * G, 256)), block(256);
        ProfScope ps(PROF_OVNEXT, s, 8.0 * (double)(n + 1) + 4.0 * (double)A->N + 4.0 * (double)n);
        if (G == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_overlap_next<8>), grid, block, 0, s, A->pos.p, A->row.p, n, rho, w_max, ja.p);
        else if (G == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_overlap_next<16>), grid, block, 0, s, A->pos.p, A->row.p, n, rho, w_max, ja.p);
        else if (G == 32) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_overlap_next<32>), grid, block, 0, s, A->pos.p, A->row.p, n, rho, w_max, ja.p);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_overlap_next<64>), grid, block, 0, s, A->pos.p, A->row.p, n, rho, w_max, ja.p);
        CP_HIP(hipGetLastError());
    }
    {
        int rounds = 0;
        while (((int64_t)1 << rounds) < n + 1) rounds++;            // ceil(log2(n + 1)): every orbit distance is below 2^rounds
        ProfScope ps(PROF_ORBIT, s, 16.0 * (double)(n + 1) * (double)(rounds + 1));
        const dim3 grid((unsigned)cdiv(n + 1, 256)), block(256);
        hipLaunchKernelGGL(k_orbit_init, grid, block, 0, s, ja.p, R.flag.p, n, w_max, isect.p);
        int32_t *jin = ja.p, *jout = jb.p;
        for (int r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(k_orbit_round, grid, block, 0, s, (const int32_t *)jin, jout, R.flag.p, n);
            std::swap(jin, jout);
        }
        CP_HIP(hipGetLastError());
    }
    return R.finish(spl_out, K_out, n_nets_out, isect.p);
}

}  // namespace cpk

using namespace cpk;

extern "C" {

int32_t cp_pack_strict(cp_csr_t A, int64_t w_max, int64_t *spl_out, int64_t *K_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl_out && K_out, CP_EINVAL, "bad argument");
        CP_REQUIRE(A->n >= 1, CP_EINVAL, "StrictChunker needs n >= 1 (the reference reads colptr[2])");
        CP_HIP(hipSetDevice(A->device));
        return run_pack_strict(A, w_max, spl_out, K_out);
    });
}

int32_t cp_pack_overlap(cp_csr_t A, double rho, int64_t w_max, int64_t *spl_out, int64_t *K_out, int64_t *n_nets_out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && spl_out && K_out, CP_EINVAL, "bad argument");
        CP_REQUIRE(A->n >= 1, CP_EINVAL, "OverlapChunker needs n >= 1 (the reference reads colptr[2])");
        CP_HIP(hipSetDevice(A->device));
        return run_pack_overlap(A, rho, w_max, spl_out, K_out, n_nets_out);
    });
}

}  // extern "C"
