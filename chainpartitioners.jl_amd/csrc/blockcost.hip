// blockcost.hip -- BlockComponentCostModel (BlockCosts.jl:19-152) as a weighted net count.  The reference's oracle is a cursor
// with a history per row part; the cost it returns is not stateful.  With Pi a split of the rows, let Q be the quotient pattern:
// A with the rows of every part merged, one entry (k, c) per part k holding a nonzero of column c.  Then
//
//     d[r](j, j') = sum over the parts k touched by the columns j .. j'-1 of beta_row[r](u_k)              u_k = rows of part k
//                 = sum over the entries (k, c) of Q with j <= c < j' whose previous entry of row k lies left of j
//     cost(j, j') = alpha_col(w) + sum_r d[r] * beta_col[r](w)                                             w = j' - j
//
// which is the "count an entry iff its previous occurrence lies left of j" rule of every link-array kernel, with a weight.
//   cp_csr_quotient / block_quotient : Q by flag -> scan -> scatter (the entries of one part are contiguous inside a column)
//   k_block_window_table             : every pair within a width window, one lane per j' (the table of chunk_scan.hip)
//   k_block_eval                     : a batch of queries, one wave each over the query's contiguous entry range of Q
// Both kernels stream next to Q's link array one more int32 per entry, the part size u_k, and read beta_row from its table by
// u: no indirection of the size of the partition.  Sums are reassociated, so both run only inside blockcost_exact.
#include "blockcost.hpp"
#include "dp.hpp"

namespace cpk {

int64_t g_opt_blockcost_par = 1;
int64_t g_blockcost_scan_packs = 0;
int64_t g_blockcost_wave_evals = 0;

// ------------------------------------------------------------------ the quotient pattern
// part of the 0-based row i, 0-based: the largest k with spl[k] - 1 <= i (spl: K + 1 1-based boundaries, spl[0] = 1, spl[K] = m + 1;
// a repeated boundary is an empty part, which no row reaches)
__global__ void __launch_bounds__(256) k_bq_part(const int32_t *__restrict__ row, const int64_t *__restrict__ spl, int64_t K, int64_t N,
                                                 int32_t *__restrict__ part)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    int64_t i = row[q], lo = 0, hi = K;
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (spl[mid] - 1 <= i) lo = mid; else hi = mid;
    }
    part[q] = (int32_t)lo;
}

// flag[q] = 1 where an entry of Q starts: the first nonzero of a column, or another part than the nonzero above it
__global__ void __launch_bounds__(256) k_bq_flag(const int64_t *__restrict__ pos, int64_t n, const int32_t *__restrict__ part, int64_t N,
                                                 int32_t *__restrict__ flag)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N) return;
    int64_t lo = 0, hi = n;            // largest c with pos[c] <= q: the column of q
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (pos[mid] <= q) lo = mid; else hi = mid;
    }
    flag[q] = (q == pos[lo]) || part[q] != part[q - 1];
}

__global__ void __launch_bounds__(256) k_bq_scatter(const int32_t *__restrict__ flag, const int64_t *__restrict__ rank, const int32_t *__restrict__ part,
                                                    int64_t N, int32_t *__restrict__ qrow)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < N && flag[q]) qrow[rank[q]] = part[q];
}

__global__ void __launch_bounds__(256) k_bq_pos(const int64_t *__restrict__ pos, const int64_t *__restrict__ rank, int64_t n, int64_t *__restrict__ qpos)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= n) qpos[c] = rank[pos[c]];
}

// qu[q] = rows of the part of entry q
__global__ void __launch_bounds__(256) k_bq_usize(const int32_t *__restrict__ qrow, const int64_t *__restrict__ spl, int64_t Nq, int32_t *__restrict__ qu)
{
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < Nq) { int64_t k = qrow[q]; qu[q] = (int32_t)(spl[k + 1] - spl[k]); }
}

static void check_split(const cp_csr_s *A, const cp_rowpart_t *Pi)
{
    CP_REQUIRE(Pi && Pi->spl && Pi->K >= 1, CP_EINVAL, "BlockComponentCostModel needs a SplitPartition of the rows");
    CP_REQUIRE(Pi->spl[0] == 1 && Pi->spl[Pi->K] == A->m + 1, CP_EINVAL, "row partition does not cover 1:m");
    CP_REQUIRE(Pi->K < (int64_t)1 << 30, CP_EUNSUPPORTED, "row partition exceeds the 32-bit link-array layout");
}

static void upload_split(const cp_rowpart_t *Pi, DBuf<int64_t> &spl, hipStream_t s)
{
    spl.alloc((size_t)Pi->K + 1);
    CP_HIP(hipMemcpyAsync(spl.p, Pi->spl, sizeof(int64_t) * (size_t)(Pi->K + 1), hipMemcpyHostToDevice, s));
}

void block_quotient(cp_csr_s *A, const cp_rowpart_t *Pi, cp_csr_s *Q)
{
    check_split(A, Pi);
    hipStream_t s = A->stream;
    const int64_t n = A->n, N = A->N, K = Pi->K;
    Q->m = K; Q->n = n; Q->N = 0;
    Q->pos.alloc((size_t)n + 1);
    if (N == 0) {
        Q->row.alloc(1);
        CP_HIP(hipMemsetAsync(Q->pos.p, 0, Q->pos.bytes(), s));
        CP_HIP(hipStreamSynchronize(s));
        return;
    }
    ProfScope ps(PROF_BLOCKQ, s, 16.0 * (double)N);
    DBuf<int64_t> spl, rank((size_t)N + 1), scratch;
    DBuf<int32_t> part((size_t)N), flag((size_t)N);
    upload_split(Pi, spl, s);
    const dim3 gN((unsigned)cdiv(N, 256)), b(256);
    hipLaunchKernelGGL(k_bq_part, gN, b, 0, s, A->row.p, spl.p, K, N, part.p);
    hipLaunchKernelGGL(k_bq_flag, gN, b, 0, s, A->pos.p, n, part.p, N, flag.p);
    exclusive_scan_i32(flag.p, rank.p, N, scratch, s);
    int64_t Nq = 0;
    CP_HIP(hipMemcpyAsync(&Nq, rank.p + N, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    Q->N = Nq;
    Q->row.alloc((size_t)(Nq > 0 ? Nq : 1));
    hipLaunchKernelGGL(k_bq_scatter, gN, b, 0, s, flag.p, rank.p, part.p, N, Q->row.p);
    hipLaunchKernelGGL(k_bq_pos, dim3((unsigned)cdiv(n + 1, 256)), b, 0, s, A->pos.p, rank.p, n, Q->pos.p);
    CP_HIP(hipGetLastError());
    CP_HIP(hipStreamSynchronize(s));                  // the staging arrays are released on return
}

// ------------------------------------------------------------------ the gate
// The table and the scan reassociate the sums block_call forms by +Delta / -Delta steps, and the wave evaluation sums a range in
// lane order: the same values only while every one of them is the true integer.  No value either side forms exceeds
//     B = (n + 1) * max|alpha_col| + sum_r S_r * max_w |beta_col[r](w)|,    S_r = N_q * max_k |beta_row[r](u_k)|
// -- every chunk of a chunking counts an entry of Q at most once, so S_r bounds sum d[r] over the chunks as well as one d[r], and
// (n + 1) chunks bound the alpha terms.  S_r is the cheap upper bound of the per-entry magnitude sum, not a reduction over Q: the N_q
// entries times the largest |beta_row[r]| at a part size u_k of Pi (the nonempty parts; read as dm_comp reads the table) -- the
// row tables are tabulated up to m + 1 rows, far past any part, and their far end must not decide.  The maxima of alpha_col and
// beta_col run over the constants and every tabulated entry.  Int64: B in 128 bits, below 2^60 (as model_exact_on: clear of the
// scan's 2^61 sentinel).  Float64: every constant and every tabulated entry of alpha_col, beta_col and beta_row integer-valued
// and B below 2^53.  alpha_row is no term of the cost (BlockCosts.jl:136-141).
template <typename T, typename F>
static void for_each_part_value(const cp_component_t &c, const cp_rowpart_t *Pi, F &&f)
{
    if (c.is_const || !c.table || c.len <= 0) { f(c.is_const ? comp_const<T>(c) : (T)0); return; }
    for (int64_t k = 0; k < Pi->K; k++) {
        int64_t u = Pi->spl[k + 1] - Pi->spl[k];
        if (u <= 0) continue;
        u -= c.lo;
        f(((const T *)c.table)[u < 0 ? 0 : u >= c.len ? c.len - 1 : u]);
    }
}

bool blockcost_exact(const cp_model_t *mdl, const cp_rowpart_t *Pi, const cp_csr_s *Q)
{
    if (mdl->kind != CP_MODEL_BLOCK || mdl->R < 0 || mdl->R > CP_MAX_R) return false;
    const int64_t n = Q->n, Nq = Q->N;
    if (mdl->dtype == CP_I64) {
        const u128 LIM = (u128)1 << 60;
        auto comp_max = [](const cp_component_t &c) {
            if (c.is_const) return mag128(c.c_i64);
            u128 r = 0;
            if (c.table) for (int64_t i = 0; i < c.len; i++) r = std::max(r, mag128(((const int64_t *)c.table)[i]));
            return r;
        };
        u128 bound = comp_max(mdl->alpha_col) * (u128)(n + 1);
        for (int r = 0; r < mdl->R; r++) {
            u128 rmax = 0;
            for_each_part_value<int64_t>(mdl->beta_row[r], Pi, [&](int64_t v) { rmax = std::max(rmax, mag128(v)); });
            u128 S = rmax * (u128)Nq;                                // < 2^95
            if (S > LIM) S = LIM;                                    // (keeps the next product inside 128 bits; still >= 2^60 unless beta_col is 0)
            bound += S * comp_max(mdl->beta_col[r]);
        }
        return bound < LIM;
    }
    bool integral = true;
    auto one = [&](double v) { if (!(std::floor(v) == v)) integral = false; return std::fabs(v); };
    auto comp_max = [&](const cp_component_t &c) {
        if (c.is_const) return one(c.c_f64);
        double r = 0;
        if (c.table) for (int64_t i = 0; i < c.len; i++) r = std::max(r, one(((const double *)c.table)[i]));
        return r;
    };
    double bound = comp_max(mdl->alpha_col) * (double)(n + 1);
    for (int r = 0; r < mdl->R; r++) {
        double rmax = 0;
        comp_max(mdl->beta_row[r]);                                   // (integer-valued at every tabulated entry, reached or not)
        for_each_part_value<double>(mdl->beta_row[r], Pi, [&](double v) { rmax = std::max(rmax, std::fabs(v)); });
        bound += rmax * (double)Nq * comp_max(mdl->beta_col[r]);
    }
    return integral && bound < 9007199254740992.0;       // 2^53 (a NaN bound fails it)
}

std::unique_ptr<BlockQ> block_quotient_exact(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi)
{
    std::unique_ptr<BlockQ> B(new BlockQ());
    B->Q.reset(new cp_csr_s());
    cp_csr_s *Q = B->Q.get();
    Q->device = A->device; Q->stream = A->stream; Q->own_stream = false;      // (borrowed: the destructor leaves the stream alone)
    block_quotient(A, Pi, Q);
    if (!blockcost_exact(mdl, Pi, Q)) return nullptr;
    ensure_links(Q);
    hipStream_t s = A->stream;
    const int64_t Nq = Q->N;
    B->qu.alloc((size_t)Nq + 16);                         // (the slack of the link arrays it is streamed next to)
    if (Nq > 0) {
        DBuf<int64_t> spl;
        upload_split(Pi, spl, s);
        ProfScope ps(PROF_BLOCKQ, s, 8.0 * (double)Nq);
        hipLaunchKernelGGL(k_bq_usize, dim3((unsigned)cdiv(Nq, 256)), dim3(256), 0, s, Q->row.p, spl.p, Nq, B->qu.p);
        CP_HIP(hipGetLastError());
        CP_HIP(hipStreamSynchronize(s));
    }
    return B;
}

// ------------------------------------------------------------------ the cost from the weighted counts
// beta_row[r] as the kernels read it: a constant or a device table by the part size
template <typename TC>
struct BlockRows {
    int32_t is_const[CP_MAX_R];
    TC c[CP_MAX_R];
    const TC *tab[CP_MAX_R];
    int64_t len[CP_MAX_R], lo[CP_MAX_R];
};
template <typename TC>
struct BlockRowsHost {
    BlockRows<TC> d;
    DBuf<TC> tabs[CP_MAX_R];
    BlockRowsHost(const cp_model_t *mdl, hipStream_t s)
    {
        memset(&d, 0, sizeof(d));
        for (int r = 0; r < mdl->R && r < CP_MAX_R; r++) {
            const cp_component_t &c = mdl->beta_row[r];
            d.is_const[r] = c.is_const; d.c[r] = comp_const<TC>(c); d.lo[r] = c.lo;
            if (!c.is_const && c.table && c.len > 0) {
                tabs[r].alloc((size_t)c.len);
                CP_HIP(hipMemcpyAsync(tabs[r].p, c.table, sizeof(TC) * (size_t)c.len, hipMemcpyHostToDevice, s));
                d.tab[r] = tabs[r].p; d.len[r] = c.len;
            }
        }
    }
};

// acc[r] += beta_row[r](u), r < R (the loops are unrolled over CP_MAX_R so that acc stays in registers)
template <typename TC>
__device__ __forceinline__ void block_add(const BlockRows<TC> &B, int R, TC (&acc)[CP_MAX_R], int64_t u)
{
#pragma unroll
    for (int r = 0; r < CP_MAX_R; r++)
        if (r < R) acc[r] = cadd(acc[r], dm_comp(B.is_const[r], B.c[r], B.tab[r], B.len[r], B.lo[r], u));
}

// the tail of block_call (seq.hip), statement for statement
template <typename TC>
__device__ __forceinline__ TC block_cost(const DevModel<TC> &f, const TC (&acc)[CP_MAX_R], int64_t w)
{
    TC c = dm_comp(f.ac_const, f.ac_c, f.ac_tab, f.ac_len, f.ac_lo, w);
#pragma unroll
    for (int r = 0; r < CP_MAX_R; r++)
        if (r < f.R) c = cadd(c, cmulv(acc[r], dm_comp(f.bc_const[r], f.bc_c[r], f.bc_tab[r], f.bc_len[r], f.bc_lo[r], w)));
    return c;
}

// ------------------------------------------------------------------ every pair inside a width window
// One lane per j' walks the candidates j = j' - d downwards as k_window_table does: column p = j' - 1 - d adds the weight of its
// entries of Q whose next entry of the same part lies at or right of j' - 1 (the last one of the part inside the window).
// Neighbouring lanes read neighbouring columns' entry ranges at every step.
template <typename TC>
__global__ void __launch_bounds__(256) k_block_window_table(DevModel<TC> M, BlockRows<TC> B, int64_t n, int64_t Wc, const int64_t *__restrict__ qpos,
                                                            const int32_t *__restrict__ qnext, const int32_t *__restrict__ qu, TC *__restrict__ F)
{
    int64_t jp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;       // 1-based j'
    if (jp > n + 1) return;
    const int64_t r = jp - 1;
    const int32_t rr = (int32_t)r;
    TC acc[CP_MAX_R];
#pragma unroll
    for (int i = 0; i < CP_MAX_R; i++) acc[i] = (TC)0;
    TC *row = F + jp * (Wc + 1);
    row[0] = block_cost(M, acc, (int64_t)0);
    for (int64_t d = 1; d <= Wc; d++) {
        const int64_t p = r - d;
        if (p < 0) break;
        for (int64_t q = qpos[p]; q < qpos[p + 1]; q++)
            if (qnext[q] >= rr) block_add(B, M.R, acc, (int64_t)qu[q]);
        row[d] = block_cost(M, acc, d);
    }
}

template <typename TC>
void block_window_table(cp_csr_s *A, const BlockQ &B, const cp_model_t *mdl, const DevModel<TC> &M, int64_t Wc, DBuf<TC> &F)
{
    const int64_t n = A->n;
    CP_REQUIRE(block_table_fits(n, Wc), CP_EINVAL, "internal: block window table beyond its size limit");
    hipStream_t s = A->stream;
    const cp_csr_s *Q = B.Q.get();
    BlockRowsHost<TC> rows(mdl, s);
    F.alloc((size_t)(n + 2) * (size_t)(Wc + 1));
    {
        ProfScope ps(PROF_BLOCKTAB, s, 8.0 * (double)Q->N * (double)Wc);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_block_window_table<TC>), dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, M, rows.d, n, Wc, Q->pos.p,
                           Q->next.p, B.qu.p, F.p);
    }
    CP_HIP(hipGetLastError());
    CP_HIP(hipStreamSynchronize(s));                  // (the row tables are released on return)
}
template void block_window_table<int64_t>(cp_csr_s *, const BlockQ &, const cp_model_t *, const DevModel<int64_t> &, int64_t, DBuf<int64_t> &);
template void block_window_table<double>(cp_csr_s *, const BlockQ &, const cp_model_t *, const DevModel<double> &, int64_t, DBuf<double> &);

// ------------------------------------------------------------------ a batch of queries, one wave each
__device__ __forceinline__ int64_t bq_shfl_down(int64_t v, int o)
{
    int lo = __shfl_down((int)(v & 0xffffffffll), o), hi = __shfl_down((int)(v >> 32), o);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ double bq_shfl_down(double v, int o) { return __longlong_as_double((long long)bq_shfl_down((int64_t)__double_as_longlong(v), o)); }

// The entries of the columns j .. j'-1 are one contiguous range of Q; an entry counts iff the previous entry of its part lies left
// of column j.  The lanes stride over the range, the partial sums meet by shuffles, lane 0 evaluates the cost.
template <typename TC>
__global__ void __launch_bounds__(256) k_block_eval(DevModel<TC> M, BlockRows<TC> B, int64_t nq, const int64_t *__restrict__ j, const int64_t *__restrict__ jp,
                                                    const int64_t *__restrict__ qpos, const int32_t *__restrict__ qprev, const int32_t *__restrict__ qu,
                                                    TC *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);       // one query per wave
    if (t >= nq) return;
    const int lane = lane_id();
    const int64_t p = j[t] - 1, r = jp[t] - 1;                                             // 0-based columns [p, r)
    const int32_t pp = (int32_t)p;
    TC acc[CP_MAX_R];
#pragma unroll
    for (int i = 0; i < CP_MAX_R; i++) acc[i] = (TC)0;
    for (int64_t q = qpos[p] + lane, q1 = qpos[r]; q < q1; q += 64)
        if (qprev[q] < pp) block_add(B, M.R, acc, (int64_t)qu[q]);
#pragma unroll
    for (int i = 0; i < CP_MAX_R; i++)
        if (i < M.R)
            for (int o = 32; o > 0; o >>= 1) acc[i] = cadd(acc[i], bq_shfl_down(acc[i], o));
    if (lane == 0) out[t] = block_cost(M, acc, r - p);
}

template <typename TC>
bool run_block_eval(cp_csr_s *A, const cp_model_t *mdl, const cp_rowpart_t *Pi, int64_t nq, const int64_t *j, const int64_t *jp, TC *out)
{
    if (!g_opt_blockcost_par || g_opt_force_brute || nq <= 0) return false;
    for (int64_t t = 0; t < nq; t++) if (!(j[t] >= 1 && jp[t] >= j[t] && jp[t] <= A->n + 1)) return false;
    std::unique_ptr<BlockQ> B = block_quotient_exact(A, mdl, Pi);
    if (!B) return false;
    hipStream_t s = A->stream;
    const cp_csr_s *Q = B->Q.get();
    HostModel<TC> HM;
    build_dev_model<TC>(mdl, HM, s);
    BlockRowsHost<TC> rows(mdl, s);
    DBuf<int64_t> dj((size_t)nq), djp((size_t)nq);
    DBuf<TC> dout((size_t)nq);
    CP_HIP(hipMemcpyAsync(dj.p, j, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    CP_HIP(hipMemcpyAsync(djp.p, jp, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(PROF_BLOCKEVAL, s, 8.0 * (double)Q->N);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_block_eval<TC>), dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, HM.d, rows.d, nq, dj.p, djp.p, Q->pos.p, Q->prev.p,
                           B->qu.p, dout.p);
    }
    CP_HIP(hipGetLastError());
    CP_HIP(hipMemcpyAsync(out, dout.p, sizeof(TC) * (size_t)nq, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    prof_collect();
    g_blockcost_wave_evals += nq;
    return true;
}
template bool run_block_eval<int64_t>(cp_csr_s *, const cp_model_t *, const cp_rowpart_t *, int64_t, const int64_t *, const int64_t *, int64_t *);
template bool run_block_eval<double>(cp_csr_s *, const cp_model_t *, const cp_rowpart_t *, int64_t, const int64_t *, const int64_t *, double *);

}  // namespace cpk

using namespace cpk;

extern "C" int32_t cp_csr_quotient(cp_csr_t A, const cp_rowpart_t *Pi, cp_csr_t *out)
{
    return guarded([&]() -> int32_t {
        CP_REQUIRE(A && out, CP_EINVAL, "null argument");
        CP_HIP(hipSetDevice(A->device));
        std::unique_ptr<cp_csr_s> Q(new cp_csr_s());
        Q->device = A->device;
        CP_HIP(hipStreamCreate(&Q->stream));
        Q->own_stream = true;
        block_quotient(A, Pi, Q.get());
        prof_collect();
        *out = Q.release();
        return CP_OK;
    });
}
