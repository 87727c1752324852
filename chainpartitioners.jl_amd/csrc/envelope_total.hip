// envelope_total.hip -- the total-cost layer of the K-part DP for the envelope model by divide and conquer ("Fact 2").
//
// Layer k >= 2 is cst[r] = min over a <= r of W[a] + f(a, r, k), the largest a among equal values.  The span d(a, r) is Monge in
// neither direction, but at any cut column M with a < M <= r it is max(SH(a), PH(r)) - min(SL(a), PL(r)): the extrema of the
// leaves a .. M-1 (the candidate side) and of M .. r-1 (the row side).  With
//     V[a]  = W[a] - a*b_vertex - pos[a]*b_pin            (the candidate key)
//     Rw[r] = alpha_k + r*b_vertex + pos[r]*b_pin         (the row term)
// the objective is V[a] + Rw[r] + b_net*d(a, r).  Every pair a < r belongs to one node [L, L + 2h) of the implicit binary tree
// over 0..n with a in the left half [L, M) and r in the right half.  SH does not rise and SL does not fall with a, so the
// candidates whose SH >= PH(r) are a prefix [L, L + xa) of the left half and those whose SL <= PL(r) a prefix [L, L + xb): two
// binary searches per row, and between the two bounds the value is one of four separable forms (k_dc_rows), each a range minimum
// of a key that depends on the candidate alone.
//
// Pairs inside an aligned block of 64 rows, and the diagonal, are the leaf pass: the candidate sweep of envelope.hip cut off at
// the block.  The levels h = 64, 128, ... <= n each build three keys (k_dc_keys) and answer every row of a right half
// (k_dc_rows).  All four minima -- the prefix of key 1, the suffix of V, a range of key 2 or 3 -- are queries of one two-level
// range-minimum structure: blocks of 64 entries with an in-block sparse table of one-byte offsets, built by one wave with
// shuffles, and a sparse table of positions over the block minima.  Every minimum is the rightmost one.
//
// The regrouped sums are the reference's values only while all of them are exact: env_dc_ok.
#include "envelope.hpp"
#include "dp.hpp"
#include <cmath>

namespace cpk {

int64_t g_env_dc_layers = 0;
int64_t g_opt_env_dc_min_n = 256;           // the measured crossover with the candidate sweep, rounded up to a power of two

constexpr int DC_LEAF = 64;      // rows of a leaf block and entries of a range-minimum block: one wave
constexpr int DC_IB = 6;         // in-block table levels t = 1 .. 6 (t = 0 is the entry itself)
constexpr int DC_KEYS = 4;       // key 0: V (per layer); keys 1 .. 3: per level
constexpr int DC_R1_CHUNK = 4096;      // candidates per workgroup of the one-row reduction

template <typename TC>
struct DcDev {
    TC *kv;                      // key q of candidate a at kv[q * n1p + a]
    uint8_t *ib;                 // ib[(q * DC_IB + t - 1) * n1p + a]: offset from a of the rightmost minimum of [a, a + 2^t) inside a's block
    int32_t *bt;                 // bt[(q * SB + s) * nb + b]: position of the rightmost minimum of the blocks [b, b + 2^s), clipped at nb
    int64_t n1p, nb;             // n + 1 rounded up to whole blocks; blocks
    int32_t SB;                  // levels of bt: floor(log2 nb) + 1
};

// ------------------------------------------------------------------ the gate
// No condition on the sign of a beta.  A total is a sum over up to K parts, so the net term enters K times: the bound is
// K*max|alpha| + n*|b_vertex| + N*|b_pin| + K*m*|b_net|.  Int64: below 2^60, so no key (at most three times the bound) wraps.
// Float64: every parameter finite and integral-valued and the bound below 2^51, so every intermediate -- regrouped or in the
// reference's order -- is an exact integer below 2^53.  A non-integral Float64 model stays on the sweep: the reference's
// left-to-right rounding is not what the regrouped sums give.
bool env_dc_ok(const cp_model_t *m, int64_t m_rows, int64_t n, int64_t N, int64_t K)
{
    const u128 k = (u128)(K > 0 ? K : 1), un = (u128)(n > 0 ? n : 0), uN = (u128)(N > 0 ? N : 0), um = (u128)(m_rows > 0 ? m_rows : 0);
    if (m->dtype == CP_I64) {
        u128 amax = mag128(m->p_i64[CP_P_ALPHA]);
        if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) amax = std::max(amax, mag128(((const int64_t *)m->alpha_k)[i]));
        const u128 bound = amax * k + mag128(m->p_i64[CP_P_VERTEX]) * un + mag128(m->p_i64[CP_P_PIN]) * uN + mag128(m->p_i64[CP_P_NET]) * um * k;
        return bound < ((u128)1 << 60);
    }
    const double lim = 2251799813685248.0;                     // 2^51
    auto whole = [&](double v) { return std::isfinite(v) && std::floor(v) == v && std::fabs(v) < lim; };
    for (int i = 0; i <= CP_P_NET; i++) if (!whole(m->p_f64[i])) return false;
    double amax = std::fabs(m->p_f64[CP_P_ALPHA]);
    if (m->alpha_k) for (int64_t i = 0; i < m->n_alpha_k; i++) {
        const double v = ((const double *)m->alpha_k)[i];
        if (!whole(v)) return false;
        amax = std::max(amax, std::fabs(v));
    }
    // (every factor is an integer below 2^51 or a count below 2^31: the products fit 128 bits)
    const u128 bound = (u128)amax * k + (u128)std::fabs(m->p_f64[CP_P_VERTEX]) * un + (u128)std::fabs(m->p_f64[CP_P_PIN]) * uN +
                       (u128)std::fabs(m->p_f64[CP_P_NET]) * um * k;
    return bound < ((u128)1 << 51);
}

// ------------------------------------------------------------------ device helpers
template <typename T>
__device__ __forceinline__ T dc_shfl_down(T v, int d)
{
    static_assert(sizeof(T) == 8, "cost keys are 8-byte elements");
    union { T t; int w[2]; } u;
    u.t = v;
    u.w[0] = __shfl_down(u.w[0], d, 64);
    u.w[1] = __shfl_down(u.w[1], d, 64);
    return u.t;
}

// (lo, hi) of the leaves [p, r), p < r <= n: the two loads of env_span without the clamp
__device__ __forceinline__ int2 dc_lohi(const EnvDev &E, int64_t p, int64_t r)
{
    const int t = 63 - __clzll((long long)(r - p));
    return env_join(E.tab[(int64_t)t * E.n + p], E.tab[(int64_t)t * E.n + (r - ((int64_t)1 << t))]);
}

template <typename TC>
__device__ __forceinline__ TC dc_row_term(const EnvDev &E, const DevModel<TC> &M, TC alpha, int64_t r)
{
    return cadd(cadd(alpha, cmulc(r, M.p[CP_P_VERTEX])), cmulc(E.pos[r], M.p[CP_P_PIN]));
}

// key q of candidate a into the structure: the value, the in-block table and the block's minimum.  The whole wave calls it with
// a = block start + lane.  After step t a lane holds the rightmost minimum of [a, a + 2^t) cut at the block's end: the partner's
// window lies to the right, so it wins ties.
template <typename TC>
__device__ __forceinline__ void dc_block_build(const DcDev<TC> &D, int q, int64_t a, TC v)
{
    const int lane = threadIdx.x & 63;
    D.kv[(size_t)q * (size_t)D.n1p + (size_t)a] = v;
    int32_t off = 0;
    for (int t = 1; t <= DC_IB; t++) {
        const int sh = 1 << (t - 1);
        const TC pv = dc_shfl_down(v, sh);
        const int32_t po = __shfl_down(off, sh, 64);
        if (lane + sh < 64 && pv <= v) { v = pv; off = po + sh; }
        D.ib[(size_t)(q * DC_IB + t - 1) * (size_t)D.n1p + (size_t)a] = (uint8_t)off;
    }
    if (lane == 0) D.bt[(size_t)q * (size_t)D.SB * (size_t)D.nb + (size_t)(a >> 6)] = (int32_t)(a + off);
}

// rightmost minimum of key q over [x, y] inside one block
template <typename TC>
__device__ __forceinline__ int64_t dc_rmq_block(const DcDev<TC> &D, int q, int64_t x, int64_t y)
{
    const int len = (int)(y - x) + 1;
    const int t = 31 - __clz(len);
    if (t == 0) return x;
    const uint8_t *lev = D.ib + (size_t)(q * DC_IB + t - 1) * (size_t)D.n1p;
    const TC *kv = D.kv + (size_t)q * (size_t)D.n1p;
    const int64_t x2 = y - ((int64_t)1 << t) + 1;
    const int64_t i1 = x + lev[x], i2 = x2 + lev[x2];
    return kv[i2] <= kv[i1] ? i2 : i1;                        // (equal values: i2 >= i1, both are rightmost in their windows)
}

// ... over [x, y], x <= y, anywhere: the tail of x's block, whole blocks between, the head of y's block, left to right
template <typename TC>
__device__ __forceinline__ int64_t dc_rmq(const DcDev<TC> &D, int q, int64_t x, int64_t y)
{
    const int64_t bx = x >> 6, by = y >> 6;
    if (bx == by) return dc_rmq_block(D, q, x, y);
    const TC *kv = D.kv + (size_t)q * (size_t)D.n1p;
    int64_t i = dc_rmq_block(D, q, x, (bx << 6) + 63);
    if (by > bx + 1) {
        const int64_t cnt = by - bx - 1;
        const int s = 63 - __clzll((long long)cnt);
        const int32_t *lev = D.bt + ((size_t)q * (size_t)D.SB + (size_t)s) * (size_t)D.nb;
        const int64_t j1 = lev[bx + 1], j2 = lev[by - ((int64_t)1 << s)];
        const int64_t j = kv[j2] <= kv[j1] ? j2 : j1;
        if (kv[j] <= kv[i]) i = j;
    }
    const int64_t j = dc_rmq_block(D, q, by << 6, y);
    if (kv[j] <= kv[i]) i = j;
    return i;
}

// ------------------------------------------------------------------ kernels
// per layer: V and its structure (key 0); entries past n hold 0 and are never asked for
template <typename TC>
__global__ void __launch_bounds__(256) k_dc_key0(EnvDev E, DevModel<TC> M, const TC *__restrict__ W, DcDev<TC> D)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= D.n1p) return;                                    // (whole waves: n1p is a multiple of 64)
    TC v = (TC)0;
    if (a <= E.n) v = csub(csub(W[a], cmulc(a, M.p[CP_P_VERTEX])), cmulc(E.pos[a], M.p[CP_P_PIN]));
    dc_block_build(D, 0, a, v);
}

// per level h = 2^lgh: keys 1 .. 3 of the candidates in the left half of a node whose middle is a row (M <= n); the other
// entries repeat V and are never asked for
template <typename TC>
__global__ void __launch_bounds__(256) k_dc_keys(EnvDev E, TC bn, int32_t lgh, DcDev<TC> D)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= D.n1p) return;
    const TC v = D.kv[a];
    TC k1 = v, k2 = v, k3 = v;
    const int64_t half = a >> lgh, mid = (half + 1) << lgh;
    if ((half & 1) == 0 && mid <= E.n) {
        const int2 s = dc_lohi(E, a, mid);
        const int64_t d = (int64_t)s.y - (int64_t)s.x;
        k1 = cadd(v, cmulc(d > 0 ? d : (int64_t)0, bn));
        k2 = cadd(v, cmulc((int64_t)s.y, bn));
        k3 = csub(v, cmulc((int64_t)s.x, bn));
    }
    dc_block_build(D, 1, a, k1);
    dc_block_build(D, 2, a, k2);
    dc_block_build(D, 3, a, k3);
}

// level s >= 1 of the table over block minima, keys q0 + blockIdx.y
template <typename TC>
__global__ void __launch_bounds__(256) k_dc_bt_level(DcDev<TC> D, int32_t q0, int32_t s)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.nb) return;
    const int q = q0 + (int)blockIdx.y;
    const TC *kv = D.kv + (size_t)q * (size_t)D.n1p;
    int32_t *lev = D.bt + ((size_t)q * (size_t)D.SB + (size_t)s) * (size_t)D.nb;
    const int32_t *below = lev - D.nb;
    const int64_t b2 = b + ((int64_t)1 << (s - 1));
    int32_t i = below[b];
    if (b2 < D.nb) { const int32_t i2 = below[b2]; if (kv[i2] <= kv[i]) i = i2; }
    lev[b] = i;
}

// the leaf pass: the pairs inside an aligned block of 64 rows and the diagonal, as k_env_sweep walks them -- one lane per row,
// the candidate's leaf is a wave-uniform load folded into the running (lo, hi) of every lane above it
template <typename TC>
__global__ void __launch_bounds__(256) k_dc_leaf(EnvDev E, DevModel<TC> M, TC alpha, const TC *__restrict__ V, TC *__restrict__ cst,
                                                 int32_t *__restrict__ ptr)
{
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t r0 = wave * DC_LEAF;
    if (r0 > E.n) return;
    int64_t r = r0 + lane;
    const bool live = r <= E.n;
    const int64_t rtop = r0 + 63 < E.n ? r0 + 63 : E.n;
    if (!live) r = rtop;
    int32_t lo = E.m + 1, hi = 0;
    TC best = (TC)0;
    int64_t bp = -1;
    for (int64_t p = rtop; p >= r0; p--) {
        if (p < rtop) {                                        // (p < rtop <= n: a column)
            const int2 leaf = E.tab[p];
            if (p < r) { lo = leaf.x < lo ? leaf.x : lo; hi = leaf.y > hi ? leaf.y : hi; }
        }
        if (r >= p) {
            const int64_t d = (int64_t)hi - (int64_t)lo;
            const TC v = cadd(V[p], cmulc(d > 0 ? d : (int64_t)0, M.p[CP_P_NET]));
            if (bp < 0 || v < best) { best = v; bp = p; }
        }
    }
    if (live) { cst[r] = cadd(best, dc_row_term(E, M, alpha, r)); ptr[r] = (int32_t)bp; }
}

// level h = 2^lgh, one lane per row of a right half: thread i is row off = i mod h of node i / h
template <typename TC>
__global__ void __launch_bounds__(256) k_dc_rows(EnvDev E, DevModel<TC> M, TC alpha, int32_t lgh, DcDev<TC> D, TC *__restrict__ cst,
                                                 int32_t *__restrict__ ptr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = (int64_t)1 << lgh, off = i & (h - 1);
    const int64_t L = (i >> lgh) << (lgh + 1), mid = L + h, r = mid + off;
    if (r > E.n) return;
    int32_t PL = E.m + 1, PH = 0;
    if (off > 0) { const int2 s = dc_lohi(E, mid, r); PL = s.x; PH = s.y; }
    int64_t lo = 0, hi = h;                                    // xa: candidates with SH(a) >= PH
    while (lo < hi) {
        const int64_t x = (lo + hi) >> 1;
        if (dc_lohi(E, L + x, mid).y >= PH) lo = x + 1; else hi = x;
    }
    const int64_t xa = lo;
    lo = 0; hi = h;                                            // xb: candidates with SL(a) <= PL
    while (lo < hi) {
        const int64_t x = (lo + hi) >> 1;
        if (dc_lohi(E, L + x, mid).x <= PL) lo = x + 1; else hi = x;
    }
    const int64_t xb = lo;
    const int64_t x0 = xa < xb ? xa : xb, x1 = xa < xb ? xb : xa;
    const TC bn = M.p[CP_P_NET], rw = dc_row_term(E, M, alpha, r);
    TC best = cst[r];
    int64_t bp = ptr[r];
    auto take = [&](TC key, int64_t a) {
        const TC v = cadd(key, rw);
        if (v < best || (v == best && a > bp)) { best = v; bp = a; }
    };
    const size_t np = (size_t)D.n1p;
    if (x0 > 0) {                                              // both extrema from the candidate side
        const int64_t a = dc_rmq(D, 1, L, L + x0 - 1);
        take(D.kv[np + (size_t)a], a);
    }
    if (x1 < h) {                                              // both from the row side
        const int64_t a = dc_rmq(D, 0, L + x1, mid - 1);
        const int64_t d = (int64_t)PH - (int64_t)PL;
        take(cadd(D.kv[a], cmulc(d > 0 ? d : (int64_t)0, bn)), a);
    }
    if (x0 < x1) {
        if (xa > xb) {                                         // hi from the candidate, lo from the row (SH >= PH >= PL: no clamp)
            const int64_t a = dc_rmq(D, 2, L + x0, L + x1 - 1);
            take(csub(D.kv[2 * np + (size_t)a], cmulc((int64_t)PL, bn)), a);
        } else {                                               // lo from the candidate, hi from the row
            const int64_t a = dc_rmq(D, 3, L + x0, L + x1 - 1);
            take(cadd(D.kv[3 * np + (size_t)a], cmulc((int64_t)PH, bn)), a);
        }
    }
    cst[r] = best; ptr[r] = (int32_t)bp;
}

// one row: min over a in [0, r] of W[a] + f(a, r, k) in the reference's order, the largest a among equals
template <typename TC>
__device__ __forceinline__ void dc_better(TC &v, int32_t &a, TC v2, int32_t a2)
{
    if (a2 >= 0 && (a < 0 || v2 < v || (v2 == v && a2 > a))) { v = v2; a = a2; }
}

template <typename TC>
__device__ __forceinline__ void dc_block_reduce(TC &v, int32_t &a)
{
    __shared__ TC sv[4];
    __shared__ int32_t sa[4];
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const TC v2 = dc_shfl_down(v, sh);
        const int32_t a2 = __shfl_down(a, sh, 64);
        dc_better(v, a, v2, a2);
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sa[threadIdx.x >> 6] = a; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) dc_better(v, a, sv[w], sa[w]);
}

template <typename TC>
__global__ void __launch_bounds__(256) k_dc_row1_part(EnvDev E, DevModel<TC> M, TC alpha, const TC *__restrict__ W, int64_t r, TC *__restrict__ pv,
                                                      int32_t *__restrict__ pa)
{
    TC v = (TC)0;
    int32_t a = -1;
    const int64_t base = (int64_t)blockIdx.x * DC_R1_CHUNK;
    for (int64_t p = base + threadIdx.x; p < base + DC_R1_CHUNK && p <= r; p += 256)
        dc_better(v, a, cadd(W[p], env_eval<TC>(E, M, alpha, p, r)), (int32_t)p);
    dc_block_reduce(v, a);
    if (threadIdx.x == 0) { pv[blockIdx.x] = v; pa[blockIdx.x] = a; }
}

template <typename TC>
__global__ void __launch_bounds__(256) k_dc_row1_fin(int64_t nparts, const TC *__restrict__ pv, const int32_t *__restrict__ pa, TC *__restrict__ cst,
                                                     int32_t *__restrict__ ptr)
{
    TC v = (TC)0;
    int32_t a = -1;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) dc_better(v, a, pv[i], pa[i]);
    dc_block_reduce(v, a);
    if (threadIdx.x == 0) { *cst = v; *ptr = a; }
}

// ------------------------------------------------------------------ the layer
template <typename TC>
void env_dc_layer(cp_csr_s *A, const EnvDev &E, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst, int32_t *ptr, int64_t r_lo, int64_t r_hi)
{
    if (r_hi < r_lo) return;
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    EnvWork *Wk = env_work_get(A);
    g_env_dc_layers++;
    ProfScope ps(PROF_ENV_DC, s, 0.0);
    if (r_lo == r_hi) {                                        // (layer K: row n + 1 alone)
        const int64_t nparts = cdiv(r_lo + 1, (int64_t)DC_R1_CHUNK);
        Wk->dc_pv.ensure((size_t)nparts); Wk->dc_pa.ensure((size_t)nparts);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_row1_part<TC>), dim3((unsigned)nparts), dim3(256), 0, s, E, M, alpha, W, r_lo, (TC *)Wk->dc_pv.p,
                           Wk->dc_pa.p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_row1_fin<TC>), dim3(1), dim3(256), 0, s, nparts, (const TC *)Wk->dc_pv.p, Wk->dc_pa.p, cst + r_lo,
                           ptr + r_lo);
        CP_HIP(hipGetLastError());
        return;
    }
    CP_REQUIRE(r_lo == 0 && r_hi == n, CP_EINTERNAL, "env_dc_layer computes one row or all of them");
    DcDev<TC> D;
    D.nb = cdiv(n1, (int64_t)DC_LEAF); D.n1p = D.nb * DC_LEAF;
    D.SB = 1;
    while (((int64_t)2 << (D.SB - 1)) <= D.nb) D.SB++;          // floor(log2 nb) + 1
    Wk->dc_kv.ensure((size_t)DC_KEYS * (size_t)D.n1p);
    Wk->dc_ib.ensure((size_t)DC_KEYS * DC_IB * (size_t)D.n1p);
    Wk->dc_bt.ensure((size_t)DC_KEYS * (size_t)D.SB * (size_t)D.nb);
    D.kv = (TC *)Wk->dc_kv.p; D.ib = Wk->dc_ib.p; D.bt = Wk->dc_bt.p;
    const unsigned ga = (unsigned)cdiv(D.n1p, 256), gb = (unsigned)cdiv(D.nb, 256);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_key0<TC>), dim3(ga), dim3(256), 0, s, E, M, W, D);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_leaf<TC>), dim3((unsigned)cdiv(D.nb, 4)), dim3(256), 0, s, E, M, alpha, (const TC *)D.kv, cst, ptr);
    int32_t built0 = 0;                                        // levels of key 0's block table built so far (level 0 is the build's)
    for (int32_t lgh = 6; ((int64_t)1 << lgh) <= n; lgh++) {
        const int32_t need = lgh - 6;                          // a left half holds 2^(lgh - 6) blocks
        for (; built0 < need; built0++)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_bt_level<TC>), dim3(gb, 1), dim3(256), 0, s, D, 0, built0 + 1);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_keys<TC>), dim3(ga), dim3(256), 0, s, E, M.p[CP_P_NET], lgh, D);
        for (int32_t lv = 1; lv <= need; lv++)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_bt_level<TC>), dim3(gb, 3), dim3(256), 0, s, D, 1, lv);
        const int64_t rows = cdiv(n1, (int64_t)2 << lgh) << lgh;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dc_rows<TC>), dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, s, E, M, alpha, lgh, D, cst, ptr);
    }
    CP_HIP(hipGetLastError());
}

template void env_dc_layer<int64_t>(cp_csr_s *, const EnvDev &, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, int64_t, int64_t);
template void env_dc_layer<double>(cp_csr_s *, const EnvDev &, const DevModel<double> &, double, const double *, double *, int32_t *, int64_t, int64_t);

}  // namespace cpk
