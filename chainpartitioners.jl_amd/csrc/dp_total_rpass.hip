// dp_total_rpass.hip -- the RIGHT PASS of a round of the total-cost DP layer (scheme: dp_total.hip): the row-major threshold counts
// cr / crl of the rows with ctz == tau (k_rpass_small, k_rpass_wave), the anchors of the last row's round-A tasks
// (k_last_row_counts), and k_setup, whose one launch left is the clear of the counters the chunks of a row add into.
#include "dp_total.hpp"

namespace cpk {

// ------------------------------------------------------------------ right part: row-major threshold counts
// cr[b][r] = #{q in columns [r-2^tau, r) : prev[q] < opt[b][r-2^tau]} for every set bit b > tau of r.
// Small ranges: one lane per row (tau <= 3).
// `ge` selects the comparison: 0: link < threshold (nets: prev[q] < B); 1: link >= threshold (self nets: first >= B
// over the rows bucketed by their LAST column).
// The 64 rows of a wave are consecutive, so they share every bit above tau + 6: planes whose bit is clear in the whole
// wave are skipped with a wave-uniform test (about half of them).
// (Tried: G = 2 .. 16 lanes per row, the group reading 16 G contiguous entries per step (a load instruction within 8 cache lines
//  instead of 64) and adding up by a butterfly: 238 / 262 / 288 / 325 us at tau = 4 .. 1 against 161 / 149 / 167 / 217 -- the
//  per-wave prelude (thresholds of two dozen planes) is then paid per 64 / G rows.)
// (Tried: deciding all planes but one by the position of the link value among the Fenwick blocks, with lane-private LDS
//  histograms -- 4x fewer VALU instructions but 300 B of LDS per row leave 2 waves per SIMD: slower.)
template <bool ge, int NB>
__global__ void __launch_bounds__(256) k_rpass_small(int tau, int nbits, int64_t n, int64_t u0, int64_t nrows, const int64_t *__restrict__ pos,
                                                     const int32_t *__restrict__ prev, const int32_t *__restrict__ opt,
                                                     int32_t *__restrict__ cr, int allp, int cap)
{
    // allp (windowed layers): every row takes part in every plane tau < b < nbits (an empty block holds the threshold -1 or a
    // stale value: its count is never read)
    int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = u < nrows;
    u += u0;
    int64_t r = ((u << 1) | 1) << tau;
    if (r > n) live = false;
    if (!live) r = 0;                                          // no bits: takes part in the ballots only
    int64_t n1 = n + 1, rL = r - ((int64_t)1 << tau);
    int32_t thr[NB], cnt[NB];
    uint32_t used = 0;                                         // planes with a set bit somewhere in the wave (uniform)
    int64_t prL = live ? prow((rL), n1 - 1) : 0;
    // all threshold loads are issued back to back (a lane without bit b reads a valid dummy slot): one memory latency, not 23
#pragma unroll
    for (int b = 0; b < NB; b++) {
        cnt[b] = 0;
        thr[b] = ge ? INT32_MAX : INT32_MIN;
        if (b <= tau || b >= nbits) continue;                  // wave-uniform
        bool on = live && (allp || ((r >> b) & 1));
        if (!__ballot(on)) continue;                           // wave-uniform
        used |= 1u << b;
        int32_t v = opt[(int64_t)b * n1 + (on ? prL : 0)];
        if (on) thr[b] = v;
    }
    // Degrees vary a lot (the bench matrix: mean 10, one column in a hundred above 60) and a wave steps as often as its longest
    // lane: every lane takes the first `cap` entries of its row on its own, sixteen per step, and what a row has beyond them
    // is counted by the whole wave, 64 entries per coalesced load with the row's thresholds broadcast (the k_rpass_wave scheme).
    int64_t q0 = 0;
    int32_t len = 0;
    if (live) { q0 = pos[rL]; len = (int32_t)(pos[r] - q0); }
    const int32_t NEVER = ge ? INT32_MIN : INT32_MAX;          // a link value that is never counted
    const int32_t mlen = len < cap ? len : cap;
    for (int32_t o = 0; o < mlen; o += 16) {                   // sixteen entries in flight per lane
        int32_t v[16];
        // four 16-byte loads (dword-aligned: the global path takes unaligned vectors; the link arrays carry 16 entries of
        // slack) instead of sixteen 4-byte ones: every lane reads another cache line, and the L1 takes a line per lane and
        // instruction whatever its width
        struct __attribute__((packed, aligned(4))) V4 { int32_t a, b, c, d; };
        const V4 *pv = reinterpret_cast<const V4 *>(prev + q0 + o);
        const int32_t rem = mlen - o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            V4 t = {NEVER, NEVER, NEVER, NEVER};
            if (4 * j < rem) t = pv[j];
            v[4 * j] = t.a; v[4 * j + 1] = t.b; v[4 * j + 2] = t.c; v[4 * j + 3] = t.d;
        }
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = j < rem ? v[j] : NEVER;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (!((used >> b) & 1)) continue;                  // wave-uniform
            int32_t t = thr[b];
            int32_t c = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) c += ge ? (v[j] >= t) : (v[j] < t);
            cnt[b] += c;
        }
    }
    {
        const int lane = threadIdx.x & 63;
        uint32_t mypl = 0;                                     // the planes this lane's row takes part in
        if (live)
            for (int b = tau + 1; b < nbits; b++) if (allp || ((r >> b) & 1)) mypl |= 1u << b;
        uint64_t rest = __ballot(len > cap);
        const int32_t q0lo = (int32_t)(uint32_t)q0, q0hi = (int32_t)(q0 >> 32);
        while (rest) {                                         // wave-uniform
            const int src = __ffsll((unsigned long long)rest) - 1;
            rest &= rest - 1;
            const int64_t a = (((int64_t)__builtin_amdgcn_readlane(q0hi, src) << 32) | (uint32_t)__builtin_amdgcn_readlane(q0lo, src)) + cap;
            const int32_t ln = __builtin_amdgcn_readlane(len, src) - cap;
            const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int32_t)mypl, src);
            for (int32_t o = 0; o < ln; o += 64) {
                const int32_t v = o + lane < ln ? prev[a + o + lane] : NEVER;
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    if (!((pl >> b) & 1)) continue;            // scalar branch
                    const int32_t t = __builtin_amdgcn_readlane(thr[b], src);
                    const int32_t c = (int32_t)__popcll(__ballot(ge ? (v >= t) : (v < t)));
                    if (lane == src) cnt[b] += c;
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int b = 0; b < NB; b++)
        if (b > tau && b < nbits && (allp || ((r >> b) & 1))) cr[(int64_t)b * n1 + prow((r), n1 - 1)] = cnt[b];
}

// Larger ranges: one wave per (row, chunk of CH columns); coalesced 64-entry loads.  The row -- hence every threshold -- is
// wave-uniform: thresholds live in SGPRs, a plane's count of 64 entries is ONE vector compare into a lane mask plus a scalar
// popcount and add (s_bcnt1 / s_add on the scalar unit), and the wave total needs no cross-lane reduction at the end.
// (Round 1 kept per-lane counters: a compare and an add per entry and plane on the vector unit, 6 shuffles per plane to finish.)
template <bool ge, int WPB>
__global__ void __launch_bounds__(64 * WPB) k_rpass_wave(int tau, int nbits, int64_t n, int64_t u0, int64_t nrows, int chunks_per_row, int ch_cols,
                                                         const int64_t *__restrict__ pos, const int32_t *__restrict__ prev,
                                                         const int32_t *__restrict__ opt, int32_t *__restrict__ cr, int allp)
{
    // WPB > 1 (the host gives such a block WPB chunks of ONE row: chunks_per_row % WPB == 0): the waves add their counts in
    // LDS and one of them updates the row.  Thousands of chunks of a row of a high round each sending an atomic to the same
    // dozen addresses cost 35 ns apiece, one after the other: 70 us of an 85 us pass.
    int64_t w = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    int64_t u = w / chunks_per_row;
    int ck = (int)(w - u * chunks_per_row);
    if (u >= nrows) return;                                    // (block-uniform when WPB > 1)
    u += u0;
    int64_t r = ((u << 1) | 1) << tau;
    if (r > n) return;
    int64_t n1 = n + 1, rL = r - ((int64_t)1 << tau);
    int64_t c0 = rL + (int64_t)ck * ch_cols, c1 = c0 + ch_cols;
    if (c1 > r) c1 = r;
    int64_t prL = prow((rL), n1 - 1);
    // planes of this row (wave-uniform).  Lane b holds plane b: it fetches the plane's threshold (ONE vector memory instruction
    // for the row -- a uniform-address load per plane cost a dozen), keeps its count and stores it at the end.  The counting
    // loop walks the set bits of `act`: v_readlane hands the threshold to the scalar side, a plane's count of 64 entries is one
    // vector compare into a lane mask and a scalar popcount.  (Thresholds and counts in scalar register ARRAYS, one slot per
    // plane, spilled 40-110 SGPRs into vector lanes and paid a skipped branch for every plane the row does not have.)
    uint32_t act = 0;
    for (int b = tau + 1; b < nbits; b++) if (allp || ((r >> b) & 1)) act |= 1u << b;
    act = __builtin_amdgcn_readfirstlane(act);
    const bool mine = lane < 32 && ((act >> lane) & 1);
    const int32_t tv = mine ? opt[(int64_t)lane * n1 + prL] : 0;
    int32_t acc = 0;
    const int64_t q0 = pos[c0], q1 = pos[c1];
    const int32_t NEVER = ge ? INT32_MIN : INT32_MAX;          // a link value that is never counted
    // 512 entries per step as two 16-byte loads per lane, the next step's issued before this one's are counted: 4 KB in flight per
    // wave at 39 VGPRs.  (With scalar-register arrays for thresholds and counts, four 16-byte loads per lane and 1024 entries per
    // step needed 101 VGPRs -- occupancy 4, 18 % slower.)
    int32_t a[8], nx[8];
    struct __attribute__((packed, aligned(4))) V4 { int32_t x, y, z, w; };      // (16-byte loads, dword-aligned: a quarter of the memory instructions)
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int64_t q = q0 + 4 * lane + 256 * k;
        V4 t = {NEVER, NEVER, NEVER, NEVER};
        if (q < q1) t = *reinterpret_cast<const V4 *>(prev + q);
        a[4 * k] = t.x; a[4 * k + 1] = q + 1 < q1 ? t.y : NEVER; a[4 * k + 2] = q + 2 < q1 ? t.z : NEVER; a[4 * k + 3] = q + 3 < q1 ? t.w : NEVER;
    }
    for (int64_t qb = q0; qb < q1; qb += 512) {                // (a wave-uniform trip count keeps the counters on the scalar unit)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int64_t q = qb + 512 + 4 * lane + 256 * k;
            V4 t = {NEVER, NEVER, NEVER, NEVER};
            if (q < q1) t = *reinterpret_cast<const V4 *>(prev + q);
            nx[4 * k] = t.x; nx[4 * k + 1] = q + 1 < q1 ? t.y : NEVER; nx[4 * k + 2] = q + 2 < q1 ? t.z : NEVER; nx[4 * k + 3] = q + 3 < q1 ? t.w : NEVER;
        }
        for (uint32_t rem = act; rem; rem &= rem - 1) {
            const int b = __ffs(rem) - 1;
            const int32_t t = __builtin_amdgcn_readlane(tv, b);
            int32_t c = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) c += (int32_t)__popcll(__ballot(ge ? (a[k] >= t) : (a[k] < t)));
            acc += lane == b ? c : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) a[k] = nx[k];
    }
    int32_t outv = acc;
    if (WPB > 1) {
        __shared__ int32_t sacc[WPB > 1 ? WPB : 1][32];
        const int wv = threadIdx.x >> 6;
        if (lane < 32) sacc[wv][lane] = mine ? outv : 0;
        __syncthreads();
        if (wv != 0) return;
        if (mine) {
            int32_t t = 0;
#pragma unroll
            for (int k = 0; k < WPB; k++) t += sacc[k][lane];
            outv = t;
        }
    }
    if (mine) {
        if (chunks_per_row == WPB) cr[(int64_t)lane * n1 + prow((r), n1 - 1)] = outv;
        else atomicAdd(&cr[(int64_t)lane * n1 + prow((r), n1 - 1)], outv);
    }
}

// ------------------------------------------------------------------ the last row n in the planes above its lowest bit
// anchors of its round-A tasks: out[b] = #{q in columns [r_b, n) : prev[q] < r_b}, out[32 + b] = #{rows with last column in
// [r_b, n) and first column >= r_b} (hyperedge costs), r_b = n with the bits below b cleared.  Entry q lies in a column >= r_b
// iff q >= pos[r_b].  Then the rows are marked final: the round of ctz(n) skips them.
__global__ void __launch_bounds__(256) k_last_row_counts(RoundDesc R, const int32_t *__restrict__ pos, const int32_t *__restrict__ prev,
                                                         const int32_t *__restrict__ lpos, const int32_t *__restrict__ lfirst, int32_t *__restrict__ out,
                                                         uint8_t *__restrict__ fin)
{
    __shared__ int32_t s_acc[64];
    if (threadIdx.x < 64) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t n = R.n, n1 = n + 1;
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)R.nlast) fin[(int64_t)R.last_b[threadIdx.x] * n1 + prow(n, n)] = (uint8_t)R.fin_stamp;
    for (int pass = 0; pass < (lpos ? 2 : 1); pass++) {
        const int32_t *cp = pass ? lpos : pos, *arr = pass ? lfirst : prev;
        for (int i = 0; i < R.nlast; i++) {                 // (the ranges are nested; together at most 2 N entries)
            const int64_t rb = (n >> R.last_b[i]) << R.last_b[i];
            int32_t c = 0;
            for (int64_t q = (int64_t)cp[rb] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x, q1 = cp[n]; q < q1; q += (int64_t)gridDim.x * blockDim.x) {
                int32_t v = arr[q];
                c += pass ? (v >= rb) : (v < rb);
            }
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_acc[pass * 32 + i], c);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && s_acc[threadIdx.x]) {
        int pass = threadIdx.x >> 5, i = threadIdx.x & 31;
        if (i < R.nlast) atomicAdd(&out[pass * 32 + R.last_b[i]], s_acc[threadIdx.x]);
    }
}

// ------------------------------------------------------------------ task setup
// element 0 of a task is the candidate p = B (its count = anchor + right part); elements i >= 1 are the
// left steps p = B - i.  Round A: B = r is virtual (not a candidate), anchor 0.
__global__ void __launch_bounds__(256) k_setup(RoundDesc R, const int32_t *__restrict__ opt, const int32_t *__restrict__ nnopt,
                                               int32_t *__restrict__ cr, int zero_cr_only,
                                               int4 *__restrict__ tdesc, const int32_t *__restrict__ pos32,
                                               uint8_t *__restrict__ tb, int32_t *__restrict__ len,
                                               const int32_t *__restrict__ nlopt, int32_t *__restrict__ crl, int32_t *__restrict__ tS0l)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R.ntask) return;
    int64_t r; int b;
    decode_task(R, t, r, b);
    int64_t n1 = R.n + 1;
    if (zero_cr_only) { cr[(int64_t)b * n1 + prow((r), n1 - 1)] = 0; if (crl) crl[(int64_t)b * n1 + prow((r), n1 - 1)] = 0; return; }
    int64_t B, a, S0, S0l = 0;
    if (R.isA) {
        B = r; a = r - ((int64_t)1 << b); S0 = 0;           // (zero_cr_only is the only use of this kernel in round A)
    } else {
        int64_t rb = (r >> b) << b;
        int64_t rL = r - ((int64_t)1 << R.tau), rR = r + ((int64_t)1 << R.tau);
        B = opt[(int64_t)b * n1 + prow((rL), n1 - 1)];
        S0 = (int64_t)nnopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + cr[(int64_t)b * n1 + prow((r), n1 - 1)];
        if (tS0l) S0l = (int64_t)nlopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + crl[(int64_t)b * n1 + prow((r), n1 - 1)];
        a = (rR - rb) < ((int64_t)1 << b) ? (int64_t)opt[(int64_t)b * n1 + prow((rR <= R.n ? rR : R.n), n1 - 1)] : rb - ((int64_t)1 << b);
        if (a > B) a = B;          // cannot happen for an inverse-Monge cost; keeps every task well-formed
    }
    tdesc[t] = make_int4((int32_t)B, (int32_t)S0, (int32_t)r, pos32[r]);      // one 16-byte record per task
    tb[t] = (uint8_t)b;
    len[t] = (int32_t)(1 + (B - a));
    if (tS0l) tS0l[t] = (int32_t)S0l;
}

// right part of one round for one counter: rows with ctz == tau stream their 2^tau columns once for all bit planes
static void launch_rpass(hipStream_t s, const RoundDesc &R, int nbits, int64_t n, int64_t rlo, int64_t rhi, const int64_t *cpos,
                         const int32_t *link, int ge, const int32_t *opt, int32_t *cr, double mean_deg)
{
    const int allp = R.G.win;
    int tau = R.tau;
    int64_t rmin = rlo - ((int64_t)1 << tau), rmax = rhi + ((int64_t)1 << tau);
    if (rmax > n) rmax = n;
    if (rmin < 0) rmin = 0;
    // rows (2u+1)<<tau in [rmin, rmax]
    int64_t u0 = rmin <= 0 ? 0 : (((rmin - 1) >> tau) + 1) >> 1;       // #rows < rmin
    int64_t u1 = ((rmax >> tau) + 1) >> 1;                              // #rows <= rmax
    int64_t nrows = u1 - u0;
    if (nrows <= 0) return;
    if (tau <= g_opt_rpass_small_tau) {
        // lane-private share of a row: rpass_cap per cent of the mean number of entries of 2^tau columns, in steps of 16
        int64_t cap = (int64_t)(0.01 * (double)g_opt_rpass_cap * mean_deg * (double)((int64_t)1 << tau));
        cap = std::max<int64_t>(16, std::min<int64_t>((cap + 15) / 16 * 16, 1 << 20));
#define RPS(GE, NB) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rpass_small<GE, NB>), dim3((unsigned)cdiv(nrows, 256)), dim3(256), 0, s, tau, nbits, n, u0, nrows, cpos, link, \
                                       opt, cr, allp, (int)cap)
        // (up to 24 bit planes -- n < 2^24 -- the per-plane registers of the kernels are a quarter fewer: one more wave per SIMD)
        if (nbits <= 24) { if (ge) RPS(true, 24); else RPS(false, 24); }
        else             { if (ge) RPS(true, NBMAX); else RPS(false, NBMAX); }
#undef RPS
    } else {
        int ch_cols = (int)g_opt_rpass_ch;          // columns per wave (cp_set_option("rpass_ch"))
        int64_t cpr = ((int64_t)1 << tau) > ch_cols ? (((int64_t)1 << tau) / ch_cols) : 1;
        if (cpr == 1) ch_cols = 1 << tau;
        int64_t waves = nrows * cpr;
#define RPW(GE, WPB) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rpass_wave<GE, WPB>), dim3((unsigned)cdiv(waves, WPB)), dim3(64 * WPB), 0, s, tau, nbits, n, u0, \
                                        nrows, (int)cpr, ch_cols, cpos, link, opt, cr, allp)
        // the chunks of a row that share a workgroup add up in LDS before the row's counters see them
        if (cpr % 16 == 0)     { if (ge) RPW(true, 16); else RPW(false, 16); }
        else if (cpr % 4 == 0) { if (ge) RPW(true, 4);  else RPW(false, 4); }
        else                   { if (ge) RPW(true, 1);  else RPW(false, 1); }
#undef RPW
    }
}

// The right pass of a tau round, both counters.  (Clearing the counters the chunks of a row add into is the one use the driver
// still has for k_setup.)
template <typename TC, bool HYP>
void right_pass(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    int64_t cols = (((C.n >> R.tau) + 1) >> 1) << R.tau;
    ProfScope ps(PROF_RPASS, s, 4.0 * (C.avg_deg + C.self_deg) * (double)cols + 8.0 * (double)R.ntask);
    if (((int64_t)1 << R.tau) > g_opt_rpass_ch) { // several chunks per row accumulate with atomics: clear first ...
        if (C.cr_consume) g_cr_consume_rounds++;  // ... unless the last layer's set-up left the cells zero (cr_consume: begin_layer)
        else {
            g_cr_clear_launches++;
            hipLaunchKernelGGL(k_setup, dim3((unsigned)cdiv(R.ntask, 256)), dim3(256), 0, s, R, Wk.pl.opt.p, Wk.pl.nnopt.p, Wk.pl.cr.p, 1,
                               Wk.tk.tdesc.p, A->pos32.p, Wk.tk.tb.p, Wk.tk.len.p, (const int32_t *)nullptr, if_hyp<HYP>(Wk.pl.crl.p), (int32_t *)nullptr);
        }
    }
    launch_rpass(s, R, C.nbits, C.n, C.rlo, C.rhi, A->pos.p, A->prev.p, 0, Wk.pl.opt.p, Wk.pl.cr.p, C.avg_deg);                   // prev[q] < B
    if (HYP) launch_rpass(s, R, C.nbits, C.n, C.rlo, C.rhi, A->lpos.p, A->lfirst.p, 1, Wk.pl.opt.p, Wk.pl.crl.p, C.self_deg);      // rows ending in the column with first >= B
}

// round A: the anchors of the last row's tasks in the planes above its lowest bit
template <typename TC, bool HYP>
void last_row_counts(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R)
{
    cp_csr_s *A = C.A;
    CP_HIP(hipMemsetAsync(Wk.pl.last_s0.p, 0, Wk.pl.last_s0.bytes(), C.s));
    hipLaunchKernelGGL(k_last_row_counts, dim3(1024), dim3(256), 0, C.s, R, A->pos32.p, A->prev.p, if_hyp<HYP>(A->lpos32.p), if_hyp<HYP>(A->lfirst.p),
                       Wk.pl.last_s0.p, Wk.pl.fin.p);
}

#define CP_INST(TC, HYP) \
    template void right_pass<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, const RoundDesc &); \
    template void last_row_counts<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, const RoundDesc &);
CP_INST(int64_t, false) CP_INST(int64_t, true) CP_INST(double, false) CP_INST(double, true)
#undef CP_INST

}  // namespace cpk
