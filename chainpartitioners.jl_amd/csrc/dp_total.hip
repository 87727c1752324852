// dp_total.hip -- one layer of the total-cost (g = +) K-part DP in O(n log^2 n) streamed column steps,
// exact to the reference's literal O(n^2) sweep including ties (largest j wins):
//
//     cst[j',k] = min_{1<=j<=j'} cst[j,k-1] + f(j,j',k)        /root/reference/src/DynamicSplitter.jl:33-46
//
// Scheme (executable spec: tests/dc_model.py; derivation: DESIGN.md section 4).  0-based boundary
// positions p = j-1, r = j'-1.
//  * candidates [0,r) of row r split, Fenwick style, into one block per set bit b of r:
//    [r_b - 2^b, r_b), r_b = r with the bits below b cleared.  All rows sharing (b, r_b) form a
//    full rectangle rows (r_b, r_b+2^b) x cols [r_b-2^b, r_b), on which the cost matrix
//    W[p] + f(p,r) is inverse-Monge for the eligible models (coverage counts are submodular), so
//    the RIGHTMOST row argmin is non-increasing in r: a monotone divide and conquer applies.
//  * rows are processed in rounds by tau = ctz(r) (high to low) after a first round for the rows
//    with r == r_b; a row's candidate range [a, B] is bounded by the argmins of its two tree neighbours
//    r - 2^tau (gives B and the anchor count) and r + 2^tau (gives a).
//  * nets(p,r) along the staircase path anchor (B, r-2^tau) -> (B,r) -> (a,r):
//      right part: columns [r-2^tau, r) join a part starting at B: + #{q : prev[q] < B}.  Only the TOTAL is
//        needed, and the same columns serve every set bit b of r (different thresholds B_b): one row-major
//        reduction pass per round (k_rpass_*), N/2 link entries per round.
//      left part: columns p = B-1 .. a join a part ending before r: + #{q in p : next[q] >= r}, one
//        candidate per column.  Per round (k_setup_short -> scan -> k_tile_t0 -> k_lpass -> k_span_short / k_open / k_fix):
//          - tasks with a handful of candidates are finished by one lane in k_setup_short;
//          - the left steps of the other tasks are flattened (1 + B - a elements per task) and cut into 256-step tiles;
//          - a tile that lies inside ONE task (4 of 5 tiles) is one contiguous run of the link array: k_lpass streams
//            it with suffix counts and evaluates it with tile-local counts (the costs are affine in the counts);
//          - the other tiles are counted cooperatively (ballot/popcount per column), segment-scanned with wave
//            shuffles, evaluated and arg-min reduced per task;
//          - tasks spanning tiles are merged by k_span_short (one lane), or k_open + k_fix (work lists).
//  * plane arrays are stored level-major (prow): the rows of one round are contiguous in every plane.
//  * width-windowed layers (candidates max(0, r - w) <= p <= r: the ConstrainedCost DP, DynamicSplitter.jl:206-258) run the same
//    kernels on another tiling of the candidates: every row has a task in every plane b <= floor(log2 w) -- standard, common
//    and mirrored blocks, see struct Geo below and DESIGN.md section 4b.
//
// Units: the right pass is dp_total_rpass.hip, the gap passes are dp_total_gap.hip, the leaf pass and the combine dp_total_leaf.hip;
// the other stages and the layer driver are here.  What the units share: dp_total.hpp.
#include "dp_total.hpp"
#include <optional>

namespace cpk {

// options and statistics of the scheme (cp_set_option / cp_get_stat: capi.hip; declared in dp.hpp)
int64_t g_opt_short_t = 8, g_opt_short_e = 64;
int64_t g_opt_own_min = 64;
int64_t g_opt_own_blk = 1;             // own tiles at absolute 256-column blocks, run in block order; 0: tiles from each task head (k_own_map)
int64_t g_opt_own_split = 1;           // own tiles of the planes >= 8 stream only their plane's variable link entries (SplitLinks); 0: the whole columns
int64_t g_own_split_tiles = 0;
int64_t g_opt_gap_split = 1;           // ... and so do the gap rounds' tiles of those planes (effective while own_split is on)
int64_t g_gap_split_tiles = 0;
int64_t g_opt_own_pair = 1;            // two own tiles per wave outside the gap rounds and the hyperedge costs (k_lpass_own<PAIR>); 0: one
int64_t g_own_pair_waves = 0, g_own_pair_lone = 0;
int64_t g_opt_own_pack = 1;            // split tiles read one packed word per step and plane (SplitLinks::vpk) where the pattern's offsets fit; effective under own_split and own_blk 1
int64_t g_own_pack_tiles = 0, g_own_pack_wide = 0;
int64_t g_opt_rpass_ch = 256;
int64_t g_opt_rpass_small_tau = 4;
int64_t g_opt_force_max = 1024;           // a round's flattened stage is replaced by own tiles when it served at most this many tasks
int64_t g_opt_setup_bs = 1024;          // lanes per block of k_setup_short (a multiple of 64, at most 1024)
int64_t g_opt_rpass_cap = 200;          // lane-private entries per row in k_rpass_small, per cent of the mean
int64_t g_opt_nospec = 0, g_spec_redo = 0;
int64_t g_opt_gap_tau = 6, g_opt_gap_min = 64, g_opt_gap_nr = 2;
int64_t g_opt_ra_cache = 1;
int64_t g_opt_leaf = 1, g_opt_block_tables = 0;
int64_t g_opt_poison = 0, g_poison_hits = 0;
int64_t g_fix_trips = 0, g_fix_edges = 0, g_fix_items = 0;
int64_t g_opt_round_alloc = 1;         // k_setup_short reserves the offsets of its lists with their slots and gives the round's verdict; 0: k_round_scans
int64_t g_round_alloc_rounds = 0;
int64_t g_opt_cr_consume = 1;          // full layers: set-up zeroes the cr / crl cells it reads and the clearing launch in front of the chunked right passes goes (begin_layer)
int64_t g_cr_consume_rounds = 0, g_cr_clear_launches = 0;

// ------------------------------------------------------------------ wave-level segmented scans (64 lanes; the Best helpers: dp_total.hpp)
// inclusive segmented sum: v = sum from the last head at or before this lane (or lane 0), f = "a head lies in [0, lane]"
__device__ __forceinline__ void wave_segsum(int32_t &v, int &f, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int32_t pv = __shfl_up(v, o);
        int pf = __shfl_up(f, o);
        if (lane >= o) { if (!f) v += pv; f |= pf; }
    }
}

template <typename TC, bool HYP>
__device__ __forceinline__ void wave_segmin(Best<TC, HYP> &x, int &f, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        Best<TC, HYP> p;
        best_clear(p);
        p.v = shfl_up64(x.v, o);
        p.p = __shfl_up(x.p, o);
        p.nn = __shfl_up(x.nn, o);
        if (HYP) best_set_nl(p, __shfl_up(best_nl(x), o));
        int pf = __shfl_up(f, o);
        if (lane >= o) { if (!f) x = better(p, x); f |= pf; }
    }
}

// ------------------------------------------------------------------ round_alloc: list slots and offsets reserved together
// cp_set_option("round_alloc", 0 | 1).  A block that appends to a task list holds its tasks' lengths, so it reserves its slots AND
// its range of the list's units (flattened steps / own tiles) with ONE 64-bit atomic, slots << ALLOC_SH | units: both bases come
// from one draw, so a later slot always has a later offset -- the order the binary searches of k_tile_t0 and k_own_map need -- and
// every appended lane writes its task's offset itself: no scan of the lengths afterwards.  (The order across blocks is whatever the
// atomics decide, as it was.)  The last block to arrive (round_alloc_finish) closes the lists and gives the round's verdict.
struct AllocSh {
    unsigned long long wpre[2][16];      // per wave and list: the packed total, then (thread 0) the exclusive prefix inside the block
    int32_t wit[16];                     // ... of the merge items
    unsigned long long base[2];          // what the list's word held before this block's draw
    int32_t ibase;
};

// one wave, one list: `on` lanes append `len` units each.  pre: the units of the wave's appending lanes below this one; returns the
// wave's packed total (the same in every lane)
__device__ __forceinline__ unsigned long long alloc_wave(bool on, int32_t len, int lane, unsigned long long ballot, int32_t &pre)
{
    const int32_t mine = on ? len : 0;
    int32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int32_t v = __shfl_up(inc, o); if (lane >= o) inc += v; }
    pre = inc - mine;
    return ((unsigned long long)__popcll(ballot) << ALLOC_SH) | (unsigned long long)(uint32_t)__shfl(inc, 63);
}

// thread 0, after the barrier behind the waves' totals: the waves' exclusive prefixes, and the block's draws.  The values come
// back while the block does other work; alloc_publish hands them to the block in front of the next barrier.
__device__ __forceinline__ void alloc_reserve(AllocSh &S, int nw, RoundCounts *__restrict__ rc, bool want_items, unsigned long long &b0, unsigned long long &b1,
                                              int32_t &bi)
{
    unsigned long long t0 = 0, t1 = 0; int32_t ti = 0;
    for (int w = 0; w < nw; w++) {
        const unsigned long long c0 = S.wpre[0][w], c1 = S.wpre[1][w]; const int32_t ci = S.wit[w];
        S.wpre[0][w] = t0; S.wpre[1][w] = t1; S.wit[w] = ti; t0 += c0; t1 += c1; ti += ci;
    }
    b0 = t0 ? __hip_atomic_fetch_add(&rc->alloc_l, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    b1 = t1 ? __hip_atomic_fetch_add(&rc->alloc_o, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    bi = (want_items && ti) ? atomicAdd(&rc->n_items, ti) : 0;
}
__device__ __forceinline__ void alloc_publish(AllocSh &S, unsigned long long b0, unsigned long long b1, int32_t bi) { S.base[0] = b0; S.base[1] = b1; S.ibase = bi; }

// an appending lane's slot and offset in list `li` (after the barrier behind alloc_publish)
__device__ __forceinline__ void alloc_place(const AllocSh &S, int li, int wv, int lane, unsigned long long ballot, int32_t pre, int32_t &idx, int64_t &off)
{
    const unsigned long long w = S.base[li] + S.wpre[li][wv];         // (slots and units add up side by side: neither carries into the other, round_alloc_fits)
    idx = (int32_t)(w >> ALLOC_SH) + (int32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    off = (int64_t)(w & ALLOC_MASK) + pre;
}

// Every block, on every path, when its lanes have written their records (the whole block calls it).  The release / ticket / acquire
// hand-off of k_fix_own: the block's stores are complete and released at agent scope before thread 0 draws the ticket; whoever
// draws the last one acquires, reads the two words, writes the closing entries offs[nlong] = T and toffs[nown] = NT, fills the
// counts and gives the verdict (round_verdict: a dropped round reads 0 in T, NT, nlong, nown -- and lists no merge items), then
// puts the ticket back for the next launch.  o_cap: slots of the own list (a count beyond it has set err: nothing is written there).
__device__ __forceinline__ void round_verdict(RoundCounts *__restrict__ rc, int64_t capT, int64_t capNT);
__device__ __forceinline__ void round_alloc_finish(RoundCounts *__restrict__ rc, int64_t *__restrict__ offs, int64_t *__restrict__ toffs, int64_t capT, int64_t capNT,
                                                   int64_t o_cap, uint32_t nblocks)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t got = __hip_atomic_fetch_add(&rc->a_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (got != nblocks - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const unsigned long long al = __hip_atomic_load(&rc->alloc_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long ao = __hip_atomic_load(&rc->alloc_o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t nl = (int64_t)(al >> ALLOC_SH), no = (int64_t)(ao >> ALLOC_SH), T = (int64_t)(al & ALLOC_MASK), NT = (int64_t)(ao & ALLOC_MASK);
    if (no > o_cap) __hip_atomic_store(&rc->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (its lanes have said so already)
    else { offs[nl] = T; if (toffs) toffs[no] = NT; }
    rc->nlong = (int32_t)nl; rc->nown = (int32_t)no;
    __hip_atomic_store(&rc->T, T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&rc->NT, NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    round_verdict(rc, capT, capNT);
    if (__hip_atomic_load(&rc->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) rc->n_items = 0;
    __hip_atomic_store(&rc->alloc_l, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&rc->alloc_o, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&rc->a_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ task setup, second form: short tasks finish here
// One lane per task.  A task with at most `short_t` candidates and at most `short_e` link entries to step over is finished
// by its lane on the spot (at low tau more than half of all tasks have ONE candidate: B == a, nothing to compare); the
// rest are appended -- in order within a block -- to the list of long tasks that the flattened kernels below process.
// (cp_set_option("short_t" / "short_e"): tunables, defaults chosen on config 3.)
template <typename TC, bool HYP>
__global__ void __launch_bounds__(1024) k_setup_short(RoundDesc R, int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt,
                                                      int32_t *__restrict__ cr, int32_t *__restrict__ crl,
                                                      const int32_t *__restrict__ pos32, const int32_t *__restrict__ next,
                                                      const int32_t *__restrict__ fpos32, const int32_t *__restrict__ flast,
                                                      const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                      int4 *__restrict__ tdesc, uint8_t *__restrict__ tb, int32_t *__restrict__ len,
                                                      int32_t *__restrict__ tS0l, int32_t *__restrict__ nlong, int32_t SHORT_T, int32_t SHORT_E,
                                                      int4 *__restrict__ o_tdesc, uint8_t *__restrict__ o_tb, int32_t *__restrict__ o_rlen,
                                                      int32_t *__restrict__ o_ntl, int32_t *__restrict__ o_tS0l, int32_t *__restrict__ n_own,
                                                      unsigned long long *__restrict__ own_steps, int32_t OWN_MIN, int32_t o_cap,
                                                      int32_t *__restrict__ err, const uint8_t *__restrict__ fin, const int32_t *__restrict__ last_s0,
                                                      int32_t *__restrict__ dbg_ntriv, const int32_t *__restrict__ anch, const int32_t *__restrict__ anch2,
                                                      int32_t *__restrict__ pz, int OWN_BLK, int CR_ZERO,
                                                      RoundCounts *arc, int64_t *__restrict__ offs, int64_t *__restrict__ o_toffs,
                                                      int32_t *__restrict__ o_ioffs, int64_t capT, int64_t capNT, int WANT_ITEMS)
{
    // arc (round_alloc: the round's counters, which nlong, n_own, own_steps and err point into; null: the lists are scanned by
    // k_round_scans): see "round_alloc" above -- offs / o_toffs / o_ioffs are written here, the verdict is given by the last block
    // CR_ZERO (cp_set_option("cr_consume", 1), full layers, rounds whose right pass adds a row's counts chunk by chunk): the task's
    // lane is the one reader of its cr / crl cell and leaves it zero for the same round of the next layer -- no clearing launch
    // pz (cp_set_option("poison", 1)): the planes were filled with an out-of-range column before the layer; a task whose bounds
    // come out of range has read a cell nobody wrote -- counted, and clamped so that the task stays well-formed
    int lane = threadIdx.x & 63;
    bool live;
    bool is_long = false, is_own = false, is_short = false;
    int64_t r = 0, B = 0, a = 0, S0 = 0, S0l = 0; int b = 0;
    uint8_t finb = 0;
    if (R.isA) {
        int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        live = t < R.ntask;
        if (live) decode_task(R, t, r, b);
    } else {
        // tau rounds: blockIdx.y is the bit plane (no per-thread search for it), blockIdx.x * 1024 + thread the task inside the plane
        b = R.tau + 1 + (int)blockIdx.y;
        int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        live = l < R.tbase[b + 1] - R.tbase[b];
        if (live) {
            l += R.tskip[b];
            if (R.G.win) r = ((l << 1) | 1) << R.tau;            // windowed layers: every row with ctz == tau, in every plane
            else {
            int sh = b - R.tau - 1;
            int64_t base = l >> sh, v = l & (((int64_t)1 << sh) - 1);
            r = (base << (b + 1)) | ((int64_t)1 << b) | (((v << 1) | 1) << R.tau);
            }
            // (rows of a tau round have ctz == tau: their plane slot needs no bit search)
            // finished by a gap pass of an earlier round?  (the flag is looked at AFTER the gathers below are on their way: one memory latency less)
            if (fin) finb = fin[(int64_t)b * (R.n + 1) + (R.n - (R.n >> R.tau)) + (r >> (R.tau + 1))] == (uint8_t)R.fin_stamp;
        }
    }
    if (live && R.G.win) {
        // windowed geometry: the block of (r, b); round A: the head row of a rectangle scans the whole block below the virtual
        // candidate B = block end, anchor = nets(block end, r) (0 for the standard and common blocks, which end at r; cached per
        // partition for the mirrored ones); round tau: bounds from the tree neighbours inside the row block of 2^b rows
        const int64_t n1 = R.n + 1;
        int64_t cs, ce;
        if (!geo_block(R.G, r, b, cs, ce)) live = false;
        else if (R.isA && R.skip_std && b < R.G.s && ((r >> b) & 1)) live = false;      // (a standard head: done by k_ra_cols)
        else if (R.isA && R.skip_mir && b < R.G.s && !((r >> b) & 1)) live = false;     // (a mirrored head: done by k_ra_layer on the mirrored table)
        else if (R.isA) {
            B = ce; a = cs;
            if (ce != r) { S0 = anch[R.aoff[b] + (r >> (b + 1))]; if (HYP) S0l = anch2[R.aoff[b] + (r >> (b + 1))]; }
        } else {
            const int64_t rL = r - ((int64_t)1 << R.tau), rR = r + ((int64_t)1 << R.tau), rect_hi = ((r >> b) + 1) << b;
            B = opt[(int64_t)b * n1 + prow((rL), n1 - 1)];
            S0 = (int64_t)nnopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + cr[(int64_t)b * n1 + prow((r), n1 - 1)];
            if (HYP) S0l = (int64_t)nlopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + crl[(int64_t)b * n1 + prow((r), n1 - 1)];
            a = (rR < rect_hi && rR <= R.n) ? (int64_t)opt[(int64_t)b * n1 + prow((rR), n1 - 1)] : cs;
            if (a > B) a = B;
        }
    }
    if (live && !R.G.win) {
        int64_t n1 = R.n + 1;
        if (R.isA) {
            // B = r_b is virtual (not a candidate).  Rows r == r_b: nothing lies right of B, anchor 0; the last row n in a
            // plane above its lowest bit: the anchor is the count of the columns [r_b, n) (k_last_row_counts)
            B = (r >> b) << b; a = B - ((int64_t)1 << b);
            if (B != r) { S0 = last_s0[b]; if (HYP) S0l = last_s0[32 + b]; }
        } else {
            int64_t rb = (r >> b) << b;
            int64_t rL = r - ((int64_t)1 << R.tau), rR = r + ((int64_t)1 << R.tau);
            B = opt[(int64_t)b * n1 + prow((rL), n1 - 1)];
            S0 = (int64_t)nnopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + cr[(int64_t)b * n1 + prow((r), n1 - 1)];
            if (HYP) S0l = (int64_t)nlopt[(int64_t)b * n1 + prow((rL), n1 - 1)] + crl[(int64_t)b * n1 + prow((r), n1 - 1)];
            if (CR_ZERO) { cr[(int64_t)b * n1 + prow((r), n1 - 1)] = 0; if (HYP) crl[(int64_t)b * n1 + prow((r), n1 - 1)] = 0; }
            // left end of the range: the winner of the right neighbour -- or, where that lies beyond the matrix, of the last
            // row n (same rectangle; known since round A); the block start for the last row of a rectangle
            a = (rR - rb) < ((int64_t)1 << b) ? (int64_t)opt[(int64_t)b * n1 + prow((rR <= R.n ? rR : R.n), n1 - 1)] : rb - ((int64_t)1 << b);
            if (a > B) a = B;          // cannot happen for an inverse-Monge cost; keeps every task well-formed
        }
    }
    if (finb) live = false;
    if (live && pz && !R.isA && ((uint64_t)B > (uint64_t)R.n || (uint64_t)a > (uint64_t)R.n)) {
        atomicAdd(pz, 1);
        B = B < 0 ? 0 : (B > R.n ? R.n : B); a = a < 0 ? 0 : (a > B ? B : a);
    }
    if (live) {
        int64_t L = 1 + (B - a);
        if (dbg_ntriv && L > 1 && !R.isA) atomicAdd(dbg_ntriv, 1);
        is_short = L <= SHORT_T && (pos32[B] - pos32[a]) <= SHORT_E && (!HYP || (fpos32[B] - fpos32[a]) <= SHORT_E);
        if (is_short) {
        } else if (o_tdesc && L >= OWN_MIN) {
            is_own = true;                           // long enough for tiles of its own (k_lpass_own): every tile is uniform
        } else {
            is_long = true;
        }
    }
    // append the remaining tasks to their list -- the flattened one, or the one of tasks with tiles of their own: ONE atomic per
    // list and 1024-lane block (same-address atomics serialise in L2), order kept inside the block
    __shared__ int32_t s_wcnt[2][16];
    __shared__ unsigned long long s_wsteps[16];
    __shared__ int32_t s_base[2];
    unsigned long long ml = __ballot(is_long), mo = __ballot(is_own);
    int wv = threadIdx.x >> 6;
    int64_t Lmine = is_own ? 1 + (B - a) : 0;
    unsigned long long lsum = 0;
    if (mo) {                                                        // wave-uniform
        lsum = (unsigned long long)Lmine;
        for (int o = 32; o > 0; o >>= 1) lsum += ((unsigned long long)(uint32_t)__shfl_down((int)(lsum >> 32), o) << 32) | (uint32_t)__shfl_down((int)(lsum & 0xffffffffull), o);
    }
    // round_alloc (arc non-null): the lists' offsets are reserved with the slots -- the wave-level prefixes of the appended lengths
    __shared__ AllocSh s_al;
    const int32_t my_ntl = is_own ? own_ntiles(OWN_BLK, B, Lmine) : 0;
    int32_t pre_l = 0, pre_o = 0, pre_i = 0;
    unsigned long long wt_l = 0, wt_o = 0; int32_t wt_i = 0;
    if (arc) {
        if (ml) wt_l = alloc_wave(is_long, (int32_t)(1 + (B - a)), lane, ml, pre_l);              // wave-uniform
        if (mo) {
            wt_o = alloc_wave(is_own, my_ntl, lane, mo, pre_o);
            const int32_t it = WANT_ITEMS ? fix_items_of(my_ntl) : 0;                              // the trips k_own_map lists of the task (gap rounds: none)
            wt_i = (int32_t)(alloc_wave(it > 0, it, lane, 0ull, pre_i) & ALLOC_MASK);
        }
    }
    if (lane == 0) {
        s_wcnt[0][wv] = (int32_t)__popcll(ml); s_wcnt[1][wv] = (int32_t)__popcll(mo); s_wsteps[wv] = lsum;
        if (arc) { s_al.wpre[0][wv] = wt_l; s_al.wpre[1][wv] = wt_o; s_al.wit[wv] = wt_i; }
    }
    __syncthreads();
    int32_t base0 = 0, base1 = 0, abi = 0;
    unsigned long long ab0 = 0, ab1 = 0;
    if (threadIdx.x == 0) {
        int32_t t0 = 0, t1 = 0; unsigned long long st = 0;
        for (int w = 0, nw = (int)(blockDim.x >> 6); w < nw; w++) {
            int32_t c0 = s_wcnt[0][w], c1 = s_wcnt[1][w];
            s_wcnt[0][w] = t0; s_wcnt[1][w] = t1; t0 += c0; t1 += c1; st += s_wsteps[w];
        }
        // (the two list positions come back from L2 while this lane, like all the others, finishes its short task below: the
        //  block used to sit at a barrier for the length of these round trips)
        if (arc) alloc_reserve(s_al, (int)(blockDim.x >> 6), arc, WANT_ITEMS != 0, ab0, ab1, abi);
        else {
            base0 = t0 ? atomicAdd(nlong, t0) : 0;
            base1 = t1 ? atomicAdd(n_own, t1) : 0;
        }
        if (st) atomicAdd(own_steps, st);
    }
    // the short tasks are finished by their lanes -- between the two barriers, while the list positions are on their way
    if (is_short) {
        const int64_t n1 = R.n + 1, L = 1 + (B - a);
        int64_t rw = (int64_t)b * n1 + prow((r), n1 - 1);
        if (L == 1 && !R.isA) {                  // one candidate: nothing to compare
            opt[rw] = (int32_t)B; nnopt[rw] = (int32_t)S0; if (HYP) nlopt[rw] = (int32_t)S0l;
        } else {
            // The walk is a chain of dependent loads (the kernel spends 2/3 of its wave cycles waiting on memory): the column pointer and
            // the previous-layer cost of the NEXT candidate are requested before the current column is stepped over, and a column's
            // entries go eight at a time -- one memory latency per candidate instead of four or five.
            const int32_t rr = (int32_t)r, posr = pos32[r];
            int64_t nn = S0, nl = S0l;
            Best<TC, HYP> best; best_clear(best);
            int32_t pp = pos32[B], pq = 0, fp = HYP ? fpos32[B] : 0, fq = 0;      // colptr of the candidate (pp, fp) and of the column after it (pq, fq)
            TC wp = W[B];
            for (int64_t i = 0; i < L; i++) {    // decreasing p: an earlier candidate wins ties
                const int64_t p = B - i;
                int32_t pn = 0, fn = 0; TC wn = (TC)0;
                if (i + 1 < L) { pn = pos32[p - 1]; wn = W[p - 1]; if (HYP) fn = fpos32[p - 1]; }
                if (i > 0) {                     // step over column p: its entries are [pp, pq)
                    for (int32_t q = pp; q < pq; q += 8) {
                        int32_t v[8];
#pragma unroll
                        for (int k = 0; k < 8; k++) v[k] = q + k < pq ? next[q + k] : -1;
#pragma unroll
                        for (int k = 0; k < 8; k++) nn += (v[k] >= rr);
                    }
                    if (HYP) for (int32_t q = fp; q < fq; q++) nl += (flast[q] < rr);
                }
                if (!(i == 0 && R.isA)) {        // (round A: p = r is not a candidate)
                    TC fv = dm_apply_affine(M, alpha, r - p, (int64_t)(posr - pp), nn, nl);
                    Best<TC, HYP> c; best_clear(c); c.v = cadd(wp, fv); c.p = (int32_t)p; c.nn = (int32_t)nn; best_set_nl(c, (int32_t)nl);
                    best = better(best, c);
                }
                pq = pp; pp = pn; wp = wn; fq = fp; fp = fn;
            }
            opt[rw] = best.p; nnopt[rw] = best.nn; if (HYP) nlopt[rw] = best_nl(best);
        }
    }
    if (threadIdx.x == 0) { s_base[0] = base0; s_base[1] = base1; if (arc) alloc_publish(s_al, ab0, ab1, abi); }
    __syncthreads();
    if (is_long) {
        int32_t idx = s_base[0] + s_wcnt[0][wv] + __popcll(ml & ((1ull << lane) - 1ull));
        if (arc) { int64_t off; alloc_place(s_al, 0, wv, lane, ml, pre_l, idx, off); offs[idx] = off; }
        tdesc[idx] = make_int4((int32_t)B, (int32_t)S0, (int32_t)r, pos32[r]);
        tb[idx] = (uint8_t)b;
        len[idx] = (int32_t)(1 + (B - a));
        if (HYP) tS0l[idx] = (int32_t)S0l;
    }
    if (is_own) {
        int32_t idx = s_base[1] + s_wcnt[1][wv] + __popcll(mo & ((1ull << lane) - 1ull));
        int64_t off = 0;
        if (arc) alloc_place(s_al, 1, wv, lane, mo, pre_o, idx, off);
        if (idx >= o_cap) *err = 1;                      // (an own task is never short) cannot happen (LayerWork sizes the list for the worst case); never write outside
        else {
            o_tdesc[idx] = make_int4((int32_t)B, (int32_t)S0, (int32_t)r, pos32[r]);
            o_tb[idx] = (uint8_t)b;
            o_rlen[idx] = (int32_t)Lmine;
            o_ntl[idx] = my_ntl;
            if (HYP) o_tS0l[idx] = (int32_t)S0l;
            if (arc) { o_toffs[idx] = off; if (WANT_ITEMS) o_ioffs[idx] = s_al.ibase + s_al.wit[wv] + pre_i; }
        }
    }
    // (every block draws its ticket, whatever its lanes met)
    if (arc) round_alloc_finish(arc, offs, o_toffs, capT, capNT, (int64_t)o_cap, gridDim.x * gridDim.y);
}

// ------------------------------------------------------------------ tile task table (one wave = one tile)
// first task overlapping each tile: last t with offs[t] <= tile*LT (one thread per tile; offs[0] = 0)
__global__ void __launch_bounds__(256) k_tile_t0(const RoundCounts *__restrict__ rc, const int64_t *__restrict__ offs,
                                                 const int4 *__restrict__ tdesc, int64_t *__restrict__ tile_t0, int4 *__restrict__ tile_rec, int no_interior,
                                                 int64_t *__restrict__ taskR)
{
    const int64_t ntask = rc->nlong, ntile = rc->ntile, T = rc->T;
    for (int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tile < ntile; tile += (int64_t)gridDim.x * blockDim.x) {
    taskR[tile] = -1;                                  // "no task continues beyond this tile" until k_lpass says otherwise
    int64_t tile_start = tile * LT;
    int64_t lo = 0, hi = ntask;
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= tile_start) lo = mid; else hi = mid;
    }
    tile_t0[tile] = lo;
    // interior tile: every step belongs to ONE task whose head lies in an earlier tile.  Record {first column, row, pos[row], 1}.
    int64_t toff = offs[lo], nx = offs[lo + 1], tend = tile_start + LT < T ? tile_start + LT : T;
    int4 rec = make_int4(0, 0, 0, 0);
    if (toff < tile_start && nx >= tend && !no_interior) {
        int4 td = tdesc[lo];
        rec = make_int4(td.x - (int32_t)(tile_start - toff), td.z, td.w, 1);
    }
    tile_rec[tile] = rec;
    }
}

// loads the offsets (relative to the tile start, 32-bit) of the tasks overlapping the tile and a bitmap of the
// task heads inside it
__device__ __forceinline__ void load_tile_tasks(const int64_t *__restrict__ offs, int64_t ntask, int64_t t0, int64_t tile_start,
                                                bool active, int32_t *s_off, unsigned long long *s_hd, int lane, int &cnt)
{
    int64_t c = ntask - t0;                  // every task has len >= 1: at most LT tasks start inside the tile
    cnt = active ? (int)(c > LT + 1 ? LT + 1 : c) : 0;
    if (lane < LT / 64) s_hd[lane] = 0ull;
    for (int i = lane; i < cnt; i += 64) {
        int64_t rel = offs[t0 + i] - tile_start;
        if (rel < -(int64_t)0x3fffffff) rel = -(int64_t)0x3fffffff;
        if (rel > (int64_t)0x3fffffff) rel = (int64_t)0x3fffffff;
        s_off[i] = (int32_t)rel;
        if (rel >= 0 && rel < LT) atomicOr(&s_hd[rel >> 6], 1ull << (rel & 63));
    }
}

// ------------------------------------------------------------------ cooperative column counts
// Every lane owns one column-like range [s, en) of `arr` and a threshold; lanes whose ranges are adjacent and
// descending form a run whose entries [q_lo, q_hi) are read as aligned 16-byte-per-lane loads (1 KiB per wave
// instruction, two in flight); position x + 4*lane' + j sits in component j of lane'.  Returns, per lane,
// #{entries of its range with  v >= thr (GE)  or  v < thr (!GE)}.  One ballot pass per distinct threshold
// (= task) touching a 256-entry block.
template <bool GE>
__device__ __forceinline__ int32_t coop_count(const int32_t *__restrict__ arr, int32_t s, int32_t en, int32_t thr, bool valid, int lane)
{
    int32_t prev_s = __shfl_up(s, 1);
    int prev_valid = __shfl_up((int)valid, 1);
    bool cont = valid && lane > 0 && prev_valid && (en == prev_s);
    unsigned long long heads = __ballot(valid && !cont);
    unsigned long long vm = __ballot(valid);
    int32_t d = 0;
    const int32_t FILL = GE ? INT32_MIN : INT32_MAX;          // never counted
    while (heads) {
        int h0 = __ffsll((long long)heads) - 1;
        heads &= heads - 1;
        int h1 = heads ? (__ffsll((long long)heads) - 1) : 64;
        unsigned long long inrun = vm & (h1 == 64 ? ~0ull : ((1ull << h1) - 1)) & ~((1ull << h0) - 1);
        int hl = 63 - __clzll((long long)inrun);          // last valid lane of the run
        int32_t q_hi = __shfl(en, h0), q_lo = __shfl(s, hl);
        bool mine = lane >= h0 && lane <= hl && en > s;
        for (int32_t x = q_lo & ~3; x < q_hi; x += 512) {
            int4 v0 = make_int4(FILL, FILL, FILL, FILL), v1 = v0;
            int32_t b0 = x + 4 * lane, b1 = b0 + 256;
            if (b0 < q_hi) v0 = *reinterpret_cast<const int4 *>(arr + b0);        // arrays are padded by 8 entries
            if (b1 < q_hi) v1 = *reinterpret_cast<const int4 *>(arr + b1);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                int32_t xc = x + c * 256;
                if (xc >= q_hi) break;                    // wave-uniform
                int4 v = c ? v1 : v0;
                // (entries outside the run need no masking: a lane only counts inside its own range, which lies in the run)
                bool ov = mine && s < xc + 256 && en > xc;
                // this lane's range covers positions [a0, a1) of the block: lanes [lo_j, hi_j) of component j
                int a0 = ov ? ((s > xc ? s : xc) - xc) : 0, a1 = ov ? ((en < xc + 256 ? en : xc + 256) - xc) : 0;
                unsigned long long rem = __ballot(ov);
                while (rem) {                             // one pass per distinct threshold touching the block
                    int l = __ffsll((long long)rem) - 1;
                    int32_t tu = __shfl(thr, l);
                    const bool f0 = GE ? v.x >= tu : v.x < tu, f1 = GE ? v.y >= tu : v.y < tu, f2 = GE ? v.z >= tu : v.z < tu, f3 = GE ? v.w >= tu : v.w < tu;
                    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2), m3 = __ballot(f3);
                    // F(x) = flagged entries at block positions < x = (flags in the lanes below lane x/4) + (flags of that lane below
                    // component x%4): the lane-below counts come from v_mbcnt chains, packed with the lane's own flags, and a lane
                    // takes  F(a1) - F(a0)  for its range [a0, a1) with two cross-lane reads
                    uint32_t P0 = 0;
                    P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, P0));
                    P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, P0));
                    P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, P0));
                    P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m3, P0));
                    const int32_t pack = (int32_t)((P0 << 3) | (uint32_t)f0 | ((uint32_t)f1 << 1) | ((uint32_t)f2 << 2));
                    const int32_t tot = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);         // (uniform)
                    const int32_t g0 = __shfl(pack, (a0 >> 2) & 63), g1 = __shfl(pack, (a1 >> 2) & 63);      // (every lane takes part)
                    bool same = ov && thr == tu;
                    if (same) {
                        int32_t F0 = (g0 >> 3) + __popc((uint32_t)g0 & ((1u << (a0 & 3)) - 1u));
                        int32_t F1 = a1 >= 256 ? tot : (g1 >> 3) + __popc((uint32_t)g1 & ((1u << (a1 & 3)) - 1u));
                        d += F1 - F0;
                    }
                    rem &= ~__ballot(same);
                }
            }
        }
    }
    return d;
}

// Interior tiles of a long task: the tile's steps e = 0 .. tl are adjacent descending columns p_first - e of ONE task, so
// the step order is the (reversed) entry order of one contiguous run [Q_lo, Q_hi) and the inclusive step prefix is a
// suffix count:  x(e) = #{q in [s(e), Q_hi) : flagged(q)},  s(e) = first entry of the step's column.  No per-column
// counts, no wave scan, no carry.  The run is streamed once in 256-entry blocks (two blocks per trip; the next trip's two loads
// are issued at the top of a trip and waited for at the top of the next one); per block: four ballots, a per-lane popcount prefix, and one gather per step whose column starts
// inside the block.  Lane l owns the steps l, l+64, l+128, l+192.
// DET (gap passes, see k_gap_finish): the entries of the run with a value strictly between sp_lo and sp_hi ("specials") are
// appended to the wave's list by the lanes that hold them (LDS counter s_cnt): s_es[i] = the entry's position (the caller turns it
// into the first step whose candidate has the entry's column on its right), s_v[i] = the value, tagged with `kind` in bit 31.
// Only the first SMAX specials are stored; s_cnt keeps counting.
// (Tried: a step's count taken once, in the block its column starts in, as TOTAL - (flagged entries below the start), the groups
//  that can start in a block picked on the scalar side -- 30 instead of 70 vector instructions per block, but 65 VGPRs: 254 ms
//  against 232; forced back to 64 VGPRs: 241 ms.)
// (Tried: the link values in 3 bytes (n < 2^24), a 12-byte load and six vector instructions to unpack four entries -- 19 % fewer
//  bytes per step, and k_lpass_own 9 % SLOWER (254 vs 232 ms per partition): at 0.8 of the HBM roofline the kernel has no vector
//  issue slots to spare.)
// PK (own_pack; own_split tiles of the geometry own_blk 1, which lie inside one 256-column block): cpos is the plane's packed words
// (SplitLinks::vpk), one load per step -- the column's start and its prefix sum as 16-bit offsets from the block's bases vb[0]; vb[1]
// holds the next block's.  A tile that is not a head tile ends at the block's last column: its run ends, and its prefix sums are
// taken from, the next block's bases; a head tile's are the offsets of its column p_first.  psum is not read.
template <bool GE, bool DET = false, bool PK = false>
__device__ __forceinline__ void interior_stream(const int32_t *__restrict__ arr, const int32_t *__restrict__ cpos, int32_t p_first, int32_t tl,
                                                int32_t thr, int lane, int32_t acc[4], int32_t sk[4], int head = 0, int32_t sp_lo = 0, int32_t sp_hi = 0,
                                                int32_t *s_es = nullptr, int32_t *s_v = nullptr, int32_t *s_cnt = nullptr, int kind = 0,
                                                const int32_t *__restrict__ psum = nullptr, const int2 *__restrict__ vb = nullptr)
{
    // No load of this function sits under a lane mask or a data-dependent branch: behind the join of a conditional load the
    // compiler cannot tell how many loads are outstanding and waits for all of them, which made every guarded load a round trip
    // of its own.  Indices are clamped into the tile instead and the guards are selects on the loaded values.
    // The tile is the wave's: its column, its length and the run's two ends are scalars, so every address below is a scalar base
    // plus a small unsigned lane offset (one VGPR, no 64-bit vector arithmetic; the masks tell the compiler how small).
    p_first = __builtin_amdgcn_readfirstlane(p_first);
    tl = __builtin_amdgcn_readfirstlane(tl) & 255;
    // Prologue, one group of loads: the column pointers of the lane's four steps (a step beyond tl reads the tile's last column),
    // the run's two ends, and with psum (wave-uniform; own_split) what a step starts from: psum[end of the run's columns] -
    // psum[its column], what the columns hold apart from the streamed entries.  (The counters are live through the loop anyway.)
    const int32_t *__restrict__ cl = cpos + (p_first - tl), *__restrict__ pl = (psum ? psum : cpos) + (p_first - tl);      // the tile's last column
    int32_t cp[4], pv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int32_t e = lane + 64 * k;
        const uint32_t d = (uint32_t)(tl - (e < tl ? e : tl)) & 255u;
        cp[k] = cl[d];
        if (!PK) pv[k] = pl[d];
    }
    int32_t Q_hi, Q_lo;
    if constexpr (PK) {
        // the same group: the words of column p_first and of the tile's last column, and the two base pairs (adjacent scalars)
        const uint32_t wt = (uint32_t)__builtin_amdgcn_readfirstlane(cl[tl]), wl = (uint32_t)__builtin_amdgcn_readfirstlane(cl[0]);
        const int2 b0 = vb[0], b1 = vb[1];
        Q_hi = head ? b0.x + (int32_t)(wt & 0xffffu) : b1.x;
        Q_lo = b0.x + (int32_t)(wl & 0xffffu);
        const int32_t ptop = head ? (int32_t)(wt >> 16) : b1.y - b0.y;              // (relative to the block's base, like the steps')
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool on = lane + 64 * k <= tl;
            sk[k] = on ? b0.x + (int32_t)((uint32_t)cp[k] & 0xffffu) : INT32_MAX;
            acc[k] = on ? ptop - (int32_t)((uint32_t)cp[k] >> 16) : 0;
        }
    } else {
    // head != 0: step 0 is the candidate p_first itself (no column stepped over): the run ends in front of that column
    const int32_t ptop = pl[tl + 1 - head];
    Q_hi = __builtin_amdgcn_readfirstlane(cl[tl + 1 - head]); Q_lo = __builtin_amdgcn_readfirstlane(cl[0]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool on = lane + 64 * k <= tl;
        sk[k] = on ? cp[k] : INT32_MAX;
        acc[k] = (psum && on) ? ptop - pv[k] : 0;
    }
    }
    // Entries: a lane whose four positions start at or above Q_hi reads the run's last aligned quad instead -- inside the eight
    // entries of slack behind every streamed array (next: ensure_links, flast: ensure_self, + 16; vnext: split_build, + 8) -- and
    // what it reads is never flagged: every block that is not `inner` guards its flags by position, an inner one holds run entries only.
    const int32_t x_end = Q_hi & ~3;
    int32_t x = Q_lo & ~3;
    // (x <= x_end wherever this is called: the offset from the trip's first entry is unsigned and below 1024 or x_end - x)
    auto quad = [&](uint32_t o) { const uint32_t r = (uint32_t)(x_end - x); return *reinterpret_cast<const int4 *>(arr + x + (o < r ? o : r)); };
    int4 c0 = quad(4 * lane), c1 = quad(256 + 4 * lane);
    for (; x < Q_hi; x += 512) {
        // the next 512 entries are issued before the current ones are touched: the wait below them is for c0 / c1 only
        const int4 n0 = quad(512 + 4 * lane), n1 = quad(768 + 4 * lane);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int32_t xc = x + c * 256;
            if (xc >= Q_hi) break;                        // wave-uniform
            int4 v = c ? c1 : c0;
            int32_t pb = xc + 4 * lane;
            // entries at or above Q_hi belong to columns above the tile: never flagged (those below Q_lo lie below every s)
            // the lane's four flags, and the four wave masks
            // (a block that lies inside the run -- all but the first and the last one -- needs none of the position guards: wave-uniform)
            const bool inner = xc >= Q_lo && xc + 256 <= Q_hi;
            bool f0 = GE ? v.x >= thr : v.x < thr, f1 = GE ? v.y >= thr : v.y < thr, f2 = GE ? v.z >= thr : v.z < thr, f3 = GE ? v.w >= thr : v.w < thr;
            if (!inner) { f0 = f0 && pb < Q_hi; f1 = f1 && pb + 1 < Q_hi; f2 = f2 && pb + 2 < Q_hi; f3 = f3 && pb + 3 < Q_hi; }
            const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2), m3 = __ballot(f3);
            if (DET) {
                const uint32_t span = (uint32_t)(sp_hi - sp_lo - 1);           // v in (sp_lo, sp_hi)  <=>  (uint)(v - sp_lo - 1) < span
                bool s0 = (uint32_t)(v.x - sp_lo - 1) < span, s1 = (uint32_t)(v.y - sp_lo - 1) < span, s2 = (uint32_t)(v.z - sp_lo - 1) < span,
                     s3 = (uint32_t)(v.w - sp_lo - 1) < span;
                if (!inner) {
                    s0 = s0 && pb >= Q_lo && pb < Q_hi; s1 = s1 && pb + 1 >= Q_lo && pb + 1 < Q_hi;
                    s2 = s2 && pb + 2 >= Q_lo && pb + 2 < Q_hi; s3 = s3 && pb + 3 >= Q_lo && pb + 3 < Q_hi;
                }
                if (s0 || s1 || s2 || s3) {                           // rare; only the lanes holding a special work here
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3) {
                            int32_t val = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
                            int slot = atomicAdd(s_cnt, 1);
                            if (slot <= SMAX - 1) {
                                s_es[slot] = pb + j;                  // (the position; its column is looked up after the stream: no load stalls the loop)
                                s_v[slot] = (int32_t)(((uint32_t)val & 0x7fffffffu) | ((uint32_t)kind << 31));
                            }
                        }
                    }
                }
            }
            int32_t tot = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);                       // uniform
            // flagged entries in the lanes below this one (v_mbcnt chains), packed with the lane's own first three flags: one
            // cross-lane read then gives a step everything it needs about the lane its column starts in
            uint32_t P0 = 0;
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m3, P0));
            const int32_t pack = (int32_t)((P0 << 3) | (uint32_t)f0 | ((uint32_t)f1 << 1) | ((uint32_t)f2 << 2));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int32_t idx = sk[k] - xc;                 // block position of the step's first entry (huge for invalid steps)
                bool inside = idx > 0 && idx < 256;
                if (__ballot(inside)) {                   // wave-uniform: some column of this group starts inside the block
                    int32_t cidx = inside ? idx : 0;
                    int src = cidx >> 2, comp = cidx & 3;
                    const int32_t g = __shfl(pack, src);
                    int32_t Fb = (g >> 3) + __popc((uint32_t)g & ((1u << comp) - 1u));        // flagged entries of the block below position idx
                    acc[k] += idx <= 0 ? tot : (inside ? tot - Fb : 0);
                } else {
                    acc[k] += idx <= 0 ? tot : 0;
                }
            }
        }
        c0 = n0; c1 = n1;
    }
}

// The same stream in parts, for the second tile of a wave with two (k_lpass_own<PAIR>): its stages leave while the first tile is at
// work -- tile_head_loads (the prologue's loads, untouched) next to the first tile's, then behind the first tile's stream
// tile_counters (counters, the run's ends) and tile_first (the first two blocks), then tile_trips (the loop).  The first tile, like
// every one-tile wave, goes through interior_stream itself.  (interior_stream written as these four in a row computes the same,
// but the compiler then lets the first trip's prefetch share a register with the second block and waits for the first two blocks
// before it sends the prefetch: one round trip more per tile of more than one trip, 1 % on the windowed layers.  So the one-tile
// form keeps its own text, and its code is what it was.)
struct TileHead { int32_t cp[4], pv[4], ptop, qhi, qlo; int2 b0, b1; };      // (PK: cp the packed words, ptop / qlo those of column p_first / the last column, b0 / b1 the bases)
struct TileRun { int32_t Q_lo, Q_hi, x, x_end; int4 c0, c1; };

template <bool PK = false>
__device__ __forceinline__ void tile_head_loads(TileHead &h, const int32_t *__restrict__ cpos, const int32_t *__restrict__ psum, int32_t p_first, int32_t tl,
                                                int head, int lane, const int2 *__restrict__ vb = nullptr)
{
    // Prologue, one group of loads: the column pointers of the lane's four steps (a step beyond tl reads the tile's last column),
    // the run's two ends, and with psum (wave-uniform; own_split) what a step starts from: psum[end of the run's columns] -
    // psum[its column], what the columns hold apart from the streamed entries.  (The counters are live through the loop anyway.)
    const int32_t *__restrict__ cl = cpos + (p_first - tl), *__restrict__ pl = (psum ? psum : cpos) + (p_first - tl);      // the tile's last column
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int32_t e = lane + 64 * k;
        const uint32_t d = (uint32_t)(tl - (e < tl ? e : tl)) & 255u;
        h.cp[k] = cl[d];
        if (!PK) h.pv[k] = pl[d];
    }
    if constexpr (PK) {                // (see interior_stream)
        h.ptop = cl[tl];
        h.qlo = cl[0];
        h.b0 = vb[0]; h.b1 = vb[1];
        return;
    }
    // head != 0: step 0 is the candidate p_first itself (no column stepped over): the run ends in front of that column
    h.ptop = pl[tl + 1 - head];
    h.qhi = cl[tl + 1 - head];
    h.qlo = cl[0];
}

// Entries: a lane whose four positions start at or above Q_hi reads the run's last aligned quad instead -- inside the eight
// entries of slack behind every streamed array (next: ensure_links, flast: ensure_self, + 16; vnext: split_build, + 8) -- and
// what it reads is never flagged: every block that is not `inner` guards its flags by position, an inner one holds run entries only.
// (x <= x_end wherever this is called: the offset from the trip's first entry is unsigned and below 1024 or x_end - x)
__device__ __forceinline__ int4 tile_quad(const int32_t *__restrict__ arr, int32_t x, int32_t x_end, uint32_t o)
{
    const uint32_t r = (uint32_t)(x_end - x);
    return *reinterpret_cast<const int4 *>(arr + x + (o < r ? o : r));
}

template <bool PK = false>
__device__ __forceinline__ void tile_counters(const TileHead &h, int32_t tl, int lane, bool psum, int32_t acc[4], int32_t sk[4], TileRun &r, int head = 0)
{
    if constexpr (PK) {
        const uint32_t wt = (uint32_t)__builtin_amdgcn_readfirstlane(h.ptop), wl = (uint32_t)__builtin_amdgcn_readfirstlane(h.qlo);
        r.Q_hi = head ? h.b0.x + (int32_t)(wt & 0xffffu) : h.b1.x;
        r.Q_lo = h.b0.x + (int32_t)(wl & 0xffffu);
        const int32_t ptop = head ? (int32_t)(wt >> 16) : h.b1.y - h.b0.y;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool on = lane + 64 * k <= tl;
            sk[k] = on ? h.b0.x + (int32_t)((uint32_t)h.cp[k] & 0xffffu) : INT32_MAX;
            acc[k] = on ? ptop - (int32_t)((uint32_t)h.cp[k] >> 16) : 0;
        }
    } else {
    r.Q_hi = __builtin_amdgcn_readfirstlane(h.qhi);
    r.Q_lo = __builtin_amdgcn_readfirstlane(h.qlo);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool on = lane + 64 * k <= tl;
        sk[k] = on ? h.cp[k] : INT32_MAX;
        acc[k] = (psum && on) ? h.ptop - h.pv[k] : 0;
    }
    }
    r.x_end = r.Q_hi & ~3;
    r.x = r.Q_lo & ~3;
}

__device__ __forceinline__ void tile_first(const int32_t *__restrict__ arr, int lane, TileRun &r)
{
    r.c0 = tile_quad(arr, r.x, r.x_end, 4 * lane);
    r.c1 = tile_quad(arr, r.x, r.x_end, 256 + 4 * lane);
}

template <bool GE, bool DET = false>
__device__ __forceinline__ void tile_trips(const int32_t *__restrict__ arr, TileRun &r, int32_t thr, int lane, int32_t acc[4], const int32_t sk[4],
                                           int32_t sp_lo = 0, int32_t sp_hi = 0, int32_t *s_es = nullptr, int32_t *s_v = nullptr, int32_t *s_cnt = nullptr,
                                           int kind = 0)
{
    const int32_t Q_lo = r.Q_lo, Q_hi = r.Q_hi, x_end = r.x_end;
    int32_t x = r.x;
    int4 c0 = r.c0, c1 = r.c1;
    for (; x < Q_hi; x += 512) {
        // the next 512 entries are issued before the current ones are touched: the wait below them is for c0 / c1 only
        const int4 n0 = tile_quad(arr, x, x_end, 512 + 4 * lane), n1 = tile_quad(arr, x, x_end, 768 + 4 * lane);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int32_t xc = x + c * 256;
            if (xc >= Q_hi) break;                        // wave-uniform
            int4 v = c ? c1 : c0;
            int32_t pb = xc + 4 * lane;
            // entries at or above Q_hi belong to columns above the tile: never flagged (those below Q_lo lie below every s)
            // the lane's four flags, and the four wave masks
            // (a block that lies inside the run -- all but the first and the last one -- needs none of the position guards: wave-uniform)
            const bool inner = xc >= Q_lo && xc + 256 <= Q_hi;
            bool f0 = GE ? v.x >= thr : v.x < thr, f1 = GE ? v.y >= thr : v.y < thr, f2 = GE ? v.z >= thr : v.z < thr, f3 = GE ? v.w >= thr : v.w < thr;
            if (!inner) { f0 = f0 && pb < Q_hi; f1 = f1 && pb + 1 < Q_hi; f2 = f2 && pb + 2 < Q_hi; f3 = f3 && pb + 3 < Q_hi; }
            const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2), m3 = __ballot(f3);
            if (DET) {
                const uint32_t span = (uint32_t)(sp_hi - sp_lo - 1);           // v in (sp_lo, sp_hi)  <=>  (uint)(v - sp_lo - 1) < span
                bool s0 = (uint32_t)(v.x - sp_lo - 1) < span, s1 = (uint32_t)(v.y - sp_lo - 1) < span, s2 = (uint32_t)(v.z - sp_lo - 1) < span,
                     s3 = (uint32_t)(v.w - sp_lo - 1) < span;
                if (!inner) {
                    s0 = s0 && pb >= Q_lo && pb < Q_hi; s1 = s1 && pb + 1 >= Q_lo && pb + 1 < Q_hi;
                    s2 = s2 && pb + 2 >= Q_lo && pb + 2 < Q_hi; s3 = s3 && pb + 3 >= Q_lo && pb + 3 < Q_hi;
                }
                if (s0 || s1 || s2 || s3) {                           // rare; only the lanes holding a special work here
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3) {
                            int32_t val = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
                            int slot = atomicAdd(s_cnt, 1);
                            if (slot <= SMAX - 1) {
                                s_es[slot] = pb + j;                  // (the position; its column is looked up after the stream: no load stalls the loop)
                                s_v[slot] = (int32_t)(((uint32_t)val & 0x7fffffffu) | ((uint32_t)kind << 31));
                            }
                        }
                    }
                }
            }
            int32_t tot = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);                       // uniform
            // flagged entries in the lanes below this one (v_mbcnt chains), packed with the lane's own first three flags: one
            // cross-lane read then gives a step everything it needs about the lane its column starts in
            uint32_t P0 = 0;
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, P0));
            P0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m3, P0));
            const int32_t pack = (int32_t)((P0 << 3) | (uint32_t)f0 | ((uint32_t)f1 << 1) | ((uint32_t)f2 << 2));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int32_t idx = sk[k] - xc;                 // block position of the step's first entry (huge for invalid steps)
                bool inside = idx > 0 && idx < 256;
                if (__ballot(inside)) {                   // wave-uniform: some column of this group starts inside the block
                    int32_t cidx = inside ? idx : 0;
                    int src = cidx >> 2, comp = cidx & 3;
                    const int32_t g = __shfl(pack, src);
                    int32_t Fb = (g >> 3) + __popc((uint32_t)g & ((1u << comp) - 1u));        // flagged entries of the block below position idx
                    acc[k] += idx <= 0 ? tot : (inside ? tot - Fb : 0);
                } else {
                    acc[k] += idx <= 0 ? tot : 0;
                }
            }
        }
        c0 = n0; c1 = n1;
    }
}


// ------------------------------------------------------------------ long tasks with tiles of their own
// A task with >= OWN_MIN steps gets tiles of its own: every tile lies in one task, so all of them -- head and tail included --
// take the uniform path: one contiguous run of the link array, suffix counts, tile-local evaluation.  k_own_map: tile ->
// (task, tile index inside the task); k_lpass_own: one wave per tile; k_fix_own: one lane per short task, one block per trip of a longer one merges the tiles
// (adding the counts made before each tile).  Tile ids are task-major, the head tile first.  Two geometries (own_ntiles / own_tile_geo):
//   blk = 1 (default, cp_set_option("own_blk")): one tile per 256-column block floor(p / LT) the task's candidates [a, B] touch
//           (the head and the tail tile partial: at most one tile more than cdiv(L, LT)).  k_own_map counts the tiles of every
//           block, a scan and k_blk_order sort the tile ids by block, and k_lpass_own runs them in that order: the four waves
//           of a workgroup mostly stream the same block's entries for different tasks (the bit planes of the round) at the
//           same time, and all but the first find them in the caches.
//   blk = 0: tiles counted from the task's own head, LT steps each (the last one partial), in task order.
// bcnt (blk = 1): tiles per column block, and each tile's rank inside its block (brank)
// items (outside the gap rounds): the work list of the merge, k_fix_own -- one item {task, first tile} per trip of FIX_TRIP tiles of
// every task of more than FIX_SERIAL tiles, appended by the trip's first tile (a wave-aggregated atomic on rc->n_items; a dropped
// round walks no tiles and lists nothing); item_of[that tile] = the item's index, by which the merge finds a task's trips in order.
__global__ void __launch_bounds__(256) k_own_map(RoundCounts *__restrict__ rc, const int64_t *__restrict__ toffs, const int4 *__restrict__ tdesc,
                                                 const int32_t *__restrict__ rlen, int4 *__restrict__ rec, int32_t *__restrict__ tile_task,
                                                 const uint8_t *__restrict__ tb, int32_t *__restrict__ gap_hi, int tau, int64_t n, int blk,
                                                 int32_t *__restrict__ bcnt, int32_t *__restrict__ brank, int2 *__restrict__ items,
                                                 int32_t *__restrict__ item_of, int split, const int32_t *__restrict__ ioffs)
{
    // ioffs (round_alloc): set-up reserved every task's items, trip j of task t is item ioffs[t] + j -- computed, not drawn: no
    // same-address atomic per wave, no item_of; rc->n_items holds their number already
    const int64_t ntask = rc->nown, ntile = rc->NT;
    for (int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tile < ntile; tile += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = ntask;                       // last task with toffs[task] <= tile
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (toffs[mid] <= tile) lo = mid; else hi = mid;
    }
    int32_t kt = (int32_t)(tile - toffs[lo]);
    if (items && ioffs) {
        if (kt % FIX_TRIP == 0 && toffs[lo + 1] - toffs[lo] > FIX_SERIAL) items[ioffs[lo] + kt / FIX_TRIP] = make_int2((int32_t)lo, kt);
    } else if (items) {
        const bool first = kt % FIX_TRIP == 0 && toffs[lo + 1] - toffs[lo] > FIX_SERIAL;
        const unsigned long long mf = __ballot(first);      // (the lanes still in the loop)
        if (mf) {
            const int lane = threadIdx.x & 63, lead = __ffsll((long long)mf) - 1;
            int32_t base = 0;
            if (lane == lead) base = atomicAdd(&rc->n_items, (int32_t)__popcll(mf));
            base = __shfl(base, lead);
            if (first) {
                const int32_t it = base + __popcll(mf & ((1ull << lane) - 1ull));
                items[it] = make_int2((int32_t)lo, kt);
                item_of[tile] = it;
            }
        }
    }
    int4 td = tdesc[lo];
    int32_t pf, tl;
    own_tile_geo(blk, td.x, rlen[lo], kt, pf, tl);
    // {column of step 0, row, pos[row], split plane (bits 10 ..; 0: the tile streams the whole columns) | tl (8 bits) | tile of a gap task | head}
    const bool isgap = gap_hi != nullptr;
    const int sb = (split && tb[lo] >= SPLIT_BMIN) ? tb[lo] : 0;
    rec[tile] = make_int4(pf, td.z, td.w, (sb << 10) | (tl << 2) | (isgap ? 2 : 0) | (kt == 0 ? 1 : 0));
    if (split == 2) {                                  // (a launch that also holds tiles of the planes below: counted here, one atomic per wave)
        const unsigned long long ms = __ballot(sb != 0);
        if (ms && (int)(threadIdx.x & 63) == __ffsll((long long)ms) - 1) atomicAdd(&rc->n_split, (int32_t)__popcll(ms));
    }
    tile_task[tile] = (int32_t)lo;
    if (bcnt) brank[tile] = atomicAdd(&bcnt[pf / LT], 1);
    if (isgap) {                                       // gap pass: rows (r - 2^tau, hi) of the rectangle are finished together
        int64_t r = td.z, b = tb[lo];
        int64_t hi = r + ((int64_t)1 << tau), re = (((r >> b) + 1) << b);
        if (hi > re) hi = re;
        if (hi > n + 1) hi = n + 1;
        gap_hi[tile] = (int32_t)hi;
    }
    }
}

// the counting sort's scatter: the tiles of column block c are border[bstart[c] .. bstart[c + 1]).  The counts have been scanned
// by now; the tile's record goes to the same slot of srec; and the tile of rank 0 of every block that has tiles puts its block's count back to zero: bcnt is all zero between
// rounds without a clearing pass (k_own_map and this kernel walk the same rc->NT tiles).
__global__ void __launch_bounds__(256) k_blk_order(const RoundCounts *__restrict__ rc, const int4 *__restrict__ rec, const int32_t *__restrict__ brank,
                                                   const int64_t *__restrict__ bstart, int32_t *__restrict__ border, int4 *__restrict__ srec,
                                                   int32_t *__restrict__ bcnt)
{
    const int64_t ntile = rc->NT;
    for (int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tile < ntile; tile += (int64_t)gridDim.x * blockDim.x) {
        const int4 r = rec[tile];
        const int32_t c = r.x / LT, rk = brank[tile];
        const int64_t slot = bstart[c] + rk;
        border[slot] = (int32_t)tile;
        srec[slot] = r;                                // (by value: the wave that runs the slot reads its record without the tile id)
        if (rk == 0) bcnt[c] = 0;
    }
}

// The tile's own winner (k_lpass_own outside the gap passes): candidates from the lane's four steps, then the wave arg-min.
// sk: the pin positions of the steps, wv: W of the candidates, acc / acc2: the counts; lane 0 holds the result.
template <typename TC, bool HYP>
__device__ __forceinline__ void own_tile_cands(Best<TC, HYP> cand[4], const int4 rec, int32_t tl, int head, int isA, const DevModel<TC> &M, TC alpha, int lane,
                                               const int32_t acc[4], const int32_t acc2[4], const int32_t sk[4], const TC wv[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int32_t e = lane + 64 * k;
        best_clear(cand[k]);
        if (e <= tl && !(head && isA && e == 0)) {     // round A: the head element p = r is not a candidate
            int32_t p = rec.x - e;
            TC fv = dm_apply_affine(M, alpha, (int64_t)(rec.y - p), (int64_t)(rec.z - sk[k]), (int64_t)acc[k], (int64_t)acc2[k]);
            cand[k].v = cadd(wv[k], fv); cand[k].p = p; cand[k].nn = acc[k]; best_set_nl(cand[k], acc2[k]);
        }
    }
}

template <typename TC, bool HYP>
__device__ __forceinline__ Best<TC, HYP> own_tile_winner(const Best<TC, HYP> cand[4], int lane)
{
    Best<TC, HYP> best; best_clear(best);
#pragma unroll
    for (int k = 0; k < 4; k++) best = better(best, cand[k]);       // increasing e = decreasing p: an earlier candidate wins ties
    for (int o = 32; o > 0; o >>= 1) {              // wave arg-min; ties -> larger p
        int src = (lane + o) & 63;
        Best<TC, HYP> c; best_clear(c); c.v = shfl64(best.v, src); c.p = __shfl(best.p, src); c.nn = __shfl(best.nn, src);
        if (HYP) best_set_nl(c, __shfl(best_nl(best), src));
        bool take = (best.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < best.v || (c.v == best.v && c.p > best.p)));
        if (lane + o < 64 && take) best = c;
    }
    return best;
}

// cp_set_option("own_pair"): the two slots of the run order wave w takes.  false: no slot is left for the wave.  A wave whose
// second slot lies beyond the order takes its first one again (s1 == s0: it loads what it has loaded, and stores once).
__host__ __device__ __forceinline__ bool own_pair_slots(int64_t w, int64_t nt, int64_t &s0, int64_t &s1)
{
    s0 = 2 * w;
    s1 = 2 * w + 1 < nt ? 2 * w + 1 : s0;
    return w >= 0 && s0 < nt;
}

// border, a_srec (blk = 1): the tile ids and their records in column-block order; wave k takes tile border[k], whose record is a_srec[k]
// PAIR (own_pair; neither GAP nor HYP): wave k takes the slots 2k and 2k + 1 of that order.
// PK (own_pack; not HYP): the split tiles of the launch take the packed words of their plane and the bases of their block
// (interior_stream<PK>): a_vpos is SplitLinks::vpk then and a_vsa is SplitLinks::vbase (pairs; stride: the blocks of vstride columns
// + 1) -- the argument list, and with it the code of the other instantiations, is what it was.  PAIR: every tile of the launch is split (own_stream).
template <typename TC, bool HYP, bool GAP, bool PAIR = false, bool PK = false>
__global__ void __launch_bounds__(256) k_lpass_own(int isA, const RoundCounts *__restrict__ rc, const int32_t *__restrict__ border,
                                                   const int32_t *__restrict__ a_pos, const int32_t *__restrict__ a_next,
                                                   const int32_t *__restrict__ a_fpos, const int32_t *__restrict__ a_flast,
                                                   int32_t *__restrict__ a_tileS, int32_t *__restrict__ a_tileS2, const int4 *__restrict__ a_rec,
                                                   const int4 *__restrict__ a_srec, const TC *__restrict__ W, DevModel<TC> M, TC alpha, Best<TC, HYP> *__restrict__ part,
                                                   int tau, const int32_t *__restrict__ gap_hi, uint8_t *__restrict__ spec, int force_spec,
                                                   Best<TC, HYP> *__restrict__ sub, int32_t *__restrict__ spv,
                                                   const int32_t *__restrict__ a_col, const int32_t *__restrict__ a_ffirst,
                                                   const int32_t *__restrict__ a_vnext, const int32_t *__restrict__ a_vpos,
                                                   const int32_t *__restrict__ a_vsa, int64_t vstride)
{
    // GAP (rounds tau <= gap_tau, see k_gap_finish): the tile is evaluated for ALL rows r' of (r - 2^tau, hi) at once: the counts
    // taken here are those of the entries every such row counts (next >= hi - 1; last <= r - 2^tau), the candidates are valued
    // with the task's own row (the rows differ by terms that do not depend on the candidate), and `spec` says whether the tile
    // holds an entry that only some of the rows count.
    // (Tried: tiles visited in column order, one contiguous share of the order per XCD, so that the ~10 passes of the bit planes
    //  over a column meet in L2: 10 % off this kernel, less than the sort of the tile list costs.  The block order of own_blk is a
    //  counting sort by 256-column block (k_own_map, one scan, k_blk_order): 4 % off, and the sort is paid.  Staging each block's
    //  entries once per round in LDS for all its tiles (one workgroup per block) was 23 % slower: DESIGN.md section 6b.)
    // (No grid-stride loop here.  The host launches one wave per tile -- PAIR: per two tiles -- of the buffer's CAPACITY, which
    //  the round's verdict (k_round_scans) has checked the true count against.  A loop over tiles cost 14 VGPRs when the body
    //  held 58 and that meant two waves per SIMD; since the grouped loads <long,false,false> holds 42, and PAIR spends the room on
    //  a second tile whose stages leave with the first one's: DESIGN.md section 6.)
    int lane = threadIdx.x & 63;
    if constexpr (PAIR && !HYP && !GAP) {
        // Two tiles, A and B, of any two tasks, planes and blocks: everything of a tile is scalar per tile.  Both records leave
        // together, then both prologues; A streams as a one-tile wave does (interior_stream; what B's prologue brought waits in 11
        // VGPRs); A's end group (pin positions, W) and B's first two blocks leave together and A is evaluated and stored under
        // them; B streams, then its end group and evaluation.  Of B's four exposed round trips outside its trips three are gone.  (Tried: B's first blocks issued with A's, and A evaluated
        // after B's stream, so that A's end group hides too: 71 VGPRs = seven waves per SIMD; held to 64 it spills.)
        // A lone wave (the order ends at A) runs A twice and a scalar branch keeps it from storing twice.
        int64_t s0, s1;
        if (!own_pair_slots((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), rc->NT, s0, s1)) return;
        const bool lone = s1 == s0;

        // A model whose pin coefficient is zero multiplies the pin count by it: its lanes all read the pin position of the tile's
        // last column instead (one line, not four: 4 of a step's ~25 bytes) -- a count >= 0 like the true one, so the product is
        // the same zero, bit for bit; the load stays where it is, unconditional.
        const uint32_t pinm = M.p[CP_P_PIN] != (TC)0 ? 255u : 0u;
        const int4 vA = border ? a_srec[s0] : a_rec[s0], vB = border ? a_srec[s1] : a_rec[s1];
        int64_t tA = s0, tB = s1;
        if (border) { tA = border[s0]; tB = border[s1]; }
        const int4 rA = make_int4(__builtin_amdgcn_readfirstlane(vA.x), __builtin_amdgcn_readfirstlane(vA.y), __builtin_amdgcn_readfirstlane(vA.z),
                                  __builtin_amdgcn_readfirstlane(vA.w));
        const int4 rB = make_int4(__builtin_amdgcn_readfirstlane(vB.x), __builtin_amdgcn_readfirstlane(vB.y), __builtin_amdgcn_readfirstlane(vB.z),
                                  __builtin_amdgcn_readfirstlane(vB.w));
        const int hdA = rA.w & 1, hdB = rB.w & 1;
        const int32_t tlA = (rA.w >> 2) & 255, tlB = (rB.w >> 2) & 255;
        const int sbA = rA.w >> 10, sbB = rB.w >> 10;                    // (own_split: the plane, or 0 -- one tile of a pair may be split, the other not)
        const int64_t soA = sbA ? (int64_t)(sbA - SPLIT_BMIN) * vstride : 0, soB = sbB ? (int64_t)(sbB - SPLIT_BMIN) * vstride : 0;
        const int32_t *__restrict__ arrA = (PK || sbA) ? a_vnext : a_next, *__restrict__ arrB = (PK || sbB) ? a_vnext : a_next;
        TileHead hB;
        TileRun uB;
        int32_t accA[4], accB[4], skA[4], skB[4];
        const int32_t zero4[4] = {0, 0, 0, 0};
        if constexpr (PK) {
            const int64_t vbstride = ((vstride + 255) >> 8) + 1;
            const int2 *__restrict__ a_vbase = reinterpret_cast<const int2 *>(a_vsa);
            const int2 *__restrict__ vbA = a_vbase + (int64_t)(sbA - SPLIT_BMIN) * vbstride + (rA.x >> 8);
            const int2 *__restrict__ vbB = a_vbase + (int64_t)(sbB - SPLIT_BMIN) * vbstride + (rB.x >> 8);
            tile_head_loads<true>(hB, a_vpos + soB, nullptr, rB.x, tlB, hdB, lane, vbB);
            interior_stream<true, false, true>(a_vnext, a_vpos + soA, rA.x, tlA, rA.y, lane, accA, skA, hdA, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, vbA);
            tile_counters<true>(hB, tlB, lane, true, accB, skB, uB, hdB);
        } else {
        tile_head_loads(hB, sbB ? a_vpos + soB : a_pos, sbB ? a_vsa + soB : (const int32_t *)nullptr, rB.x, tlB, hdB, lane);
        interior_stream<true>(arrA, sbA ? a_vpos + soA : a_pos, rA.x, tlA, rA.y, lane, accA, skA, hdA, 0, 0, nullptr, nullptr, nullptr, 0,
                              sbA ? a_vsa + soA : (const int32_t *)nullptr);
        tile_counters(hB, tlB, lane, sbB != 0, accB, skB, uB);
        }
        TC wv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int32_t e = lane + 64 * k;
            const uint32_t d = (uint32_t)(tlA - (e < tlA ? e : tlA)) & 255u;
            skA[k] = (a_pos + (rA.x - tlA))[d & pinm];
            wv[k] = (W + (rA.x - tlA))[d];
        }
        tile_first(arrB, lane, uB);
        Best<TC, HYP> cand[4];
        {
            const int sel = tlA >> 6;
            if (lane == (tlA & 63)) a_tileS[tA] = sel == 0 ? accA[0] : sel == 1 ? accA[1] : sel == 2 ? accA[2] : accA[3];
            own_tile_cands<TC, HYP>(cand, rA, tlA, hdA, isA, M, alpha, lane, accA, zero4, skA, wv);
            const Best<TC, HYP> best = own_tile_winner<TC, HYP>(cand, lane);
            if (lane == 0) part[tA] = best;
        }
        tile_trips<true>(arrB, uB, rB.y, lane, accB, skB);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int32_t e = lane + 64 * k;
            const uint32_t d = (uint32_t)(tlB - (e < tlB ? e : tlB)) & 255u;
            skB[k] = (a_pos + (rB.x - tlB))[d & pinm];
            wv[k] = (W + (rB.x - tlB))[d];
        }
        if (lone) return;
        {
            const int sel = tlB >> 6;
            if (lane == (tlB & 63)) a_tileS[tB] = sel == 0 ? accB[0] : sel == 1 ? accB[1] : sel == 2 ? accB[2] : accB[3];
            own_tile_cands<TC, HYP>(cand, rB, tlB, hdB, isA, M, alpha, lane, accB, zero4, skB, wv);
            const Best<TC, HYP> best = own_tile_winner<TC, HYP>(cand, lane);
            if (lane == 0) part[tB] = best;
        }
        return;
    }
    int64_t tile = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= rc->NT) return;
    // (own_blk: k_blk_order left the record next to the tile id, in the order the waves run: one level of loads, not two)
    const int4 vrec = border ? a_srec[tile] : a_rec[tile];
    if (border) tile = border[tile];
    // (the record is the wave's: its words as scalars -- the addresses made from them are scalar bases, and five VGPRs fewer)
    const int32_t rw = __builtin_amdgcn_readfirstlane(vrec.w);
    const int4 rec = make_int4(__builtin_amdgcn_readfirstlane(vrec.x), __builtin_amdgcn_readfirstlane(vrec.y), __builtin_amdgcn_readfirstlane(vrec.z), rw);
    int head = rw & 1;
    int32_t tl = (rw >> 2) & 255;
    int32_t acc[4], acc2[4] = {0, 0, 0, 0}, sk[4], sk2[4];
    __shared__ int32_t s_es_all[4][2][SMAX + 1], s_v_all[4][2][SMAX + 1];      // the wave's specials: as found / sorted by step
    __shared__ int32_t s_cnt_all[4];
    int32_t(*s_es)[SMAX + 1] = s_es_all[threadIdx.x >> 6], (*s_v)[SMAX + 1] = s_v_all[threadIdx.x >> 6];
    int ns = 0;
    if (GAP && (rw & 2)) {
        int32_t *s_cnt = &s_cnt_all[threadIdx.x >> 6];
        if (lane == 0) *s_cnt = 0;
        __threadfence_block();
        int32_t rL = rec.y - (1 << tau), hi1 = gap_hi[tile] - 1;
        // gap_split (k_own_map put the plane into the record, as for the other rounds): the classification of SplitLinks holds for a
        // gap task of plane b -- its rows (rL, hi) lie in the rectangle's rows, thr = hi - 1 and the special interval (rL, hi - 1) in
        // the sibling block's range -- so an entry below the plane is neither counted nor special, one above it is counted by every
        // row and never special (the prefix difference the stream starts its counters from), and only the plane's variable entries
        // are compared and tested
        const int sb = HYP ? 0 : rw >> 10;                               // (scalar: the arrays stay scalar operands)
        const int64_t so = sb ? (int64_t)(sb - SPLIT_BMIN) * vstride : 0;
        if constexpr (PK) {            // (wave-uniform: the plane-7 tiles of the launch stream the whole columns)
            if (sb) interior_stream<true, true, true>(a_vnext, a_vpos + so, rec.x, tl, hi1, lane, acc, sk, head, rL, hi1, s_es[0], s_v[0], s_cnt, 0, nullptr,
                                                      reinterpret_cast<const int2 *>(a_vsa) + (int64_t)(sb - SPLIT_BMIN) * (((vstride + 255) >> 8) + 1) + (rec.x >> 8));
            else interior_stream<true, true>(a_next, a_pos, rec.x, tl, hi1, lane, acc, sk, head, rL, hi1, s_es[0], s_v[0], s_cnt, 0);
        } else
        interior_stream<true, true>(sb ? a_vnext : a_next, sb ? a_vpos + so : a_pos, rec.x, tl, hi1, lane, acc, sk, head, rL, hi1, s_es[0], s_v[0], s_cnt, 0,
                                    sb ? a_vsa + so : (const int32_t *)nullptr);
        if (HYP) interior_stream<false, true>(a_flast, a_fpos, rec.x, tl, rL + 1, lane, acc2, sk2, head, rL, hi1, s_es[0], s_v[0], s_cnt, 1);
        __threadfence_block();
        ns = *s_cnt;
        if (force_spec) ns = SMAX + 1;
        if (ns > 0 && ns <= SMAX) {                     // positions -> steps: first step whose candidate has the entry's column on its right
            if (HYP) {
                if (lane < ns) {
                    const int32_t q = s_es[0][lane];
                    const bool k1 = s_v[0][lane] < 0;   // (bit 31: an entry of the second list)
                    s_es[0][lane] = rec.x - (k1 ? a_ffirst[q] : a_col[q]);
                }
            } else {
                // ... = the number of the tile's steps whose column starts above the position, from the starts the wave holds (sk: of
                // the streamed array, whichever it is).  Empty columns have equal starts: the entry's column is the LARGEST one that
                // starts at or below it.  (At most SMAX rounds of four ballots, in the rare tile with specials; no array, no load.)
                int32_t es = 0;
                for (int i = 0; i < ns; i++) {
                    const int32_t q = s_es[0][i];       // (uniform)
                    int32_t c = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) c += (int32_t)__popcll(__ballot(lane + 64 * k <= tl && sk[k] > q));
                    if (lane == i) es = c;
                }
                __threadfence_block();
                if (lane < ns) s_es[0][lane] = es;
            }
            __threadfence_block();
        }
        if (!HYP) {                                     // (the pin count wants the column's own position: what sk holds unless the tile is split; reloaded either way)
#pragma unroll
            for (int k = 0; k < 4; k++) { const int32_t e = lane + 64 * k; sk[k] = (a_pos + (rec.x - tl))[(uint32_t)(tl - (e < tl ? e : tl)) & 255u]; }
        }
    } else if (!HYP && !GAP) {
        // own_split (k_own_map put the plane into the record): only the plane's variable entries are streamed; the entries every
        // row of the rectangle counts are a difference of prefix sums per step (the stream starts its counters from it), and the pin
        // count wants the column's own position
        const int sb = rw >> 10;                                         // (scalar: the arrays stay scalar operands)
        const int64_t so = sb ? (int64_t)(sb - SPLIT_BMIN) * vstride : 0;
        if constexpr (PK) {            // (wave-uniform: tiles of the planes below SPLIT_BMIN stream the whole columns)
            if (sb) interior_stream<true, false, true>(a_vnext, a_vpos + so, rec.x, tl, rec.y, lane, acc, sk, head, 0, 0, nullptr, nullptr, nullptr, 0, nullptr,
                                                       reinterpret_cast<const int2 *>(a_vsa) + (int64_t)(sb - SPLIT_BMIN) * (((vstride + 255) >> 8) + 1) + (rec.x >> 8));
            else interior_stream<true>(a_next, a_pos, rec.x, tl, rec.y, lane, acc, sk, head);
        } else
        interior_stream<true>(sb ? a_vnext : a_next, sb ? a_vpos + so : a_pos, rec.x, tl, rec.y, lane, acc, sk, head, 0, 0, nullptr, nullptr, nullptr, 0,
                              sb ? a_vsa + so : (const int32_t *)nullptr);
        // (a_pos is what the stream's sk holds when the tile is not split: reloaded either way, in one group with W below)
#pragma unroll
        for (int k = 0; k < 4; k++) { const int32_t e = lane + 64 * k; sk[k] = (a_pos + (rec.x - tl))[(uint32_t)(tl - (e < tl ? e : tl)) & 255u]; }
    } else {
        interior_stream<true>(a_next, a_pos, rec.x, tl, rec.y, lane, acc, sk, head);
        if (HYP) interior_stream<false>(a_flast, a_fpos, rec.x, tl, rec.y, lane, acc2, sk2, head);
    }
    // end of the wave, one group of loads: W of the lane's four candidates (and the pin positions above), at steps clamped into
    // the tile; the evaluation selects afterwards
    TC wv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { const int32_t e = lane + 64 * k; wv[k] = (W + (rec.x - tl))[(uint32_t)(tl - (e < tl ? e : tl)) & 255u]; }
    int sel = tl >> 6;
    if (lane == (tl & 63)) {
        a_tileS[tile] = sel == 0 ? acc[0] : sel == 1 ? acc[1] : sel == 2 ? acc[2] : acc[3];
        if (HYP) a_tileS2[tile] = sel == 0 ? acc2[0] : sel == 1 ? acc2[1] : sel == 2 ? acc2[2] : acc2[3];
    }
    // tile-local evaluation (the costs are affine in the counts; k_fix_own adds the counts made before the tile)
    Best<TC, HYP> cand[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int32_t e = lane + 64 * k;
        best_clear(cand[k]);
        if (e <= tl && !(head && isA && e == 0)) {     // round A: the head element p = r is not a candidate
            int32_t p = rec.x - e;
            TC fv = dm_apply_affine(M, alpha, (int64_t)(rec.y - p), (int64_t)(rec.z - sk[k]), (int64_t)acc[k], (int64_t)acc2[k]);
            cand[k].v = cadd(wv[k], fv); cand[k].p = p; cand[k].nn = acc[k]; best_set_nl(cand[k], acc2[k]);
        }
    }
    if (GAP && ns > SMAX) {                             // too many specials: k_gap_finish walks the tile entry by entry
        if (lane == 0) spec[tile] = 255;
        return;
    }
    if (!GAP || ns == 0) {                              // one winner
        Best<TC, HYP> best; best_clear(best);
#pragma unroll
        for (int k = 0; k < 4; k++) best = better(best, cand[k]);       // increasing e = decreasing p: an earlier candidate wins ties
        for (int o = 32; o > 0; o >>= 1) {              // wave arg-min; ties -> larger p
            int src = (lane + o) & 63;
            Best<TC, HYP> c; best_clear(c); c.v = shfl64(best.v, src); c.p = __shfl(best.p, src); c.nn = __shfl(best.nn, src);
            if (HYP) best_set_nl(c, __shfl(best_nl(best), src));
            bool take = (best.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < best.v || (c.v == best.v && c.p > best.p)));
            if (lane + o < 64 && take) best = c;
        }
        if (lane == 0) { part[tile] = best; if (GAP) spec[tile] = 0; }
        return;
    }
    // GAP with specials: they cut the tile into segments of candidates that see the same specials on their right; every
    // segment keeps a winner of its own (the rows weigh the segments differently): one segmented arg-min scan.
    __threadfence_block();                              // (lane 0 wrote the list)
    if (lane < ns) {                                    // sort by step: rank = number of specials in front
        int32_t es_i = s_es[0][lane]; int rank = 0;
        for (int j = 0; j < ns; j++) { int32_t es_j = s_es[0][j]; rank += (es_j < es_i) || (es_j == es_i && j < lane); }
        s_es[1][rank] = es_i; s_v[1][rank] = s_v[0][lane];
    }
    __threadfence_block();
    int seg[4] = {0, 0, 0, 0}, hd[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ns; i++) {
        int32_t es_i = s_es[1][i];                      // (uniform)
#pragma unroll
        for (int k = 0; k < 4; k++) { seg[k] += (es_i <= lane + 64 * k); hd[k] |= (es_i == lane + 64 * k); }
    }
    if (lane == 0) hd[0] = 1;
    const int64_t sbase = tile * (SMAX + 1);
    if (lane <= ns) {                                   // segments without a candidate (two specials at one step, a special at step 0)
        int32_t lo = lane == 0 ? 0 : s_es[1][lane - 1], hi = lane == ns ? tl + 1 : s_es[1][lane];
        if (hi <= lo) { Best<TC, HYP> z; best_clear(z); sub[sbase + lane] = z; }
    }
    Best<TC, HYP> bcarry; best_clear(bcarry);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int32_t e = lane + 64 * k;
        Best<TC, HYP> x = cand[k];
        int f = hd[k];
        wave_segmin<TC, HYP>(x, f, lane);
        if (!f) x = better(bcarry, x);
        {
            Best<TC, HYP> nb; best_clear(nb); nb.v = shfl64(x.v, 63); nb.p = __shfl(x.p, 63); nb.nn = __shfl(x.nn, 63);
            if (HYP) best_set_nl(nb, __shfl(best_nl(x), 63));
            bcarry = nb;
        }
        int nh = __shfl_down(hd[k], 1), nh0 = __shfl(hd[k + 1], 0);
        if (lane == 63) nh = nh0;
        if (e <= tl && (e == tl || nh)) sub[sbase + seg[k]] = x;       // the last candidate of a segment holds its winner
    }
    if (lane < ns) spv[sbase + lane] = s_v[1][lane];
    if (lane == 0) spec[tile] = (uint8_t)ns;
}

// Merging the tiles of a task, one launch (k_fix_own), the role of a block chosen by its index.  The counts made before a tile
// are the task's anchor plus the counts of the task's earlier tiles (tileS, written by k_lpass_own) -- sums inside ONE task, so no
// device-wide prefix over the round's tiles is made for them.  (The gap rounds do make one: k_gap_finish and its helpers look
// tiles up at random.)
//   lane blocks: one LANE per task; up to FIX_SERIAL tiles are merged by the lane with a running sum, longer tasks are left to
//   item blocks: one BLOCK per item {task, first tile} of the list k_own_map made: a trip of FIX_TRIP tiles, merged with the
//     trip-LOCAL exclusive prefix as base (the trip's first tile: 0).  The costs are affine in the counts, so what the task's
//     earlier trips counted adds the same amount to every candidate of the trip: neither the order nor the ties inside the trip
//     depend on it.  A task of one trip is finished by its block (anchor added to the winner).  Otherwise the block leaves a
//     record {winner, the trip's counts} and draws a ticket of its task; whoever draws the last one folds the task: the records in
//     trip order, a running base from the anchor on, each trip winner raised by its base through the same fix_merge arithmetic
//     (sums of integers below 2^53 / wrapping Int64: adding the base in two steps is exact) and compared by the same rule --
//     smaller value, then larger p, a total order: the winner does not depend on who finishes when.  The folder puts the ticket
//     back to zero (no clearing pass between rounds: the b_cnt pattern of k_blk_order).  No block waits for another one.
//     Records cross XCDs: written with agent-scope stores, released at agent scope before the ticket is drawn, read by the
//     folder behind an agent-scope acquire with agent-scope loads (never from a stale L1 / L2 line).
// (Tried: k_lpass_own writing the winner of a single-tile task itself -- the dependent loads at the end of every wave cost it
//  more than the merge saves.)
template <typename TC, bool HYP>
__device__ __forceinline__ void fix_merge(Best<TC, HYP> &acc, Best<TC, HYP> c, int64_t base, int64_t base2, const DevModel<TC> &M)
{
    if (c.p >= 0) {
        c.v = cadd(c.v, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, base, base2));
        c.nn = (int32_t)(c.nn + base);
        if (HYP) best_set_nl(c, (int32_t)(best_nl(c) + base2));
    }
    bool take = (acc.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < acc.v || (c.v == acc.v && c.p > acc.p)));
    if (take) acc = c;
}

template <typename TC> __device__ __forceinline__ unsigned long long fix_bits(TC v);
template <> __device__ __forceinline__ unsigned long long fix_bits<int64_t>(int64_t v) { return (unsigned long long)v; }
template <> __device__ __forceinline__ unsigned long long fix_bits<double>(double v) { return (unsigned long long)__double_as_longlong(v); }
template <typename TC> __device__ __forceinline__ TC fix_val(unsigned long long w);
template <> __device__ __forceinline__ int64_t fix_val<int64_t>(unsigned long long w) { return (int64_t)w; }
template <> __device__ __forceinline__ double fix_val<double>(unsigned long long w) { return __longlong_as_double((long long)w); }

template <typename TC, bool HYP>
__device__ __forceinline__ void best_wave_min(Best<TC, HYP> &acc, int lane)      // lane 0 ends with the wave's winner
{
    for (int o = 32; o > 0; o >>= 1) {
        int src = (lane + o) & 63;
        Best<TC, HYP> c; best_clear(c); c.v = shfl64(acc.v, src); c.p = __shfl(acc.p, src); c.nn = __shfl(acc.nn, src);
        if (HYP) best_set_nl(c, __shfl(best_nl(acc), src));
        bool take = (acc.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < acc.v || (c.v == acc.v && c.p > acc.p)));
        if (lane + o < 64 && take) acc = c;
    }
}

// grid: `iblocks` item blocks (grid stride over rc->n_items), then the lane blocks (grid stride over rc->nown)
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_fix_own(RoundCounts *__restrict__ rc, const int64_t *__restrict__ toffs, const Best<TC, HYP> *__restrict__ part,
                                                 const int4 *__restrict__ tdesc, const uint8_t *__restrict__ tb, const int32_t *__restrict__ tS0l,
                                                 const int32_t *__restrict__ tileS, const int32_t *__restrict__ tileS2, DevModel<TC> M,
                                                 int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt, int64_t n1,
                                                 const int2 *__restrict__ items, const int32_t *__restrict__ item_of,
                                                 unsigned long long *__restrict__ trec, uint32_t *__restrict__ tick, int iblocks,
                                                 const int32_t *__restrict__ ioffs)
{
    // ioffs (round_alloc): trip j of task t is item ioffs[t] + j; null: item_of[the trip's first tile], as k_own_map drew it
    __shared__ Best<TC, HYP> s_part[4];
    __shared__ int64_t s_w[4], s_w2[4];
    __shared__ int64_t s_pre[FIX_TRIP], s_pre2[HYP ? FIX_TRIP : 1];      // per tile of the trip: the counts since its wave's first tile
    // (The lane blocks carry these 16 / 32 KB without using them: static LDS is per kernel.  A dozen lane blocks per round -- the
    //  allocation limits nothing there.)
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)blockIdx.x >= iblocks) {
        // ---- lane blocks
        const int64_t ntask = rc->nown;
        const int64_t nlb = (int64_t)gridDim.x - iblocks;
        for (int64_t t0 = ((int64_t)blockIdx.x - iblocks) * blockDim.x; t0 < ntask; t0 += nlb * blockDim.x) {      // wave-uniform
            int64_t t = t0 + threadIdx.x;
            int64_t k0 = 0, k1 = 0;
            if (t < ntask) { k0 = toffs[t]; k1 = toffs[t + 1]; }
            int64_t nt = k1 - k0;
            const unsigned long long e1 = __ballot(nt == 1), e2 = __ballot(nt == FIX_SERIAL), e3 = __ballot(nt == FIX_SERIAL + 1);
            if (lane == 0) {
                const int32_t em = (e1 ? 1 : 0) | (e2 ? 2 : 0) | (e3 ? 4 : 0);
                if (em & ~rc->n_edge) atomicOr(&rc->n_edge, em);
            }
            if (nt < 1 || nt > FIX_SERIAL) continue;
            int4 td = tdesc[t];
            int64_t run = td.y, run2 = HYP ? (int64_t)tS0l[t] : 0;     // the counts made before tile k
            Best<TC, HYP> acc; best_clear(acc);
            for (int64_t k = k0; k < k1; k++) {                        // (the winner does not depend on the order: larger p wins ties)
                fix_merge<TC, HYP>(acc, part[k], run, run2, M);
                run += tileS[k];
                if (HYP) run2 += tileS2[k];
            }
            int64_t rw = (int64_t)tb[t] * n1 + prow(((int64_t)td.z), n1 - 1);
            opt[rw] = acc.p; nnopt[rw] = acc.nn;
            if (HYP) nlopt[rw] = best_nl(acc);
        }
        return;
    }
    // ---- item blocks
    // (In every round the last row of the top rectangle owns a task over its whole block -- tens of thousands of tiles, a dozen
    //  trips and more: as one block's serial walk that task alone set the length of the launch.)
    const int64_t nlist = rc->n_items;
    for (int64_t i = blockIdx.x; i < nlist; i += iblocks) {          // block-uniform: the barriers below are reached by the whole block
        const int2 it = items[i];
        const int64_t t = it.x;
        const int64_t k0 = toffs[t], k1 = toffs[t + 1], kt = k0 + it.y;
        Best<TC, HYP> acc; best_clear(acc);
        // the 16-byte partials: lane x takes the tiles x, x + 256, ... of the trip (neighbouring lanes, neighbouring records)
        Best<TC, HYP> cc[FIX_U];
#pragma unroll
        for (int u = 0; u < FIX_U; u++) {
            const int64_t k = kt + u * 256 + (int64_t)threadIdx.x;
            best_clear(cc[u]);
            if (k < k1) cc[u] = part[k];
        }
        // the 4-byte counts: lane x takes FIX_U consecutive tiles, scans them with its wave and leaves every tile's exclusive
        // prefix inside the wave's 64 * FIX_U tiles in LDS
        int32_t ts[FIX_U], ts2[FIX_U];
        int64_t sum = 0, sum2 = 0;
#pragma unroll
        for (int u = 0; u < FIX_U; u++) {
            const int64_t k = kt + (int64_t)threadIdx.x * FIX_U + u;
            ts[u] = 0; ts2[u] = 0;
            if (k < k1) { ts[u] = tileS[k]; if (HYP) ts2[u] = tileS2[k]; }
            sum += ts[u]; sum2 += ts2[u];
        }
        int64_t inc = sum, inc2 = sum2;
        for (int o = 1; o < 64; o <<= 1) {
            int64_t v = shfl_up64(inc, o);
            if (lane >= o) inc += v;
            if (HYP) { int64_t v2 = shfl_up64(inc2, o); if (lane >= o) inc2 += v2; }
        }
        __syncthreads();                                     // (the previous item's prefixes and partials have been read)
        {
            int64_t run = inc - sum, run2 = inc2 - sum2;
#pragma unroll
            for (int u = 0; u < FIX_U; u++) {
                s_pre[threadIdx.x * FIX_U + u] = run; run += ts[u];
                if (HYP) { s_pre2[threadIdx.x * FIX_U + u] = run2; run2 += ts2[u]; }
            }
        }
        if (lane == 63) { s_w[wv] = inc; if (HYP) s_w2[wv] = inc2; }
        __syncthreads();
        int64_t wb[5], wb2[5];                               // counts of the trip before wave w's tiles; [4]: the trip's total
        wb[0] = 0; wb2[0] = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { wb[w + 1] = wb[w] + s_w[w]; wb2[w + 1] = HYP ? wb2[w] + s_w2[w] : 0; }
#pragma unroll
        for (int u = 0; u < FIX_U; u++) {                    // tile u * 256 + x of the trip was scanned by wave (u * 256 + x) / (64 * FIX_U)
            static_assert((64 * FIX_U) % 256 == 0, "a wave's tiles are whole rows of 256");
            const int e = u * 256 + (int)threadIdx.x, w = (u * 256) / (64 * FIX_U);
            fix_merge<TC, HYP>(acc, cc[u], wb[w] + s_pre[e], HYP ? wb2[w] + s_pre2[e] : 0, M);
        }
        best_wave_min<TC, HYP>(acc, lane);
        if (lane == 0) s_part[wv] = acc;
        __syncthreads();
        if (wv != 0) continue;                               // (wave-uniform; the other waves go on to the next item's loads)
        const int64_t ntrip = (k1 - k0 + FIX_TRIP - 1) / FIX_TRIP;
        const int4 td = tdesc[t];
        const int64_t anchor = td.y, anchor2 = HYP ? (int64_t)tS0l[t] : 0;
        Best<TC, HYP> out; best_clear(out);
        bool write = false;
        if (lane == 0) {
            for (int w = 1; w < 4; w++) {
                Best<TC, HYP> c = s_part[w];
                bool take = (acc.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < acc.v || (c.v == acc.v && c.p > acc.p)));
                if (take) acc = c;
            }
        }
        if (ntrip == 1) {                                    // the whole task: the anchor on top, done
            if (lane == 0) { fix_merge<TC, HYP>(out, acc, anchor, anchor2, M); write = true; }
        } else {
            uint32_t got = 0;
            if (lane == 0) {
                unsigned long long *r = trec + (size_t)i * FIX_REC_W;
                __hip_atomic_store(r + 0, fix_bits<TC>(acc.v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(r + 1, (unsigned long long)(uint32_t)acc.p | ((unsigned long long)(uint32_t)acc.nn << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(r + 2, (unsigned long long)wb[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (HYP) {
                    __hip_atomic_store(r + 3, (unsigned long long)(uint32_t)best_nl(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(r + 4, (unsigned long long)wb2[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // The record is released at agent scope BEFORE the ticket is drawn.  The fence alone is the release the memory model asks
                // for; the explicit wait behind it is there because a release fence's own wait for the stores has been seen to be
                // dropped by the compiler when a waited load or a used atomic precedes it, and ACQ_REL on the ticket costs nothing more
                // (one more write-back of an L2 that is clean by then) and makes the last arriver's acquire part of the atomic itself.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                got = __hip_atomic_fetch_add(&tick[t], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            }
            got = (uint32_t)__shfl((int)got, 0);
            if ((int64_t)got != ntrip - 1) continue;         // (wave-uniform) somebody else draws the last ticket
            // ---- the fold, by this wave: lane j takes the trips j, j + 64, ... in order
            // Only lane 0 drew the ticket, all 64 lanes read records.  What that relies on: the acquire fence is one instruction of the
            // WAVE (it drops the stale lines of this CU's L1 and of this XCD's L2 for every lane), it is executed after the ticket's
            // value has come back, and every record word is read by an agent-scope load, which is served from neither of those caches.
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            int64_t base = anchor, base2 = anchor2;
            for (int64_t j0 = 0; j0 < ntrip; j0 += 64) {
                const int64_t j = j0 + lane;
                Best<TC, HYP> c; best_clear(c);
                int64_t s1 = 0, s2 = 0;
                if (j < ntrip) {
                    const unsigned long long *r = trec + (size_t)(ioffs ? ioffs[t] + (int32_t)j : item_of[k0 + j * FIX_TRIP]) * FIX_REC_W;
                    const unsigned long long w0 = __hip_atomic_load(r + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long w1 = __hip_atomic_load(r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s1 = (int64_t)__hip_atomic_load(r + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    c.v = fix_val<TC>(w0); c.p = (int32_t)(uint32_t)w1; c.nn = (int32_t)(uint32_t)(w1 >> 32);
                    if (HYP) {
                        best_set_nl(c, (int32_t)(uint32_t)__hip_atomic_load(r + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                        s2 = (int64_t)__hip_atomic_load(r + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                int64_t inc1 = s1, incb = s2;
                for (int o = 1; o < 64; o <<= 1) {
                    int64_t v = shfl_up64(inc1, o);
                    if (lane >= o) inc1 += v;
                    if (HYP) { int64_t v2 = shfl_up64(incb, o); if (lane >= o) incb += v2; }
                }
                fix_merge<TC, HYP>(out, c, base + inc1 - s1, base2 + incb - s2, M);
                base += shfl64(inc1, 63);
                if (HYP) base2 += shfl64(incb, 63);
            }
            best_wave_min<TC, HYP>(out, lane);
            if (lane == 0) {
                __hip_atomic_store(&tick[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (every ticket of the task is drawn: zero again for the next round)
                atomicAdd(&rc->n_trips, 1);
                write = true;
            }
        }
        if (write) {
            int64_t rw = (int64_t)tb[t] * n1 + prow(((int64_t)td.z), n1 - 1);
            opt[rw] = out.p; nnopt[rw] = out.nn;
            if (HYP) nlopt[rw] = best_nl(out);
        }
    }
}

// ------------------------------------------------------------------ left part: stream, scan, evaluate, arg-min
// HYP: hyperedge-cut costs carry a second count (self nets): rows bucketed by their FIRST column (fpos / flast),
// a column p joining on the left adds the rows with first == p and last < r.

template <typename TC, bool HYP>
__global__ void __launch_bounds__(256, 6) k_lpass(RoundDesc R, const RoundCounts *__restrict__ rc, const int64_t *__restrict__ a_offs,
                                                  const int4 *__restrict__ a_tdesc, const int32_t *__restrict__ a_tS0l,
                                                  const uint8_t *__restrict__ a_tb, const int32_t *__restrict__ a_pos,
                                                  const int32_t *__restrict__ a_next, const int32_t *__restrict__ a_fpos,
                                                  const int32_t *__restrict__ a_flast, int32_t *__restrict__ a_opt,
                                                  int32_t *__restrict__ a_nnopt, int32_t *__restrict__ a_nlopt,
                                                  int32_t *__restrict__ a_loc, int32_t *__restrict__ a_loc2,
                                                  int32_t *__restrict__ a_tileS, int32_t *__restrict__ a_tileS2,
                                                  int64_t *__restrict__ a_taskR, const int64_t *__restrict__ a_tile_t0,
                                                  const int4 *__restrict__ a_tile_rec,
                                                  const TC *__restrict__ W, DevModel<TC> M, TC alpha, Best<TC, HYP> *__restrict__ partR,
                                                  Best<TC, HYP> *__restrict__ partL)
{
    __shared__ int32_t s_off_all[4][LT + 2];
    __shared__ unsigned long long s_hd_all[4][LT / 64];
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (no grid-stride loop: the host launches one wave per tile of the buffers' capacity, see k_lpass_own)
    const int64_t T = rc->T, ntask = rc->nlong;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    int64_t tile_start = tile * LT;
    bool active = tile_start < T;
    int32_t *s_off = s_off_all[wave];
    unsigned long long *s_hd = s_hd_all[wave];
    // interior tile (k_tile_t0 classified it): four out of five tiles -- the D&C re-scans the wide gaps of the arg-min
    // staircase at every level.  Wave-uniform fast path: nothing to look up, one threshold, nothing to evaluate here
    // (k_open finishes these tiles from `loc`).
    int4 rec = active ? a_tile_rec[tile] : make_int4(0, 0, 0, 0);
    bool interior = rec.w != 0;
    int64_t t0 = 0; int cnt = 0;
    if (!interior) {
        t0 = active ? a_tile_t0[tile] : 0;
        load_tile_tasks(a_offs, ntask, t0, tile_start, active, s_off, s_hd, lane, cnt);
    }
    __syncthreads();
    if (!active) return;
    if (interior) {
        // The admitted costs are affine in the counts with constant coefficients, and all steps of the tile share the count
        // made before the tile (the same task): the tile's arg-min does not depend on it.  Evaluate with the counts since
        // the tile start; k_fix adds the task's base when it merges the tiles.
        int32_t tl = (T - tile_start < LT) ? (int32_t)(T - tile_start) - 1 : LT - 1;
        int32_t acc[4], acc2[4] = {0, 0, 0, 0}, sk[4], sk2[4];
        interior_stream<true>(a_next, a_pos, rec.x, tl, rec.y, lane, acc, sk);
        if (HYP) interior_stream<false>(a_flast, a_fpos, rec.x, tl, rec.y, lane, acc2, sk2);
        int sel = tl >> 6;
        if (lane == (tl & 63)) {
            a_tileS[tile] = sel == 0 ? acc[0] : sel == 1 ? acc[1] : sel == 2 ? acc[2] : acc[3];
            if (HYP) a_tileS2[tile] = sel == 0 ? acc2[0] : sel == 1 ? acc2[1] : sel == 2 ? acc2[2] : acc2[3];
        }
        Best<TC, HYP> best; best_clear(best);
#pragma unroll
        for (int k = 0; k < 4; k++) {                       // increasing e = decreasing p: an earlier candidate wins ties
            int32_t e = lane + 64 * k;
            if (e <= tl) {
                int32_t p = rec.x - e;
                TC fv = dm_apply_affine(M, alpha, (int64_t)(rec.y - p), (int64_t)(rec.z - sk[k]), (int64_t)acc[k], (int64_t)acc2[k]);
                Best<TC, HYP> c; best_clear(c); c.v = cadd(W[p], fv); c.p = p; c.nn = acc[k]; best_set_nl(c, acc2[k]);
                best = better(best, c);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {                  // wave arg-min; ties -> larger p
            int src = (lane + o) & 63;
            Best<TC, HYP> c; best_clear(c); c.v = shfl64(best.v, src); c.p = __shfl(best.p, src); c.nn = __shfl(best.nn, src);
            if (HYP) best_set_nl(c, __shfl(best_nl(best), src));
            bool take = (best.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < best.v || (c.v == best.v && c.p > best.p)));
            if (lane + o < 64 && take) best = c;
        }
        if (lane == 0) partL[tile] = best;
        return;
    }
    // local task index of a step = (#heads at or before it in the tile) - (1 if the tile starts with a head)
    int head_at0 = (s_off[0] == 0) ? 1 : 0;
    int hd_before = 0;                                  // heads in the groups already processed
    int64_t n1 = R.n + 1;
    int32_t tile_last = (T - tile_start < LT) ? (int32_t)(T - tile_start) - 1 : LT - 1;     // relative to the tile start
    // everything below is 32-bit: step indices are relative to the tile, nonzero positions are < 2^31

    constexpr int NG = LT / 64;
    int32_t carryS = 0, carryS2 = 0;                   // segmented-sum state across the groups of the tile
    Best<TC, HYP> bcarry; best_clear(bcarry);
    for (int g = 0; g < NG; g++) {
        int32_t e = g * 64 + lane;
        bool valid = e <= tile_last;
        int32_t t = 0, i = 0, r = 0, B = 0, p = -1, toff = 0, seg_last = -1, s = 0, en = 0, s2 = 0, en2 = 0, posr = 0;
        int32_t s0 = 0, s0l = 0; TC wp = (TC)0;
        unsigned long long hmask = s_hd[g];
        if (valid) {
            int li = hd_before + __popcll(hmask & ((2ull << lane) - 1)) - head_at0;
            t = (int32_t)t0 + li;
            toff = s_off[li];
            if (li + 1 < cnt) seg_last = s_off[li + 1] - 1;
            else { int64_t nx = a_offs[(int64_t)t + 1] - tile_start; seg_last = nx > 0x3fffffff ? 0x3fffffff : (int32_t)nx - 1; }
            i = e - toff;
            int4 td = a_tdesc[t];
            B = td.x; s0 = td.y; r = td.z; posr = td.w;
            if (HYP) s0l = a_tS0l[t];
            p = B - i;
            if (i == 0) { s = en = a_pos[B]; if (HYP) s2 = en2 = a_fpos[B]; }
            else { s = a_pos[p]; en = a_pos[p + 1]; if (HYP) { s2 = a_fpos[p]; en2 = a_fpos[p + 1]; } }
            wp = W[p];
            if (i == 0 && R.isA) p = -1;              // round A: element 0 (p = r) is not a candidate
        }
        hd_before += __popcll(hmask);
        int32_t thr = valid ? r : INT32_MAX;
        int32_t d = coop_count<true>(a_next, s, en, thr, valid, lane);                  // next[q] >= r
        int32_t d2 = 0;
        if (HYP) d2 = coop_count<false>(a_flast, s2, en2, thr, valid, lane);           // last < r
        // ---- segmented prefix of the step counts (restart at every task head)
        int f = valid ? (i == 0) : 1;
        int32_t x = d;
        wave_segsum(x, f, lane);
        if (!f) x += carryS;
        carryS = __shfl(x, 63);
        int32_t x2 = 0;
        if (HYP) {
            int f2 = valid ? (i == 0) : 1;
            x2 = d2;
            wave_segsum(x2, f2, lane);
            if (!f2) x2 += carryS2;
            carryS2 = __shfl(x2, 63);
        }
        // ---- evaluate (only where the task head lies in this tile: the count is final)
        bool head_in_tile = valid && toff >= 0;
        Best<TC, HYP> bx; best_clear(bx);
        if (head_in_tile && p >= 0) {
            int64_t nn = (int64_t)s0 + x, nl = HYP ? (int64_t)s0l + x2 : 0;
            TC fv = dm_apply_affine(M, alpha, (int64_t)(r - p), (int64_t)(posr - s), nn, nl);     // s == pos[p] for every candidate
            bx.v = cadd(wp, fv); bx.p = p; bx.nn = (int32_t)nn; best_set_nl(bx, (int32_t)nl);
        } else if (valid && !head_in_tile) {
            a_loc[tile_start + e] = x;                  // counts since the tile start; finished by k_open
            if (HYP) a_loc2[tile_start + e] = x2;
        }
        int bf = valid ? (i == 0) : 1;
        wave_segmin<TC, HYP>(bx, bf, lane);
        if (!bf) bx = better(bcarry, bx);
        {
            Best<TC, HYP> nb; best_clear(nb); nb.v = shfl64(bx.v, 63); nb.p = __shfl(bx.p, 63); nb.nn = __shfl(bx.nn, 63);
            if (HYP) best_set_nl(nb, __shfl(best_nl(bx), 63));
            bcarry = nb;
        }
        if (head_in_tile) {
            if (e == seg_last) {
                int b = a_tb[t];
                a_opt[(int64_t)b * n1 + prow((r), n1 - 1)] = bx.p;
                a_nnopt[(int64_t)b * n1 + prow((r), n1 - 1)] = bx.nn;
                if (HYP) a_nlopt[(int64_t)b * n1 + prow((r), n1 - 1)] = best_nl(bx);
            } else if (e == tile_last) {
                partR[tile] = bx; a_taskR[tile] = (int64_t)t;
            }
        }
    }
    if (lane == 0) { a_tileS[tile] = carryS; if (HYP) a_tileS2[tile] = carryS2; }   // counts since the last head of the tile
}

// ------------------------------------------------------------------ tasks that span tiles
// A task whose steps continue beyond its head tile is finished in one of two ways:
//  * short spans (the task ends in the next tile, at most SPAN_SHORT steps there): ONE LANE evaluates the remaining
//    steps from the counts k_lpass left in `loc`, merges them with the head tile's partial and writes the winner
//    (k_span_short, one lane per tile -- at low tau nearly every tile boundary cuts a short task);
//  * long spans: every covered tile is reduced by one wave (k_open), then one wave per head tile merges the
//    partials (k_fix).  k_span_short appends those tiles to two work lists; the wave kernels walk the lists.
constexpr int SPAN_SHORT = 32;

template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_span_short(RoundDesc R, RoundCounts *__restrict__ rc, const int64_t *__restrict__ a_offs,
                                                    const int4 *__restrict__ a_tdesc, const int32_t *__restrict__ a_tS0l,
                                                    const uint8_t *__restrict__ a_tb, const int32_t *__restrict__ a_pos,
                                                    const int32_t *__restrict__ a_loc, const int32_t *__restrict__ a_loc2,
                                                    const int64_t *__restrict__ a_tile_t0, const int64_t *__restrict__ a_taskR,
                                                    const int32_t *__restrict__ a_tileS, const int32_t *__restrict__ a_tileS2,
                                                    const Best<TC, HYP> *__restrict__ partR, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                    int32_t *__restrict__ a_opt, int32_t *__restrict__ a_nnopt, int32_t *__restrict__ a_nlopt,
                                                    int32_t *__restrict__ open_list, int32_t *__restrict__ fix_list,
                                                    const int4 *__restrict__ a_tile_rec)
{
    int lane = threadIdx.x & 63;
    const int64_t ntile = rc->ntile;
    for (int64_t tbase = (int64_t)blockIdx.x * blockDim.x; tbase < ntile; tbase += (int64_t)gridDim.x * blockDim.x) {      // wave-uniform
    int64_t tile = tbase + threadIdx.x;
    bool in = tile < ntile;
    int64_t n1 = R.n + 1;
    // ---- role 1: this tile is the head tile of a task that continues beyond it
    bool fix_long = false;
    if (in) {
        int64_t t = a_taskR[tile];
        if (t >= 0) {
            int64_t end = a_offs[t + 1] - 1, ntl = (tile + 1) * LT;
            int64_t open_len = end - ntl + 1;
            // (a partial last tile can be both "fully covered" = interior, evaluated by k_lpass, and short: interior wins)
            if (end / LT == tile + 1 && open_len <= SPAN_SHORT && a_tile_rec[tile + 1].w == 0) {
                int4 td = a_tdesc[t];
                int64_t toff = a_offs[t];
                int64_t B = td.x, r = td.z;
                int64_t base = (int64_t)td.y + a_tileS[tile];           // counts up to the end of the head tile
                int64_t base2 = HYP ? (int64_t)a_tS0l[t] + a_tileS2[tile] : 0;
                Best<TC, HYP> best = partR[tile];
                for (int64_t e = ntl; e <= end; e++) {                  // decreasing p: earlier candidates win ties
                    int64_t p = B - (e - toff);
                    int64_t nn = base + a_loc[e], nl = HYP ? base2 + a_loc2[e] : 0;
                    TC fv = dm_apply_affine(M, alpha, r - p, (int64_t)(td.w - a_pos[p]), nn, nl);
                    Best<TC, HYP> c; best_clear(c); c.v = cadd(W[p], fv); c.p = (int32_t)p; c.nn = (int32_t)nn; best_set_nl(c, (int32_t)nl);
                    best = better(best, c);
                }
                int b = a_tb[t];
                a_opt[(int64_t)b * n1 + prow((r), n1 - 1)] = best.p;
                a_nnopt[(int64_t)b * n1 + prow((r), n1 - 1)] = best.nn;
                if (HYP) a_nlopt[(int64_t)b * n1 + prow((r), n1 - 1)] = best_nl(best);
            } else {
                fix_long = true;
            }
        }
    }
    // ---- role 2: this tile starts inside a task of a long span
    bool open_long = false;
    if (in && a_tile_rec[tile].w == 0) {                   // interior tiles were evaluated by k_lpass
        int64_t tile_start = tile * LT;
        int64_t t0 = a_tile_t0[tile];
        int64_t toff0 = a_offs[t0];
        if (toff0 < tile_start) {
            int64_t end0 = a_offs[t0 + 1] - 1, h = toff0 / LT;
            bool is_short = (end0 / LT == h + 1) && (end0 - tile_start + 1 <= SPAN_SHORT);
            open_long = !is_short;
        }
    }
    // wave-aggregated appends
    unsigned long long mo = __ballot(open_long), mf = __ballot(fix_long);
    int32_t bo = 0, bf = 0;
    if (lane == 0) {
        if (mo) bo = atomicAdd(&rc->n_open, (int32_t)__popcll(mo));
        if (mf) bf = atomicAdd(&rc->n_fix, (int32_t)__popcll(mf));
    }
    bo = __shfl(bo, 0); bf = __shfl(bf, 0);
    unsigned long long below = (1ull << lane) - 1ull;
    if (open_long) open_list[bo + __popcll(mo & below)] = (int32_t)tile;
    if (fix_long) fix_list[bf + __popcll(mf & below)] = (int32_t)tile;
    }
}

// open-left part of a tile of a long span (the task started in an earlier tile): one wave per listed tile
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_open(RoundDesc R, const RoundCounts *__restrict__ rc, const int64_t *__restrict__ a_offs,
                                              const int4 *__restrict__ a_tdesc,
                                              const int32_t *__restrict__ a_tS0l,
                                              const int32_t *__restrict__ a_pos, const int32_t *__restrict__ a_loc,
                                              const int32_t *__restrict__ a_loc2, const int64_t *__restrict__ a_tile_t0,
                                              const int64_t *__restrict__ tilePS,
                                              const int64_t *__restrict__ tilePS2, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                              Best<TC, HYP> *__restrict__ partL, const int32_t *__restrict__ open_list)
{
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t cnt = rc->n_open, T = rc->T;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < cnt; w += nw) {
        int64_t tile = open_list[w];
        int64_t tile_start = tile * LT;
        int64_t t = a_tile_t0[tile];                        // task of the tile's first step
        int64_t toff = a_offs[t];
        int64_t last = a_offs[t + 1] - 1;
        int64_t tile_last = tile_start + LT - 1;
        if (tile_last > T - 1) tile_last = T - 1;
        if (last > tile_last) last = tile_last;
        int4 td = a_tdesc[t];
        int64_t r = td.z, B = td.x;
        // counts of this task in earlier tiles: its head tile contributes "since the last head", every tile in
        // between is covered entirely by the task: a range sum over the per-tile tails (tilePS = their prefix sums)
        int64_t base = (int64_t)td.y + (tilePS[tile] - tilePS[toff / LT]);
        int64_t base2 = HYP ? (int64_t)a_tS0l[t] + (tilePS2[tile] - tilePS2[toff / LT]) : 0;
        Best<TC, HYP> best; best_clear(best);
        for (int64_t e = tile_start + lane; e <= last; e += 64) {
            int64_t p = B - (e - toff);
            int64_t nn = base + a_loc[e], nl = HYP ? base2 + a_loc2[e] : 0;
            TC fv = dm_apply_affine(M, alpha, r - p, (int64_t)(td.w - a_pos[p]), nn, nl);
            Best<TC, HYP> c; best_clear(c); c.v = cadd(W[p], fv); c.p = (int32_t)p; c.nn = (int32_t)nn; best_set_nl(c, (int32_t)nl);
            best = better(best, c);                         // a lane visits its steps in increasing e (decreasing p)
        }
        // wave arg-min; ties -> larger p
        for (int o = 32; o > 0; o >>= 1) {
            int src = (lane + o) & 63;
            Best<TC, HYP> c; best_clear(c); c.v = shfl64(best.v, src); c.p = __shfl(best.p, src); c.nn = __shfl(best.nn, src);
            if (HYP) best_set_nl(c, __shfl(best_nl(best), src));
            bool take = (best.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < best.v || (c.v == best.v && c.p > best.p)));
            if (lane + o < 64 && take) best = c;
        }
        if (lane == 0) partL[tile] = best;
    }
}

// a task of a long span: combine the head tile's partial with the partials of the tiles it covers
// (one wave per listed head tile)
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_fix(const RoundCounts *__restrict__ rc, const int64_t *__restrict__ offs, const int64_t *__restrict__ taskR,
                                             const Best<TC, HYP> *__restrict__ partL, const Best<TC, HYP> *__restrict__ partR,
                                             const int4 *__restrict__ tdesc, const uint8_t *__restrict__ tb,
                                             int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt, int64_t n1,
                                             const int32_t *__restrict__ fix_list,
                                             const int4 *__restrict__ tile_rec, const int64_t *__restrict__ tilePS, const int64_t *__restrict__ tilePS2,
                                             const int32_t *__restrict__ tS0l, DevModel<TC> M)
{
    int lane = threadIdx.x & 63;
    int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t cnt = rc->n_fix;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < cnt; w += nw) {
        int64_t tile = fix_list[w];
        int64_t t = taskR[tile];
        int64_t end_tile = (offs[t + 1] - 1) / LT;
        int64_t S0 = tdesc[t].y, S0l = HYP ? (int64_t)tS0l[t] : 0;
        Best<TC, HYP> acc; best_clear(acc);
        for (int64_t k = tile + 1 + lane; k <= end_tile; k += 64) {
            Best<TC, HYP> c = partL[k];
            if (tile_rec[k].w != 0 && c.p >= 0) {            // interior tile: counts and value are relative to the tile start
                int64_t base = S0 + (tilePS[k] - tilePS[tile]);
                int64_t base2 = HYP ? S0l + (tilePS2[k] - tilePS2[tile]) : 0;
                c.v = cadd(c.v, dm_apply_affine(M, (TC)0, (int64_t)0, (int64_t)0, base, base2));       // the costs are affine in the counts
                c.nn = (int32_t)(c.nn + base);
                if (HYP) best_set_nl(c, (int32_t)(best_nl(c) + base2));
            }
            bool take = (acc.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < acc.v || (c.v == acc.v && c.p > acc.p)));
            if (take) acc = c;
        }
        for (int o = 32; o > 0; o >>= 1) {
            int src = (lane + o) & 63;
            Best<TC, HYP> c; best_clear(c); c.v = shfl64(acc.v, src); c.p = __shfl(acc.p, src); c.nn = __shfl(acc.nn, src);
            if (HYP) best_set_nl(c, __shfl(best_nl(acc), src));
            bool take = (acc.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < acc.v || (c.v == acc.v && c.p > acc.p)));
            if (lane + o < 64 && take) acc = c;
        }
        if (lane == 0) {
            Best<TC, HYP> res = better(partR[tile], acc);   // the head tile holds the larger p: wins ties
            int64_t r = tdesc[t].z; int b = tb[t];
            opt[(int64_t)b * n1 + prow((r), n1 - 1)] = res.p;
            nnopt[(int64_t)b * n1 + prow((r), n1 - 1)] = res.nn;
            if (HYP) nlopt[(int64_t)b * n1 + prow((r), n1 - 1)] = best_nl(res);
        }
    }
}

// ---- anchors of the mirrored head tasks (windowed layers), once per (pattern, w)
// hist[e] = #{q : e(q) = e}, e(q) = min(next[q], col[q] + w, n): then  nets(max(0, r - w), r) = pos[r] - #{q : e(q) < r}   (an entry is counted by
// the window ending before r iff it lies in a column < r, is the LAST occurrence of its row before r, and its column is >= r - w)
// Without atomics (10^8 scattered atomic adds took 12.5 ms; this takes the time of two column passes): the entries with e = x are
//   * next[q] = x <= col[q] + w : one per entry q' of COLUMN x whose previous occurrence is within the window, prev[q'] >= max(0, x - w);
//   * col[q] + w = x < next[q]  : the entries of column x - w that do not come back by column x;
// one lane per column x < n (hist[n] is never read: E[r] sums the values below r <= n), eight loads in flight.
__global__ void __launch_bounds__(256) k_win_hist(int64_t n, int64_t w, const int32_t *__restrict__ pos, const int32_t *__restrict__ prev,
                                                  const int32_t *__restrict__ next, int32_t *__restrict__ hist)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > n) return;
    int32_t c = 0;
    if (x < n) {
        const int32_t lo = (int32_t)(x > w ? x - w : 0);
        for (int32_t q = pos[x], q1 = pos[x + 1]; q < q1; q += 8) {
            int32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? prev[q + k] : -1;
#pragma unroll
            for (int k = 0; k < 8; k++) c += (v[k] >= lo);
        }
        if (x >= w) {
            const int32_t xx = (int32_t)x;
            for (int32_t q = pos[x - w], q1 = pos[x - w + 1]; q < q1; q += 8) {
                int32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? next[q + k] : INT32_MIN;
#pragma unroll
                for (int k = 0; k < 8; k++) c += (v[k] > xx);
            }
        }
    }
    hist[x] = c;
}
// the same for whole rows (self nets): rows with first >= r - w and last < r  =  #{last < r} - #{max(last, first + w) < r}
__global__ void __launch_bounds__(256) k_win_hist_rows(int64_t m, int64_t n, int64_t w, const int32_t *__restrict__ rfirst, const int32_t *__restrict__ rlast,
                                                       int32_t *__restrict__ hist)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    int64_t f = rfirst[i];
    if (f < 0) return;                                      // empty row
    int64_t e = f + w, l = rlast[i];
    if (l > e) e = l;
    if (e > n) e = n;
    atomicAdd(&hist[e], 1);
}
// one wave per mirrored head (plane b < s, rho = idx << (b+1)): entries of the block's columns passing the test
//   tot[aoff[b] + idx] = #{q in the columns of the block : next[q] >= rho}   (GE)   /   #{rows starting in the block with last < rho}
template <bool GE>
__global__ void __launch_bounds__(256) k_win_block_totals(RoundDesc R, int64_t nitems, const int32_t *__restrict__ cpos, const int32_t *__restrict__ arr,
                                                          int32_t *__restrict__ tot)
{
    const int lane = threadIdx.x & 63;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < nitems; it += (int64_t)gridDim.x * 4) {
        int b = 0;
        while (it >= R.aoff[b + 1]) b++;
        const int64_t idx = it - R.aoff[b], rho = idx << (b + 1);
        int32_t c = 0;
        int64_t cs, ce;
        if (idx >= 1 && rho <= R.n && geo_block(R.G, rho, b, cs, ce)) {
            const int32_t thr = (int32_t)rho;
            for (int32_t q = cpos[cs] + lane, q1 = cpos[ce]; q < q1; q += 64) { const int32_t v = arr[q]; c += GE ? (v >= thr) : (v < thr); }
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) tot[it] = c;
    }
}
// anchor of (b, rho) = count of the whole window [max(0, rho - w), rho) minus the totals of the blocks b' <= b left of the block's end
__global__ void __launch_bounds__(256) k_win_anchors(RoundDesc R, int64_t nitems, const int64_t *__restrict__ base, const int64_t *__restrict__ E,
                                                     const int32_t *__restrict__ tot, int32_t *__restrict__ anch)
{
    int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= nitems) return;
    int b = 0;
    while (it >= R.aoff[b + 1]) b++;
    const int64_t idx = it - R.aoff[b], rho = idx << (b + 1);
    if (idx < 1 || rho > R.n) { anch[it] = 0; return; }
    int64_t v = base[rho] - E[rho];
    for (int bb = 0; bb <= b; bb++) v -= tot[R.aoff[bb] + (rho >> (bb + 1))];
    anch[it] = (int32_t)v;
}

// leaf pass: the part [64 g + 62 - w, 64 g) of every group (E from the histogram of width w - 62)
__global__ void __launch_bounds__(256) k_leaf_anchors(int64_t ng, int64_t n, const int64_t *__restrict__ base, const int64_t *__restrict__ E,
                                                      int32_t *__restrict__ anch)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int64_t r = g << 6;
    anch[g] = r <= n ? (int32_t)(base[r] - E[r]) : 0;
}

// ------------------------------------------------------------------ round A from cached counts
// Round A (row r against its lowest block [r - 2^b, r), b = ctz(r)) is the one round whose candidate ranges do not depend on
// the layer: nets(p, r) for all its (row, candidate) pairs -- sum_r 2^ctz(r) = n log2(n) / 2 values -- is computed ONCE per
// partition and kept (4 B each); a layer then evaluates round A by streaming counts, W and pos (16 B per candidate instead
// of the candidate's whole column).  Elements are stored level by level (b), row by row, candidate p = r - 1 - i at index i;
// every level is padded to whole tiles of LT elements.
// tiles of level b: [tbase[b], tbase[b+1]); rows of the levels >= 9: [rbase[b], rbase[b+1]).
// mir_w = 0: the unconstrained scheme's round-A rows -- level b holds the rows r = (2u+1) 2^b, candidates r - 1 - i, i < 2^b.
// mir_w = w > 0: the MIRRORED heads of the windowed geometry (geo_block) -- level b < s holds the rows r = (u+1) 2^(b+1),
// candidates ce - 1 - i with ce = r + 2^(b+1) - 1 - w (those below column 0 do not exist); the counts carry the head's anchor
// nets(ce, r), at aoff[b] + (r >> (b+1)) of the window anchors.  tlo / thi: the tiles of each level a windowed layer needs.

__device__ __forceinline__ int64_t ra_row(const RATab &T, int b, int64_t u)
{
    return T.mir_w ? (u + 1) << (b + 1) : ((u << 1) | 1) << b;
}

__device__ __forceinline__ bool ra_decode(const RATab &T, int64_t tile, int j, int &b, int64_t &r, int64_t &p, int64_t &i)
{
    b = 0;
    while (tile >= T.tbase[b + 1]) b++;                     // (uniform per tile)
    int64_t e = (tile - T.tbase[b]) * LT + j;               // element inside the level
    int64_t u = e >> b;
    i = e & (((int64_t)1 << b) - 1);
    r = ra_row(T, b, u);
    p = (T.mir_w ? r + ((int64_t)2 << b) - 1 - T.mir_w : r) - 1 - i;
    return r <= T.n && p >= 0;
}

// d[E] = #{q in column p : next[q] >= r} (d2: rows whose first column is p and whose last column is < r)
__global__ void __launch_bounds__(256) k_ra_colcount(RATab T, const int32_t *__restrict__ pos, const int32_t *__restrict__ next,
                                                     const int32_t *__restrict__ fpos, const int32_t *__restrict__ flast,
                                                     int32_t *__restrict__ d, int32_t *__restrict__ d2)
{
    int b; int64_t r, p, i;
    bool ok = ra_decode(T, blockIdx.x, threadIdx.x, b, r, p, i);
    int64_t E = (int64_t)blockIdx.x * LT + threadIdx.x;
    int32_t c = 0, c2 = 0;
    if (ok) {
        int32_t rr = (int32_t)r;
        for (int32_t q = pos[p], q1 = pos[p + 1]; q < q1; q += 8) {        // eight loads in flight (one at a time: a memory latency per entry)
            int32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = q + k < q1 ? next[q + k] : INT32_MIN;
#pragma unroll
            for (int k = 0; k < 8; k++) c += (v[k] >= rr);
        }
        if (d2) for (int32_t q = fpos[p], q1 = fpos[p + 1]; q < q1; q++) c2 += (flast[q] < rr);
    }
    d[E] = c;
    if (d2) d2[E] = c2;
}

// c[E] = sum of d over the row's elements 0 .. i  (G = exclusive prefix sums of d over all elements)
__global__ void __launch_bounds__(256) k_ra_final(RATab T, const int64_t *__restrict__ G, int32_t *__restrict__ c, const int32_t *__restrict__ anch)
{
    int b; int64_t r, p, i;
    ra_decode(T, blockIdx.x, threadIdx.x, b, r, p, i);
    int64_t E = (int64_t)blockIdx.x * LT + threadIdx.x;
    int32_t v = (int32_t)(G[E + 1] - G[E - i]);
    if (anch && r <= T.n) v += anch[T.aoff[b] + (r >> (b + 1))];            // (mirrored heads: the part [ce, r) the block's columns stand on)
    c[E] = v;
}

template <typename TC, bool HYP>
__device__ __forceinline__ bool ra_takes(const Best<TC, HYP> &x, const Best<TC, HYP> &c)      // c replaces x: smaller value, or equal value and larger p
{
    return (x.p < 0) ? (c.p >= 0) : (c.p >= 0 && (c.v < x.v || (c.v == x.v && c.p > x.p)));
}

// one wave per tile of LT elements; a lane holds four consecutive elements.  Rows of up to LT candidates (b <= 8) lie inside
// one tile and are finished here; longer rows leave one partial per tile for k_ra_merge.
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_ra_layer(RATab T, int64_t ntile, const int32_t *__restrict__ cnt, const int32_t *__restrict__ cnt2,
                                                  const int32_t *__restrict__ pos, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                  int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt,
                                                  Best<TC, HYP> *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntile) return;
    const int64_t n1 = T.n + 1;
    const int64_t E0 = tile * LT + 4 * lane;
    const int4 c4 = *reinterpret_cast<const int4 *>(cnt + E0);
    int4 d4 = make_int4(0, 0, 0, 0);
    if (HYP) d4 = *reinterpret_cast<const int4 *>(cnt2 + E0);
    // the lane's first element is decoded; from level 2 on the other three are the next candidates of the same row
    int b = 0;
    int64_t r0, p0, i0;
    const bool ok0 = ra_decode(T, tile, 4 * lane, b, r0, p0, i0);
    if (tile < T.tlo[b] || tile >= T.thi[b]) return;        // (uniform) a windowed layer: rows far from its window
    Best<TC, HYP> cand[4];
    int64_t rk[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int64_t r = r0, p = p0 - k;
        bool ok = ok0 && p >= 0;                            // (mirrored heads: a block may be cut off at column 0)
        if (b < 2) { int bb; int64_t ii; ok = ra_decode(T, tile, 4 * lane + k, bb, r, p, ii); }      // (uniform branch)
        rk[k] = ok ? r : 0;
        best_clear(cand[k]);
        if (ok) {
            int32_t c = k == 0 ? c4.x : k == 1 ? c4.y : k == 2 ? c4.z : c4.w, c2 = k == 0 ? d4.x : k == 1 ? d4.y : k == 2 ? d4.z : d4.w;
            cand[k].v = cadd(W[p], dm_apply_affine(M, alpha, r - p, (int64_t)(pos[r] - pos[p]), (int64_t)c, (int64_t)c2));
            cand[k].p = (int32_t)p; cand[k].nn = c; best_set_nl(cand[k], c2);
        }
    }
    if (b < 2) {                                            // rows of one or two candidates: finished inside the lane
        const int per = 1 << b;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((k & (per - 1)) != 0 || rk[k] == 0) continue;
            Best<TC, HYP> x = cand[k];
            if (per == 2 && ra_takes(x, cand[k + 1 < 4 ? k + 1 : 3])) x = cand[k + 1 < 4 ? k + 1 : 3];
            int64_t rw = (int64_t)b * n1 + prow((rk[k]), n1 - 1);
            opt[rw] = x.p; nnopt[rw] = x.nn;
            if (HYP) nlopt[rw] = best_nl(x);
        }
        return;
    }
    Best<TC, HYP> x = cand[0];
#pragma unroll
    for (int k = 1; k < 4; k++) if (ra_takes(x, cand[k])) x = cand[k];
    const int lpr = b >= 8 ? 64 : (1 << (b - 2));          // lanes per row
    for (int o = 1; o < lpr; o <<= 1) {                     // butterfly inside the row's lanes: every lane ends with the winner
        Best<TC, HYP> c; best_clear(c);
        c.v = shfl64(x.v, lane ^ o); c.p = __shfl(x.p, lane ^ o); c.nn = __shfl(x.nn, lane ^ o);
        if (HYP) best_set_nl(c, __shfl(best_nl(x), lane ^ o));
        if (ra_takes(x, c)) x = c;
    }
    if ((lane & (lpr - 1)) == 0) {
        if (b <= 8) {
            if (rk[0]) {
                int64_t rw = (int64_t)b * n1 + prow((rk[0]), n1 - 1);
                opt[rw] = x.p; nnopt[rw] = x.nn;
                if (HYP) nlopt[rw] = best_nl(x);
            }
        } else {
            part[tile - T.tbase[9]] = x;
        }
    }
}

// The same round, COLUMN-major: one wave per 256 consecutive candidates p, all levels.  A candidate p belongs to the round-A row
// of every level b whose bit is clear in p (r = p with the bits below b cleared, plus 2^b), a dozen rows on average: k_ra_layer reads
// its cost W[p] and its column pointer once per row (16 B per (candidate, row)); here they are read once per candidate and
// only the 4-byte cached count is read per row -- 60 B instead of 190 B per candidate and layer.  Lane l holds the candidates
// P0 + 4 l .. + 3; the count elements of a row are stored by descending p (ra_decode), so a lane's four are one aligned vector.
// Rows of up to 256 candidates (b <= 8) lie inside the wave's columns and are finished here (butterfly over the row's lanes);
// longer rows leave one partial per 256 candidates for k_ra_merge, in the slot k_ra_layer would use.
template <typename TC, bool HYP, bool MIR>
__global__ void __launch_bounds__(256) k_ra_cols(RATab T, const int32_t *__restrict__ cnt, const int32_t *__restrict__ cnt2,
                                                 const int32_t *__restrict__ pos, const TC *__restrict__ W, DevModel<TC> M, TC alpha,
                                                 int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt,
                                                 Best<TC, HYP> *__restrict__ part, int64_t tile0, int64_t tile1, int bmin)
{
    // levels bmin .. nbits - 1 (the leaf pass computes the levels below LEAF_T itself: their rows are never multiples of 64).
    // tiles [tile0, tile1) of 256 consecutive values of the coordinate z (a windowed layer needs the rows near its window only).
    // MIR = false: z = p, the candidate p belongs to the level-b row of the block [r - 2^b, r) iff bit b of z is CLEAR.
    // MIR = true (table with mir_w = w): z = p + w + 1, p belongs to the mirrored head rho = z with the bits <= b cleared
    // (block [rho + 2^b - 1 - w, rho + 2^(b+1) - 1 - w)) iff bit b of z is SET.  In both maps a row's 2^b candidates are an aligned
    // block of z and its elements run by descending z: element i = (2^b - 1) - (z mod 2^b).
    const int lane = threadIdx.x & 63;
    const int64_t n = T.n, n1 = n + 1, off = MIR ? T.mir_w + 1 : 0;
    const int64_t Z0 = (tile0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * LT;
    if (Z0 - off >= n || Z0 >= tile1 * LT) return;          // (wave-uniform) candidates are the columns 0 .. n - 1
    const int64_t z0 = Z0 + 4 * lane, p0 = z0 - off;
    TC wv[4]; int32_t pv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { int64_t p = p0 + k; p = p < 0 ? 0 : p < n ? p : n; wv[k] = W[p]; pv[k] = pos[p]; }
    for (int b = bmin; b < T.nbits; b++) {
        if (b >= 8 && (bool)((Z0 >> b) & 1) != MIR) continue;       // (wave-uniform) no row of this level over the wave's columns
        // the lane's row of this level and its candidates among z0 .. z0 + 3:
        //   b = 0: two rows of one candidate each; b = 1: one row of two; b >= 2: all four
        const int64_t mask = ((int64_t)1 << b) - 1;
        const bool cov = b < 2 || (bool)((z0 >> b) & 1) == MIR;
        const int64_t zr = (z0 >> (b + 1)) << (b + 1);              // z0 with the bits <= b cleared
        const int64_t r = MIR ? zr : zr + ((int64_t)1 << b);        // (b = 0: the first of the lane's two rows)
        const int64_t u = MIR ? (z0 >> (b + 1)) - 1 : z0 >> (b + 1);
        // the lane's candidates k0, k0 + 1 (b = 1) or 0 .. 3 (b >= 2); element of the LAST one (the smallest index)
        const int k0 = (b == 1 && MIR) ? 2 : 0;
        const int64_t zlast = b == 1 ? z0 + k0 + 1 : z0 + 3;
        const int64_t E = (T.tbase[b] << 8) + ((u << b) | (mask - (zlast & mask)));
        int32_t c[4] = {0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
        if (b == 0) {
            // single candidates: z0 + k (k = 0, 2; mirrored: 1, 3) -> rows r, r + 2; their elements are neighbours
            const int kk = MIR ? 1 : 0;
            const int64_t E0 = (T.tbase[0] << 8) + u;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t rk = r + 2 * j, pk = p0 + kk + 2 * j;
                if (rk >= 1 && rk <= n && pk >= 0 && (!MIR || u + j >= 0)) {
                    const int64_t rw = prow((rk), n1 - 1);
                    opt[rw] = (int32_t)pk; nnopt[rw] = cnt[E0 + j]; if (HYP) nlopt[rw] = cnt2[E0 + j];
                }
            }
            continue;
        }
        const bool rok = cov && r >= 1 && r <= n && u >= 0;
        if (rok) {
            if (b >= 2) {
                const int4 t = *reinterpret_cast<const int4 *>(cnt + E);
                c[3] = t.x; c[2] = t.y; c[1] = t.z; c[0] = t.w;
                if (HYP) { const int4 t2 = *reinterpret_cast<const int4 *>(cnt2 + E); d[3] = t2.x; d[2] = t2.y; d[1] = t2.z; d[0] = t2.w; }
            } else {
                const int2 t = *reinterpret_cast<const int2 *>(cnt + E);
                c[k0 + 1] = t.x; c[k0] = t.y;
                if (HYP) { const int2 t2 = *reinterpret_cast<const int2 *>(cnt2 + E); d[k0 + 1] = t2.x; d[k0] = t2.y; }
            }
        }
        const int32_t posr = pos[rok ? r : 0];
        Best<TC, HYP> x; best_clear(x);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (b == 1 && (k < k0 || k > k0 + 1)) continue;
            if (!rok || p0 + k < 0) continue;               // (mirrored heads: a block may be cut off at column 0)
            Best<TC, HYP> cc; best_clear(cc);
            cc.v = cadd(wv[k], dm_apply_affine(M, alpha, r - (p0 + k), (int64_t)(posr - pv[k]), (int64_t)c[k], (int64_t)d[k]));
            cc.p = (int32_t)(p0 + k); cc.nn = c[k]; best_set_nl(cc, d[k]);
            if (ra_takes(x, cc)) x = cc;
        }
        const int lpr = b <= 2 ? 1 : b >= 8 ? 64 : (1 << (b - 2));          // lanes per row
        for (int o = 1; o < lpr; o <<= 1) {                 // butterfly inside the row's lanes: every lane ends with the winner
            Best<TC, HYP> cc; best_clear(cc);
            cc.v = shfl64(x.v, lane ^ o); cc.p = __shfl(x.p, lane ^ o); cc.nn = __shfl(x.nn, lane ^ o);
            if (HYP) best_set_nl(cc, __shfl(best_nl(x), lane ^ o));
            if (ra_takes(x, cc)) x = cc;
        }
        if ((lane & (lpr - 1)) == 0 && rok) {
            if (b <= 8) {
                if (x.p >= 0) {
                    const int64_t rw = (int64_t)b * n1 + prow((r), n1 - 1);
                    opt[rw] = x.p; nnopt[rw] = x.nn;
                    if (HYP) nlopt[rw] = best_nl(x);
                }
            } else {
                // lane 0: the wave's smallest element of the row is that of its last column
                const int64_t el = (u << b) | (mask - ((Z0 + LT - 1) & mask));
                part[T.tbase[b] + (el >> 8) - T.tbase[9]] = x;
            }
        }
    }
}

// rows of more than LT candidates (b >= 9): one wave per row merges the row's tile partials
template <typename TC, bool HYP>
__global__ void __launch_bounds__(256) k_ra_merge(RATab T, int64_t nrow, const Best<TC, HYP> *__restrict__ part,
                                                  int32_t *__restrict__ opt, int32_t *__restrict__ nnopt, int32_t *__restrict__ nlopt)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nrow) return;
    int b = 9;
    while (w >= T.rbase[b + 1]) b++;
    const int64_t u = w - T.rbase[b], r = ra_row(T, b, u), n1 = T.n + 1;
    const int64_t t0 = T.tbase[b] + (u << (b - 8)) - T.tbase[9], cntt = (int64_t)1 << (b - 8);
    Best<TC, HYP> x; best_clear(x);
    // (the top row's block is half the matrix -- 2^15 partials at n = 10^7: eight loads per lane in flight; one at a time, that row
    //  alone made the kernel 160 us long)
    for (int64_t kb = lane; kb < cntt; kb += 512) {
        Best<TC, HYP> cc[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { best_clear(cc[u]); if (kb + 64 * u < cntt) cc[u] = part[t0 + kb + 64 * u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) if (kb + 64 * u < cntt && ra_takes(x, cc[u])) x = cc[u];
    }
    for (int o = 32; o > 0; o >>= 1) {
        Best<TC, HYP> c; best_clear(c);
        c.v = shfl64(x.v, lane ^ o); c.p = __shfl(x.p, lane ^ o); c.nn = __shfl(x.nn, lane ^ o);
        if (HYP) best_set_nl(c, __shfl(best_nl(x), lane ^ o));
        if (ra_takes(x, c)) x = c;
    }
    if (lane == 0 && r <= T.n) {
        int64_t rw = (int64_t)b * n1 + prow((r), n1 - 1);
        opt[rw] = x.p; nnopt[rw] = x.nn;
        if (HYP) nlopt[rw] = best_nl(x);
    }
}

// ------------------------------------------------------------------ end of a round's counting phase
// The verdict on a round's scan totals, by one thread: derives the tile count and checks the totals against the capacities of
// the buffers the host sized from its prediction (the previous layer); on overflow -- or a flag set earlier in the round -- the
// round's work is dropped (T, NT, nlong, nown read as 0 by every later kernel of the round) and the flag makes the host redo the layer.
__device__ __forceinline__ void round_verdict(RoundCounts *__restrict__ rc, int64_t capT, int64_t capNT)
{
    int64_t T = __hip_atomic_load(&rc->T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t NT = __hip_atomic_load(&rc->NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (T > capT || NT > capNT || rc->err) { rc->err = 1; rc->T = 0; rc->NT = 0; rc->nlong = 0; rc->nown = 0; T = 0; }
    rc->ntile = (int32_t)((T + LT - 1) / LT);
}
// (task lists beyond LB_MAX entries are scanned by the three-launch form: the verdict as a launch of its own)
__global__ void k_round_finish(RoundCounts *__restrict__ rc, int64_t capT, int64_t capNT) { round_verdict(rc, capT, capNT); }

// One launch for len -> offs (total T), o_ntl -> o_toffs (total NT) and the verdict.  The first nbA tickets are the blocks of the
// first scan, the rest those of the second (status words st[nbA ..]): a block still waits only for blocks of its own scan with
// lower tickets.  Each scan's total is written by one thread, which then counts itself in ticket[1]; the one that finds the
// other already counted (the counter stood at `done0` when the launch began: the host counts two per launch) gives the
// verdict.  (By then every block that has work has read its element count: the verdict may zero nlong / nown under the blocks
// that start later -- they are beyond the last block of either count and return.)  The counts are clamped to the sizes the
// grid was made for (nmaxA / nmaxB; a count beyond them has set err in k_setup_short): each range always holds the block
// that writes its total, so the verdict is given in every launch, as it was by a kernel of its own.
__global__ void __launch_bounds__(SCAN_T) k_round_scans(RoundCounts *__restrict__ rc, const int32_t *__restrict__ len, int64_t *__restrict__ offs,
                                                        const int32_t *__restrict__ ntl, int64_t *__restrict__ toffs, uint32_t nbA, int two,
                                                        int64_t nmaxA, int64_t nmaxB, int64_t capT, int64_t capNT, unsigned long long *__restrict__ st,
                                                        uint32_t *__restrict__ ticket, uint32_t tbase, uint32_t epoch, uint32_t done0)
{
    __shared__ int64_t sh[SCAN_T];
    __shared__ uint32_t s_bid;
    __shared__ int64_t s_prefix;
    if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1u) - tbase;
    __syncthreads();
    const uint32_t bid = s_bid;
    const bool second = bid >= nbA;
    int64_t n = second ? (int64_t)rc->nown : (int64_t)rc->nlong;
    const int64_t nmax = second ? nmaxB : nmaxA;
    n = n < 0 ? 0 : (n > nmax ? nmax : n);
    const bool wrote = second ? scan_lb_block(ntl, toffs, n, &rc->NT, st + nbA, (int64_t)(bid - nbA), epoch, sh, &s_prefix)
                              : scan_lb_block(len, offs, n, &rc->T, st, (int64_t)bid, epoch, sh, &s_prefix);
    if (wrote && (!two || __hip_atomic_fetch_add(ticket + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) - done0 == 1u))
        round_verdict(rc, capT, capNT);
}

// host side of k_round_scans: lenA[0 .. rc->nlong) -> offs, lenB[0 .. rc->nown) -> toffs (two = false: the first only)
static void launch_round_scans(RoundCounts *rc, const int32_t *lenA, int64_t *offs, int64_t nmaxA, const int32_t *lenB, int64_t *toffs, int64_t nmaxB,
                               bool two, int64_t capT, int64_t capNT, ScanWS &ws, hipStream_t s)
{
    if (nmaxA < 0) nmaxA = 0;
    if (nmaxB < 0) nmaxB = 0;
    const int64_t nbA = nmaxA / SCAN_TILE + 1, nbB = two ? nmaxB / SCAN_TILE + 1 : 0;      // (each covers the block that holds index n == n_max)
    const uint32_t tbase = scan_ws_begin(ws, nbA + nbB, s);
    const uint32_t done0 = ws.pairs;
    if (two) ws.pairs += 2u;
    hipLaunchKernelGGL(k_round_scans, dim3((unsigned)(nbA + nbB)), dim3(SCAN_T), 0, s, rc, lenA, offs, lenB, toffs, (uint32_t)nbA, two ? 1 : 0,
                       nmaxA, nmaxB, capT, capNT, ws.st.p, ws.ticket.p, tbase, ws.epoch, done0);
    CP_HIP(hipGetLastError());
}

// Test entry (cp_test_round_scans): the launch above on host arrays with the counts na / nb on the device (grids for na_max / nb_max),
// `reps` times on one ScanWS (tickets, epochs and the totals' counter go on from launch to launch).
// res: {T, NT, nlong, nown, ntile, err} after the last launch; offs_out: na + 1 values, toffs_out: nb + 1 values (what the scans wrote).
void dp_round_scans_test(const int32_t *a, int64_t na, int64_t na_max, const int32_t *b, int64_t nb, int64_t nb_max, int two, int64_t capT, int64_t capNT,
                         int err_in, int reps, int64_t *offs_out, int64_t *toffs_out, int64_t *res)
{
    CP_REQUIRE(na >= 0 && nb >= 0 && na <= na_max && nb <= nb_max && na_max < INT32_MAX && nb_max < INT32_MAX && reps >= 1, CP_EINVAL, "round scans test: bad sizes");
    hipStream_t s = nullptr;
    DBuf<int32_t> da((size_t)na_max + 1), db((size_t)nb_max + 1);
    DBuf<int64_t> doffs((size_t)na_max + 2), dtoffs((size_t)nb_max + 2);
    DBuf<RoundCounts> drc(1);
    ScanWS ws;
    // (entries beyond the counts hold a value that would show in any sum that read them)
    CP_HIP(hipMemsetAsync(da.p, 0x01, da.bytes(), s));
    CP_HIP(hipMemsetAsync(db.p, 0x01, db.bytes(), s));
    if (na > 0) CP_HIP(hipMemcpyAsync(da.p, a, sizeof(int32_t) * (size_t)na, hipMemcpyHostToDevice, s));
    if (nb > 0) CP_HIP(hipMemcpyAsync(db.p, b, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, s));
    RoundCounts h;
    for (int r = 0; r < reps; r++) {
        memset(&h, 0, sizeof(h));
        h.nlong = (int32_t)na; h.nown = (int32_t)nb; h.err = err_in;
        CP_HIP(hipMemsetAsync(doffs.p, 0xFF, doffs.bytes(), s));
        CP_HIP(hipMemsetAsync(dtoffs.p, 0xFF, dtoffs.bytes(), s));
        CP_HIP(hipMemcpyAsync(drc.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
        CP_HIP(hipStreamSynchronize(s));               // (h is reused)
        launch_round_scans(drc.p, da.p, doffs.p, na_max, db.p, dtoffs.p, nb_max, two != 0, capT, capNT, ws, s);
    }
    CP_HIP(hipMemcpyAsync(&h, drc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(offs_out, doffs.p, sizeof(int64_t) * (size_t)(na + 1), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(toffs_out, dtoffs.p, sizeof(int64_t) * (size_t)(nb + 1), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    res[0] = h.T; res[1] = h.NT; res[2] = h.nlong; res[3] = h.nown; res[4] = h.ntile; res[5] = h.err;
}

// Test entry (cp_test_list_alloc): the block-level allocation of k_setup_short (alloc_wave / alloc_reserve / alloc_place) and its
// closing (round_alloc_finish) on host arrays of lengths.  Lane i appends a[i] units to the first list (i < na) and b[i] tiles to
// the second (i < nb); blocks of `bs` lanes, and one block more that appends nothing.
// The sequence wave prefix / reserve / publish / place is spelled again here (k_setup_short spreads it over its short-task walk to
// hide the atomics' round trips): this entry proves the helpers, not their wiring in set-up -- s_wcnt against the indices of
// alloc_place and the o_cap branch there are covered by the layer-parity tests only.
__global__ void __launch_bounds__(1024) k_list_alloc_test(RoundCounts *rc, const int32_t *__restrict__ a, int64_t na, const int32_t *__restrict__ b, int64_t nb,
                                                          int64_t *__restrict__ offs, int64_t *__restrict__ toffs, int32_t *__restrict__ ioffs,
                                                          int32_t *__restrict__ slot_a, int32_t *__restrict__ slot_b, int64_t capT, int64_t capNT, int32_t o_cap)
{
    __shared__ AllocSh S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool onA = i < na, onB = i < nb;
    const int32_t la = onA ? a[i] : 0, lb = onB ? b[i] : 0;
    const unsigned long long ml = __ballot(onA), mo = __ballot(onB);
    int32_t pre_l = 0, pre_o = 0, pre_i = 0;
    unsigned long long wt_l = 0, wt_o = 0; int32_t wt_i = 0;
    if (ml) wt_l = alloc_wave(onA, la, lane, ml, pre_l);
    if (mo) {
        wt_o = alloc_wave(onB, lb, lane, mo, pre_o);
        const int32_t it = fix_items_of(lb);
        wt_i = (int32_t)(alloc_wave(it > 0, it, lane, 0ull, pre_i) & ALLOC_MASK);
    }
    if (lane == 0) { S.wpre[0][wv] = wt_l; S.wpre[1][wv] = wt_o; S.wit[wv] = wt_i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b0, b1; int32_t bi;
        alloc_reserve(S, (int)(blockDim.x >> 6), rc, true, b0, b1, bi);
        alloc_publish(S, b0, b1, bi);
    }
    __syncthreads();
    if (onA) { int32_t idx; int64_t off; alloc_place(S, 0, wv, lane, ml, pre_l, idx, off); offs[idx] = off; slot_a[i] = idx; }
    if (onB) {
        int32_t idx; int64_t off;
        alloc_place(S, 1, wv, lane, mo, pre_o, idx, off);
        slot_b[i] = idx;
        if (idx >= o_cap) rc->err = 1;
        else { toffs[idx] = off; ioffs[idx] = S.ibase + S.wit[wv] + pre_i; }
    }
    round_alloc_finish(rc, offs, toffs, capT, capNT, (int64_t)o_cap, gridDim.x);
}

// res: {T, NT, nlong, nown, ntile, err, n_items, the ticket, the two packed words or-ed} after the last of `reps` launches on one record,
// then round_alloc_fits(fit_ntask, fit_n, fit_own_min).  offs_out: na + 1 values by slot, slot_a: the slot of lane i; toffs_out,
// slot_b, ioffs_out (by slot) likewise.  o_cap: slots of the second list.
void dp_list_alloc_test(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int bs, int64_t capT, int64_t capNT, int64_t o_cap, int err_in, int reps,
                        int64_t fit_ntask, int64_t fit_n, int64_t fit_own_min, int64_t *offs_out, int32_t *slot_a, int64_t *toffs_out, int32_t *slot_b,
                        int32_t *ioffs_out, int64_t *res)
{
    CP_REQUIRE(na >= 0 && nb >= 0 && na < ((int64_t)1 << 24) && nb < ((int64_t)1 << 24) && reps >= 1 && bs >= 64 && bs <= 1024 && bs % 64 == 0 && o_cap >= 0 &&
               o_cap <= nb, CP_EINVAL, "list alloc test: bad sizes");
    hipStream_t s = nullptr;
    DBuf<int32_t> da((size_t)na + 1), db((size_t)nb + 1), dsa((size_t)na + 1), dsb((size_t)nb + 1), dio((size_t)nb + 1);
    DBuf<int64_t> doffs((size_t)na + 1), dtoffs((size_t)nb + 1);
    DBuf<RoundCounts> drc(1);
    if (na > 0) CP_HIP(hipMemcpyAsync(da.p, a, sizeof(int32_t) * (size_t)na, hipMemcpyHostToDevice, s));
    if (nb > 0) CP_HIP(hipMemcpyAsync(db.p, b, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, s));
    RoundCounts h;
    memset(&h, 0, sizeof(h));
    CP_HIP(hipMemcpyAsync(drc.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
    const unsigned grid = (unsigned)(cdiv(std::max(na, nb), (int64_t)bs) + 1);
    for (int r = 0; r < reps; r++) {
        // (the record goes on from launch to launch: the ticket and the packed words come back as zeros; the counts are set again)
        CP_HIP(hipMemsetAsync(&drc.p->err, 0, sizeof(int32_t), s));
        if (err_in) CP_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&drc.p->err), 1, 1, s));
        CP_HIP(hipMemsetAsync(&drc.p->n_items, 0, sizeof(int32_t), s));
        CP_HIP(hipMemsetAsync(doffs.p, 0xFF, doffs.bytes(), s)); CP_HIP(hipMemsetAsync(dtoffs.p, 0xFF, dtoffs.bytes(), s));
        CP_HIP(hipMemsetAsync(dsa.p, 0xFF, dsa.bytes(), s)); CP_HIP(hipMemsetAsync(dsb.p, 0xFF, dsb.bytes(), s)); CP_HIP(hipMemsetAsync(dio.p, 0xFF, dio.bytes(), s));
        hipLaunchKernelGGL(k_list_alloc_test, dim3(grid), dim3((unsigned)bs), 0, s, drc.p, da.p, na, db.p, nb, doffs.p, dtoffs.p, dio.p, dsa.p, dsb.p, capT, capNT,
                           (int32_t)o_cap);
        CP_HIP(hipGetLastError());
    }
    CP_HIP(hipMemcpyAsync(&h, drc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(offs_out, doffs.p, sizeof(int64_t) * (size_t)(na + 1), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(toffs_out, dtoffs.p, sizeof(int64_t) * (size_t)(nb + 1), hipMemcpyDeviceToHost, s));
    if (na > 0) CP_HIP(hipMemcpyAsync(slot_a, dsa.p, sizeof(int32_t) * (size_t)na, hipMemcpyDeviceToHost, s));
    if (nb > 0) CP_HIP(hipMemcpyAsync(slot_b, dsb.p, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, s));
    if (nb > 0) CP_HIP(hipMemcpyAsync(ioffs_out, dio.p, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    res[0] = h.T; res[1] = h.NT; res[2] = h.nlong; res[3] = h.nown; res[4] = h.ntile; res[5] = h.err; res[6] = h.n_items; res[7] = h.a_ticket;
    res[8] = (int64_t)(h.alloc_l | h.alloc_o); res[9] = round_alloc_fits(fit_ntask, fit_n, fit_own_min) ? 1 : 0;
}

// ------------------------------------------------------------------ host side of the own-tile merge (k_fix_own)
// the grid, from what the host knows: the round's tiles (predicted or exact) and tasks.  Both roles walk their device-side
// counts with grid strides, so a count beyond the estimate costs time only.
struct FixGrid { int iblocks, lblocks; };
static FixGrid fix_grid(int64_t nt, int64_t ntask)
{
    nt = std::max<int64_t>(nt, 0); ntask = std::max<int64_t>(ntask, 0);
    const int64_t items = nt / FIX_TRIP + std::min<int64_t>(ntask, nt / (FIX_SERIAL + 1)) + 1;
    FixGrid g;
    g.iblocks = (int)std::min<int64_t>(items, 2048);
    g.lblocks = (int)std::min<int64_t>(std::max<int64_t>(cdiv(ntask, (int64_t)256), 1), 4096);
    return g;
}
template <typename TC, bool HYP>
static void launch_fix_own(hipStream_t s, RoundCounts *rc, const int64_t *toffs, const Best<TC, HYP> *part, const int4 *tdesc, const uint8_t *tb,
                           const int32_t *tS0l, const int32_t *tileS, const int32_t *tileS2, const DevModel<TC> &M, int32_t *opt, int32_t *nnopt,
                           int32_t *nlopt, int64_t n, const int2 *items, const int32_t *item_of, unsigned long long *trec, uint32_t *tick,
                           int64_t nt, int64_t ntask, const int32_t *ioffs)
{
    const FixGrid g = fix_grid(nt, ntask);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fix_own<TC, HYP>), dim3((unsigned)(g.iblocks + g.lblocks)), dim3(256), 0, s, rc, toffs, part, tdesc, tb, tS0l, tileS,
                       tileS2, M, opt, nnopt, nlopt, n + 1, items, item_of, trec, tick, g.iblocks, ioffs);
    CP_HIP(hipGetLastError());
}

// Test entry (cp_test_fix_merge): k_own_map (tiles counted from the task heads: it lists the items) and the merge launch on host
// arrays, `reps` times on one workspace (the tickets must come back to zero).  Task t has the tiles toffs[t] .. toffs[t + 1),
// partial records {part_v (the value's 8 bytes), part_p (< 0: an empty tile), part_nn, part_nl}, tile counts tile_s / tile_s2,
// anchors anchor / anchor2 and writes its winner to the cell of (plane[t], row[t]) of planes over the rows 0 .. n.
// res: {items listed, tasks folded from more than one trip, the edge bits, tickets left nonzero} of the last launch.
template <typename TC, bool HYP>
static void fix_merge_test_run(const cp_model_t *model, int64_t ntask, const int64_t *toffs, const int64_t *part_v, const int32_t *part_p, const int32_t *part_nn,
                               const int32_t *part_nl, const int32_t *tile_s, const int32_t *tile_s2, const int32_t *anchor, const int32_t *anchor2,
                               const int32_t *row, const int32_t *plane, int64_t n, int reps, int32_t *p_out, int32_t *nn_out, int32_t *nl_out, int64_t *res)
{
    hipStream_t s = nullptr;
    const int64_t NT = toffs[ntask], n1 = n + 1;
    int np = 1;
    for (int64_t t = 0; t < ntask; t++) np = std::max(np, plane[t] + 1);
    std::vector<Best<TC, HYP>> hpart((size_t)NT);
    for (int64_t k = 0; k < NT; k++) {
        Best<TC, HYP> b;
        memset(&b, 0, sizeof(b));
        memcpy(&b.v, part_v + k, sizeof(TC)); b.p = part_p[k]; b.nn = part_nn[k];
        if constexpr (HYP) b.nl = part_nl[k];
        hpart[(size_t)k] = b;
    }
    std::vector<int4> htd((size_t)ntask);
    std::vector<uint8_t> htb((size_t)ntask);
    std::vector<int32_t> hrlen((size_t)ntask);
    for (int64_t t = 0; t < ntask; t++) {
        htd[(size_t)t] = make_int4(0, anchor[t], row[t], 0); htb[(size_t)t] = (uint8_t)plane[t];
        hrlen[(size_t)t] = (int32_t)std::min<int64_t>((toffs[t + 1] - toffs[t]) * LT, INT32_MAX);
    }
    HostModel<TC> HM;
    build_dev_model<TC>(model, HM, s);
    const size_t c = (size_t)NT, icap = fix_items_cap(c), pl = (size_t)np * (size_t)n1;
    DBuf<int64_t> dtoffs((size_t)ntask + 1);
    DBuf<Best<TC, HYP>> dpart(c);
    DBuf<int4> dtd((size_t)ntask), drec(c);
    DBuf<uint8_t> dtb((size_t)ntask);
    DBuf<int32_t> drlen((size_t)ntask), dS0l((size_t)ntask), dS(c), dS2(c), dtask(c), ditem_of(c), dopt(pl), dnn(pl), dnl(pl);
    DBuf<int2> ditems(icap);
    DBuf<unsigned long long> dtrec(icap * FIX_REC_W);
    DBuf<uint32_t> dtick((size_t)ntask);
    DBuf<RoundCounts> drc(1);
    auto up = [&](void *d, const void *h, size_t bytes) { CP_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s)); };
    up(dtoffs.p, toffs, dtoffs.bytes()); up(dpart.p, hpart.data(), dpart.bytes()); up(dtd.p, htd.data(), dtd.bytes()); up(dtb.p, htb.data(), dtb.bytes());
    up(drlen.p, hrlen.data(), drlen.bytes()); up(dS.p, tile_s, dS.bytes());
    if (HYP) { up(dS0l.p, anchor2, dS0l.bytes()); up(dS2.p, tile_s2, dS2.bytes()); }
    CP_HIP(hipMemsetAsync(dtick.p, 0, dtick.bytes(), s));
    // round_alloc: the items' bases as set-up reserves them (here: in task order) and their number; 0: k_own_map draws them
    std::vector<int32_t> hioffs((size_t)ntask);
    int32_t n_items0 = 0;
    for (int64_t t = 0; t < ntask; t++) {
        hioffs[(size_t)t] = n_items0;
        n_items0 += fix_items_of(toffs[t + 1] - toffs[t]);
    }
    DBuf<int32_t> dioffs((size_t)ntask);
    up(dioffs.p, hioffs.data(), dioffs.bytes());
    const int32_t *ioffs = g_opt_round_alloc ? dioffs.p : nullptr;
    RoundCounts h;
    for (int r = 0; r < reps; r++) {
        memset(&h, 0, sizeof(h));
        h.nown = (int32_t)ntask; h.NT = NT; h.n_items = ioffs ? n_items0 : 0;
        up(drc.p, &h, sizeof(h));
        // (whatever a launch does not write shows: no column, and records / items of the launch before are gone)
        CP_HIP(hipMemsetAsync(dopt.p, 0xFF, dopt.bytes(), s)); CP_HIP(hipMemsetAsync(dnn.p, 0xFF, dnn.bytes(), s)); CP_HIP(hipMemsetAsync(dnl.p, 0xFF, dnl.bytes(), s));
        CP_HIP(hipMemsetAsync(ditems.p, 0x7F, ditems.bytes(), s)); CP_HIP(hipMemsetAsync(ditem_of.p, 0x7F, ditem_of.bytes(), s));
        CP_HIP(hipMemsetAsync(dtrec.p, 0x7F, dtrec.bytes(), s));
        hipLaunchKernelGGL(k_own_map, dim3((unsigned)std::min<int64_t>(cdiv(NT, (int64_t)256), 8192)), dim3(256), 0, s, drc.p, dtoffs.p, dtd.p, drlen.p, drec.p,
                           dtask.p, dtb.p, (int32_t *)nullptr, 0, n, 0, (int32_t *)nullptr, (int32_t *)nullptr, ditems.p, ditem_of.p, 0, ioffs);
        launch_fix_own<TC, HYP>(s, drc.p, dtoffs.p, dpart.p, dtd.p, dtb.p, HYP ? dS0l.p : nullptr, dS.p, HYP ? dS2.p : nullptr, HM.d, dopt.p, dnn.p, HYP ? dnl.p : nullptr, n,
                                ditems.p, ditem_of.p, dtrec.p, dtick.p, NT, ntask, ioffs);
        CP_HIP(hipMemcpyAsync(&h, drc.p, sizeof(h), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));               // (h is reused)
        g_fix_items += h.n_items;
    }
    std::vector<int32_t> hopt(pl), hnn(pl), hnl(HYP ? pl : 0);
    std::vector<uint32_t> htick((size_t)ntask);
    CP_HIP(hipMemcpyAsync(hopt.data(), dopt.p, dopt.bytes(), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(hnn.data(), dnn.p, dnn.bytes(), hipMemcpyDeviceToHost, s));
    if (HYP) CP_HIP(hipMemcpyAsync(hnl.data(), dnl.p, dnl.bytes(), hipMemcpyDeviceToHost, s));
    CP_HIP(hipMemcpyAsync(htick.data(), dtick.p, dtick.bytes(), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    int64_t left = 0;
    for (int64_t t = 0; t < ntask; t++) {
        const int64_t r = row[t];
        const int lv = __builtin_ctzll((unsigned long long)r);                  // prow on the host
        const size_t cell = (size_t)plane[t] * (size_t)n1 + (size_t)((n - (n >> lv)) + (r >> (lv + 1)));
        p_out[t] = hopt[cell]; nn_out[t] = hnn[cell];
        if (HYP) nl_out[t] = hnl[cell];
        left += htick[(size_t)t] != 0;
    }
    res[0] = h.n_items; res[1] = h.n_trips; res[2] = h.n_edge; res[3] = left;
}

void dp_fix_merge_test(const cp_model_t *model, int64_t ntask, const int64_t *toffs, const int64_t *part_v, const int32_t *part_p, const int32_t *part_nn,
                       const int32_t *part_nl, const int32_t *tile_s, const int32_t *tile_s2, const int32_t *anchor, const int32_t *anchor2, const int32_t *row,
                       const int32_t *plane, int64_t n, int reps, int32_t *p_out, int32_t *nn_out, int32_t *nl_out, int64_t *res)
{
    const bool hyp = model->kind == CP_MODEL_HYPEREDGE_CUT;
    CP_REQUIRE(model->kind == CP_MODEL_WORK || model->kind == CP_MODEL_CONNECTIVITY || hyp, CP_EINVAL, "fix merge test: not a model of the O(n log^2 n) scheme");
    CP_REQUIRE(!hyp || (part_nl && tile_s2 && anchor2 && nl_out), CP_EINVAL, "fix merge test: a hyperedge model needs the second counts");
    CP_REQUIRE(ntask >= 1 && ntask < ((int64_t)1 << 24) && n >= 1 && n < ((int64_t)1 << 26) && reps >= 1 && reps <= 16, CP_EINVAL, "fix merge test: bad sizes");
    CP_REQUIRE(toffs[0] == 0, CP_EINVAL, "fix merge test: toffs must start at 0");
    for (int64_t t = 0; t < ntask; t++) {
        CP_REQUIRE(toffs[t + 1] > toffs[t] && toffs[t + 1] < ((int64_t)1 << 26), CP_EINVAL, "fix merge test: every task needs a tile, 2^26 tiles at most");
        CP_REQUIRE(row[t] >= 1 && row[t] <= n && plane[t] >= 0 && plane[t] < 4, CP_EINVAL, "fix merge test: rows are 1 .. n, planes 0 .. 3");
    }
    with_cost_type(model->dtype, [&](auto tag) {
        using TC = decltype(tag);
        if (hyp) fix_merge_test_run<TC, true>(model, ntask, toffs, part_v, part_p, part_nn, part_nl, tile_s, tile_s2, anchor, anchor2, row, plane, n, reps, p_out, nn_out, nl_out, res);
        else fix_merge_test_run<TC, false>(model, ntask, toffs, part_v, part_p, part_nn, part_nl, tile_s, tile_s2, anchor, anchor2, row, plane, n, reps, p_out, nn_out, nl_out, res);
    });
}

// ------------------------------------------------------------------ the link entries split by plane (own_split; SplitLinks: dp_total.hpp)
__device__ __forceinline__ int split_plane(int32_t p, int32_t x) { return 31 - __clz((int)(p ^ x)); }       // (-1 for x == p)

// one lane per column: cnt[b][p] = the column's entries with h == SPLIT_BMIN + b (column n: none)
__global__ void __launch_bounds__(256) k_split_count(const int32_t *__restrict__ pos, const int32_t *__restrict__ next, int64_t n, int nb,
                                                     int32_t *__restrict__ cnt)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    int32_t c[SPLIT_NB];
#pragma unroll
    for (int b = 0; b < SPLIT_NB; b++) c[b] = 0;
    if (p < n)
        for (int32_t q = pos[p], qe = pos[p + 1]; q < qe; q++) {
            const int h = split_plane((int32_t)p, next[q]) - SPLIT_BMIN;
#pragma unroll
            for (int b = 0; b < SPLIT_NB; b++) c[b] += (h == b);
        }
#pragma unroll
    for (int b = 0; b < SPLIT_NB; b++) if (b < nb) cnt[(int64_t)b * (n + 1) + p] = c[b];
}

// one lane per column, one block per 256-column block: the column's variable entries to their planes, in entry order, and the packed
// words (SplitLinks) -- with  vsa[b][p] = sum over b' > b of (vpos[b'][p] - vpos[b'][0])  the column's two in-block offsets, from the
// bases thread 0 (the block's first column) leaves in LDS and in vbase; they go where the counts were.  Both offsets grow with p, so a
// block's last column holds its largest ones: it alone raises vmax (and reads it first: few blocks get as far as the atomic).
__global__ void __launch_bounds__(256) k_split_scatter(const int32_t *__restrict__ pos, const int32_t *__restrict__ next, int64_t n, int nb,
                                                       const int32_t *__restrict__ vpos, int32_t *__restrict__ vnext, int32_t *__restrict__ vpk,
                                                       int2 *__restrict__ vbase, int64_t nblk, int32_t *__restrict__ vmax)
{
    __shared__ int32_t s_bp[SPLIT_NB], s_bs[SPLIT_NB];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p <= n;
    int32_t c[SPLIT_NB];
#pragma unroll
    for (int b = 0; b < SPLIT_NB; b++) c[b] = (b < nb && live) ? vpos[(int64_t)b * (n + 1) + p] : 0;
    if (threadIdx.x == 0) {                          // (p <= n: the grid has no block without a column)
        int32_t above = 0;
#pragma unroll
        for (int b = SPLIT_NB - 1; b >= 0; b--)
            if (b < nb) {
                s_bp[b] = c[b]; s_bs[b] = above;
                vbase[(int64_t)b * (nblk + 1) + blockIdx.x] = make_int2(c[b], above);
                if ((int64_t)blockIdx.x == nblk - 1) vbase[(int64_t)b * (nblk + 1) + nblk] = make_int2(vpos[(int64_t)(b + 1) * (n + 1)], 0);
                above += c[b] - vpos[(int64_t)b * (n + 1)];
            }
    }
    __syncthreads();
    if (live) {
        int32_t above = 0, mp = 0, ms = 0;
#pragma unroll
        for (int b = SPLIT_NB - 1; b >= 0; b--)
            if (b < nb) {
                const int32_t op = c[b] - s_bp[b], os = above - s_bs[b];
                vpk[(int64_t)b * (n + 1) + p] = (int32_t)(((uint32_t)op & 0xffffu) | ((uint32_t)os << 16));
                mp = op > mp ? op : mp; ms = os > ms ? os : ms;
                above += c[b] - vpos[(int64_t)b * (n + 1)];
            }
        if (threadIdx.x == 255 || p == n) {
            if (mp > vmax[0]) atomicMax(&vmax[0], mp);
            if (ms > vmax[1]) atomicMax(&vmax[1], ms);
        }
    }
    if (p < n)
        for (int32_t q = pos[p], qe = pos[p + 1]; q < qe; q++) {
            const int32_t x = next[q];
            const int h = split_plane((int32_t)p, x) - SPLIT_BMIN;
            int32_t dst = -1;
#pragma unroll
            for (int b = 0; b < SPLIT_NB; b++) if (h == b) { dst = c[b]; c[b]++; }
            if (dst >= 0) vnext[dst] = x;
        }
}

// one lane per column: the wide vsa from vpos (split_wide)
__global__ void __launch_bounds__(256) k_split_vsa(int64_t n, int nb, const int32_t *__restrict__ vpos, int32_t *__restrict__ vsa)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    int32_t above = 0;
    for (int b = nb - 1; b >= 0; b--) {
        vsa[(int64_t)b * (n + 1) + p] = above;
        above += vpos[(int64_t)b * (n + 1) + p] - vpos[(int64_t)b * (n + 1)];
    }
}

static void split_build(cp_csr_s *A, SplitLinks &S, DBuf<int64_t> &scratch)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, n1 = n + 1;
    int nbits = 1;
    while (((int64_t)1 << nbits) <= n) nbits++;
    S.nb = std::max(0, nbits - SPLIT_BMIN); S.stride = n1; S.nblk = cdiv(n1, 256);
    S.packed = false; S.has_wide = false; S.max_off[0] = S.max_off[1] = 0;
    for (auto &t : S.tot) t = 0;
    if (S.nb > 0) {
        CP_REQUIRE(S.nb <= SPLIT_NB, CP_EINVAL, "n exceeds the bit-plane budget");
        const size_t cells = (size_t)S.nb * (size_t)n1;
        S.vpos.ensure(cells + 1); S.vpk.ensure(cells + 1); S.vnext.ensure((size_t)A->N + 8);
        S.vbase.ensure((size_t)S.nb * (size_t)(S.nblk + 1)); S.vmax.ensure(2);
        const unsigned grid = (unsigned)S.nblk;
        CP_HIP(hipMemsetAsync(S.vmax.p, 0, 2 * sizeof(int32_t), s));
        // (the counts live in vpk until the scatter writes it)
        hipLaunchKernelGGL(k_split_count, dim3(grid), dim3(256), 0, s, A->pos32.p, A->next.p, n, S.nb, S.vpk.p);
        exclusive_scan_i32_i32(S.vpk.p, S.vpos.p, (int64_t)cells, scratch, s);
        hipLaunchKernelGGL(k_split_scatter, dim3(grid), dim3(256), 0, s, A->pos32.p, A->next.p, n, S.nb, S.vpos.p, S.vnext.p, S.vpk.p, S.vbase.p, S.nblk,
                           S.vmax.p);
        CP_HIP(hipGetLastError());
        int32_t st[SPLIT_NB + 1];                       // the planes' starts and the total: the entries a round's planes stream
        for (int b = 0; b <= S.nb; b++)
            CP_HIP(hipMemcpyAsync(&st[b], S.vpos.p + (size_t)b * (size_t)n1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CP_HIP(hipMemcpyAsync(S.max_off, S.vmax.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CP_HIP(hipStreamSynchronize(s));
        for (int b = 0; b < S.nb; b++) S.tot[b] = (int64_t)st[b + 1] - st[b];
        S.tot[S.nb] = st[S.nb];
        S.packed = S.max_off[0] <= 0xffff && S.max_off[1] <= 0xffff;
    }
    S.built = true;
}

// the wide vsa, for whoever does not take the packed words: an offset that does not fit, own_blk 0, own_pack 0, cp_test_own_split
static void split_wide(cp_csr_s *A, SplitLinks &S)
{
    if (S.has_wide) return;
    if (S.nb > 0) {
        S.vsa.ensure((size_t)S.nb * (size_t)S.stride + 1);
        hipLaunchKernelGGL(k_split_vsa, dim3((unsigned)S.nblk), dim3(256), 0, A->stream, A->n, S.nb, S.vpos.p, S.vsa.p);
        CP_HIP(hipGetLastError());
    }
    S.has_wide = true;
}

// Test entry (cp_test_own_pair): what own_pair_slots gives wave `wave` among nt tiles -- the function the kernel calls
void dp_own_pair_test(int64_t nt, int64_t wave, int64_t *res)
{
    int64_t s0 = 0, s1 = 0;
    res[0] = own_pair_slots(wave, nt, s0, s1) ? 1 : 0;
    res[1] = s0;
    res[2] = s1;
}

// Test entry (cp_test_own_split): the three arrays of the pattern on the host.  vpos_out / vsa_out: nb (n + 1) words, vnext_out: room
// for the N entries; res: {nb, entries in vnext}.
void dp_own_split_test(cp_csr_s *A, int32_t *vpos_out, int32_t *vsa_out, int32_t *vnext_out, int64_t *res)
{
    ensure_links(A);
    SplitLinks S;
    DBuf<int64_t> scratch;
    split_build(A, S, scratch);
    split_wide(A, S);
    res[0] = S.nb; res[1] = S.tot[S.nb];
    if (S.nb <= 0) return;
    const size_t cells = (size_t)S.nb * (size_t)S.stride;
    CP_HIP(hipMemcpyAsync(vpos_out, S.vpos.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipMemcpyAsync(vsa_out, S.vsa.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    if (res[1] > 0) CP_HIP(hipMemcpyAsync(vnext_out, S.vnext.p, (size_t)res[1] * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipStreamSynchronize(A->stream));
}

// Test entry (cp_test_own_pack): the packed words and the block bases of the pattern on the host.  vpk_out: nb (n + 1) words;
// vbase_out: nb (blocks + 1) pairs {start, prefix sum}; res: {nb, blocks per plane, packed, largest start offset, largest prefix offset}.
void dp_own_pack_test(cp_csr_s *A, int32_t *vpk_out, int32_t *vbase_out, int64_t *res)
{
    ensure_links(A);
    SplitLinks S;
    DBuf<int64_t> scratch;
    split_build(A, S, scratch);
    res[0] = S.nb; res[1] = S.nblk; res[2] = S.packed ? 1 : 0; res[3] = S.max_off[0]; res[4] = S.max_off[1];
    if (S.nb <= 0) return;
    CP_HIP(hipMemcpyAsync(vpk_out, S.vpk.p, (size_t)S.nb * (size_t)S.stride * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipMemcpyAsync(vbase_out, S.vbase.p, (size_t)S.nb * (size_t)(S.nblk + 1) * sizeof(int2), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipStreamSynchronize(A->stream));
}

// ------------------------------------------------------------------ host driver for one layer
// number of rows r <= x of the form (base << (b+1)) | (1 << b) | ((2v+1) << tau): the rows with ctz == tau whose bit b is set
static int64_t count_rows(int b, int tau, int64_t x)
{
    if (x < 0) return 0;
    int sh = b - tau - 1;
    int64_t V = (int64_t)1 << sh;
    int64_t nfull = (x + ((int64_t)1 << tau)) >> (b + 1);
    int64_t cnt = nfull * V;
    int64_t y = x - (nfull << (b + 1)) - ((int64_t)1 << b);
    if (y >= ((int64_t)1 << tau)) cnt += ((y >> tau) + 1) >> 1;
    return cnt;
}

// Rows computed by a run restricted to the row tile [rlo, rhi]: every row r with
//     r - 2^ctz(r) <= rhi  and  r + 2^ctz(r) >= rlo
// -- the tile plus the O(log n) tree ancestors its rows take their candidate bounds from (closed under ancestors).
static void make_round(RoundDesc &R, bool isA, int tau, int nbits, int64_t n, int64_t rlo, int64_t rhi, const Geo &G = Geo{0, 0, 0},
                       const int64_t *aoff = nullptr)
{
    memset(&R, 0, sizeof(R));
    R.isA = isA; R.tau = tau; R.nbits = nbits; R.n = n; R.G = G;
    if (G.win) {
        // every row takes part in every plane b <= s.  Round A: plane b holds the heads of its rectangles, the multiples of 2^b
        // (index l <-> row (l + 1) << b); round tau: every plane b in (tau, s] holds the rows with ctz == tau (index l <-> row
        // (2 l + 1) << tau).  A row tile [rlo, rhi] needs the rows within 2^tau of it in round tau (their tree neighbours are then
        // computed by the earlier rounds) and the heads within 2^(b+1) of it in plane b.
        if (aoff) for (int b = 0; b < 32; b++) R.aoff[b] = aoff[b];
        int64_t acc = 0;
        for (int b = 0; b < 36; b++) {
            R.tbase[b] = acc;
            if (b > G.s || (!isA && b <= tau)) continue;
            if (isA) {
                int64_t lo = rlo - ((int64_t)2 << b), hi = rhi + ((int64_t)1 << b);
                if (lo < ((int64_t)1 << b)) lo = (int64_t)1 << b;
                if (hi > n) hi = n;
                int64_t l0 = ((lo + ((int64_t)1 << b) - 1) >> b) - 1, l1 = (hi >> b) - 1;      // first / last head index
                R.tskip[b] = l0;
                acc += l1 >= l0 ? l1 - l0 + 1 : 0;
            } else {
                int64_t rmin = rlo - ((int64_t)1 << tau), rmax = rhi + ((int64_t)1 << tau);
                if (rmax > n) rmax = n;
                int64_t u0 = rmin <= 0 ? 0 : (((rmin - 1) >> tau) + 1) >> 1, u1 = ((rmax >> tau) + 1) >> 1;
                R.tskip[b] = u0;
                acc += u1 > u0 ? u1 - u0 : 0;
            }
        }
        R.ntask = acc;
        return;
    }
    if (isA) {
        int64_t r0 = rlo > 1 ? rlo : 1, r1 = rhi < n ? rhi : n;
        R.a_r0 = r0; R.a_nmain = r1 >= r0 ? r1 - r0 + 1 : 0;
        R.nextra = 0;
        for (int b = 0; b < nbits; b++) {            // rows with ctz == b just outside the tile
            int64_t step = (int64_t)1 << b;
            // left of the tile: r in [rlo - 2^b, rlo) ; right: r in (rhi, rhi + 2^b]
            for (int side = 0; side < 2; side++) {
                int64_t lo = side == 0 ? rlo - step : rhi + 1, hi = side == 0 ? rlo - 1 : rhi + step;
                if (lo < 1) lo = 1;
                if (hi > n) hi = n;
                for (int64_t r = ((lo + step - 1) >> b) << b; r <= hi; r += step)
                    if (r >= 1 && ((r >> b) & 1) && R.nextra < 64) R.extra[R.nextra++] = r;      // ctz(r) == b exactly
            }
        }
        R.nlast = 0;
        if (n >= 1) {
            int lowest = 0;
            while (!((n >> lowest) & 1)) lowest++;
            for (int b = lowest + 1; b < nbits; b++) if ((n >> b) & 1) R.last_b[R.nlast++] = b;
        }
        R.ntask = R.a_nmain + R.nextra + R.nlast;
        return;
    }
    int64_t rmin = rlo - ((int64_t)1 << tau), rmax = rhi + ((int64_t)1 << tau);
    if (rmax > n) rmax = n;
    int64_t acc = 0;
    for (int b = 0; b <= tau; b++) R.tbase[b] = 0;
    for (int b = tau + 1; b < nbits; b++) {
        R.tbase[b] = acc;
        int64_t skip = count_rows(b, tau, rmin - 1);
        int64_t cnt = count_rows(b, tau, rmax) - skip;
        R.tskip[b] = skip;
        acc += cnt > 0 ? cnt : 0;
    }
    for (int b = nbits; b < 36; b++) R.tbase[b] = acc;
    R.ntask = acc;
}

// Builds a cached round-A table: the counts of `levels` levels of rows_of(b) rows each (they depend on the pattern only -- once per
// partition; the table of the mirrored heads of the windowed geometry, mir_w > 0, also on the window width: once per (pattern, w),
// after win_build, whose anchors `anch` / `anch2` its counts carry).  Fills the cache's table, counts (c2: second count) and
// sizes; `part` gets room for the partials of the rows of more than LT candidates.
template <typename TC, typename Rows>
static void ra_build(cp_csr_s *A, LayerWork<TC> &Wk, RaCache<TC> &Ra, int levels, Rows rows_of, int64_t mir_w, const int32_t *anch, const int32_t *anch2)
{
    hipStream_t s = A->stream;
    const bool hyp = Wk.hyp;
    RATab &T = Ra.tab;
    memset(&T, 0, sizeof(T));
    T.nbits = levels; T.n = A->n; T.mir_w = mir_w;
    for (int b = 0; b < 33; b++) { T.tlo[b] = 0; T.thi[b] = INT64_MAX; T.aoff[b] = (mir_w && b < 32) ? Wk.win.aoff[b] : 0; }
    int64_t tb = 0, rb = 0;
    for (int b = 0; b < 33; b++) {
        T.tbase[b] = tb; T.rbase[b] = rb;
        if (b >= levels) continue;
        const int64_t nrows = rows_of(b);
        tb += cdiv(nrows << b, LT);
        if (b >= 9) rb += nrows;
    }
    Ra.ntile = tb; Ra.nrow = rb;
    const size_t total = (size_t)tb * LT;
    Ra.c.ensure(total + 8);
    if (hyp) Ra.c2.ensure(total + 8);
    Ra.part.ensure((size_t)std::max<int64_t>(1, tb - T.tbase[9]));
    if (tb > 0) {
        DBuf<int64_t> &G = Wk.sc.ra_G, &scratch = Wk.sc.scratch;        // (kept with the layer scratch: 8 B per element)
        G.ensure(total + 1);
        hipLaunchKernelGGL(k_ra_colcount, dim3((unsigned)tb), dim3(LT), 0, s, T, A->pos32.p, A->next.p, hyp ? A->fpos32.p : (const int32_t *)nullptr,
                           hyp ? A->flast.p : (const int32_t *)nullptr, Ra.c.p, hyp ? Ra.c2.p : (int32_t *)nullptr);
        exclusive_scan_i32(Ra.c.p, G.p, (int64_t)total, scratch, s);
        hipLaunchKernelGGL(k_ra_final, dim3((unsigned)tb), dim3(LT), 0, s, T, G.p, Ra.c.p, anch);
        if (hyp) {
            exclusive_scan_i32(Ra.c2.p, G.p, (int64_t)total, scratch, s);
            hipLaunchKernelGGL(k_ra_final, dim3((unsigned)tb), dim3(LT), 0, s, T, G.p, Ra.c2.p, anch2);
        }
        CP_HIP(hipGetLastError());
    }
    Ra.built = true; Ra.w = mir_w;
}
// the table of the unconstrained scheme's round A (the windowed layers' standard heads are its levels below s)
template <typename TC>
static void ra_build_std(cp_csr_s *A, LayerWork<TC> &Wk)
{
    const int64_t n = A->n;
    ra_build<TC>(A, Wk, Wk.ra, Wk.nbits, [n](int b) { return ((n >> b) + 1) >> 1; }, 0, nullptr, nullptr);
}
// ... and of the mirrored heads of the current window: rows (u + 1) 2^(b+1) <= n
template <typename TC>
static void ra_build_mir(cp_csr_s *A, LayerWork<TC> &Wk)
{
    const int64_t n = A->n;
    ra_build<TC>(A, Wk, Wk.mir, Wk.G.s, [n](int b) { return n >> (b + 1); }, Wk.G.w, Wk.win.w_anch.p, Wk.win.w_anch2.p);
}

// the nets (pass 0) / self nets (pass 1) a window of width x cuts, per column into w_hist and as prefix sums into w_E
template <typename TC>
static void win_hist_scan(cp_csr_s *A, LayerWork<TC> &Wk, int64_t x, int pass)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    if (pass == 1 || A->N == 0) CP_HIP(hipMemsetAsync(Wk.win.w_hist.p, 0, sizeof(int32_t) * (size_t)(n + 1), s));
    if (pass == 0) { if (A->N > 0) hipLaunchKernelGGL(k_win_hist, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, s, n, x, A->pos32.p, A->prev.p, A->next.p, Wk.win.w_hist.p); }
    else if (A->m > 0) hipLaunchKernelGGL(k_win_hist_rows, dim3((unsigned)cdiv(A->m, 256)), dim3(256), 0, s, A->m, n, x, A->rfirst.p, A->rlast.p, Wk.win.w_hist.p);
    exclusive_scan_i32(Wk.win.w_hist.p, Wk.win.w_E.p, n + 1, Wk.sc.scratch, s);
}

// anchors of the mirrored head tasks of the windowed layers (k_win_*): once per (pattern, w)
template <typename TC>
static void win_build(cp_csr_s *A, LayerWork<TC> &Wk)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n, w = Wk.G.w;
    const int sb = Wk.G.s;
    int64_t acc = 0;
    for (int b = 0; b < 33; b++) { Wk.win.aoff[b] = acc; if (b < sb) acc += (n >> (b + 1)) + 1; }      // heads of plane b: rho = idx << (b+1), idx <= n >> (b+1)
    Wk.win.nitems = acc;
    const size_t ni = (size_t)(acc > 0 ? acc : 1);
    Wk.win.w_anch.ensure(ni); Wk.win.w_tot.ensure(ni); Wk.win.w_hist.ensure((size_t)n + 2); Wk.win.w_E.ensure((size_t)n + 2);
    if (Wk.hyp) Wk.win.w_anch2.ensure(ni);
    Wk.win.built = false;
    if (acc > 0) {
        RoundDesc R;
        make_round(R, true, 0, sb + 1, n, 0, n, Wk.G, Wk.win.aoff);
        const unsigned wg = (unsigned)std::min<int64_t>(cdiv(acc, 4), 65536);
        for (int pass = 0; pass < (Wk.hyp ? 2 : 1); pass++) {
            win_hist_scan<TC>(A, Wk, w, pass);
            if (pass == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_win_block_totals<true>), dim3(wg), dim3(256), 0, s, R, acc, A->pos32.p, A->next.p, Wk.win.w_tot.p);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_win_block_totals<false>), dim3(wg), dim3(256), 0, s, R, acc, A->fpos32.p, A->flast.p, Wk.win.w_tot.p);
            hipLaunchKernelGGL(k_win_anchors, dim3((unsigned)cdiv(acc, 256)), dim3(256), 0, s, R, acc, pass == 0 ? A->pos.p : A->lpos.p, Wk.win.w_E.p, Wk.win.w_tot.p,
                               pass == 0 ? Wk.win.w_anch.p : Wk.win.w_anch2.p);
        }
        CP_HIP(hipGetLastError());
    }
    // leaf pass (dp_total_leaf.hip): anchors of the inner mirrored blocks, nets(64 g + 62 - w, 64 g) for every group g -- the same
    // histogram with the width w - 62
    Wk.win.leaf_anch.release(); Wk.win.leaf_anch2.release();
    if (sb >= LEAF_T && w > 62) {
        const int64_t ng = (n >> LEAF_T) + 1;
        Wk.win.leaf_anch.alloc((size_t)ng);
        if (Wk.hyp) Wk.win.leaf_anch2.alloc((size_t)ng);
        for (int pass = 0; pass < (Wk.hyp ? 2 : 1); pass++) {
            win_hist_scan<TC>(A, Wk, w - 62, pass);
            hipLaunchKernelGGL(k_leaf_anchors, dim3((unsigned)cdiv(ng, 256)), dim3(256), 0, s, ng, n, pass == 0 ? A->pos.p : A->lpos.p, Wk.win.w_E.p,
                               pass == 0 ? Wk.win.leaf_anch.p : Wk.win.leaf_anch2.p);
        }
        CP_HIP(hipGetLastError());
    }
    Wk.win.built = true; Wk.win.w = w;
}

constexpr int64_t LB_MAX = 1 << 20;      // largest scan (elements) done in a single launch

// Round A from a cache with the table T (the cache's own, or a copy cut to the levels and tiles a windowed layer needs): the
// column-major kernel over the candidate tiles [tile0, tile1) (`mirrored`: the table of the mirrored heads) or the row-major one
// over the cache's tiles, then the rows of more than LT candidates (nrow_merge of them) merge their partials.
template <typename TC, bool HYP>
static void launch_round_a(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RaCache<TC> &Ra, const RATab &T, int64_t nrow_merge, int64_t tile0, int64_t tile1,
                           int bmin, bool mirrored, bool colmajor)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    int32_t *nl = if_hyp<HYP>(Wk.pl.nlopt.p);
    if (colmajor)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mirrored ? k_ra_cols<TC, HYP, true> : k_ra_cols<TC, HYP, false>), dim3((unsigned)std::max<int64_t>(1, cdiv(tile1 - tile0, 4))), dim3(256), 0, s,
                           T, Ra.c.p, if_hyp<HYP>(Ra.c2.p), A->pos32.p, C.W, C.M, C.alpha, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, recs<HYP>(Ra.part), tile0, tile1, bmin);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ra_layer<TC, HYP>), dim3((unsigned)cdiv(Ra.ntile, 4)), dim3(256), 0, s, T, Ra.ntile, Ra.c.p, if_hyp<HYP>(Ra.c2.p), A->pos32.p, C.W, C.M,
                           C.alpha, Wk.pl.opt.p, Wk.pl.nnopt.p, nl, recs<HYP>(Ra.part));
    if (nrow_merge > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ra_merge<TC, HYP>), dim3((unsigned)cdiv(nrow_merge, 4)), dim3(256), 0, s, T, nrow_merge, recs<HYP>(Ra.part), Wk.pl.opt.p,
                           Wk.pl.nnopt.p, nl);
    CP_HIP(hipGetLastError());
}

// A full layer: round A of the rows' lowest blocks from the cached counts; what is left of round A for the generic round is the
// last row in its upper planes
template <typename TC, bool HYP>
static void round_a_full(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    if (!Wk.ra.built) { ProfScope ps(PROF_LINKS, s, 0.0); ra_build_std<TC>(C.A, Wk); }
    ProfScope ps(PROF_RA, s, 16.0 * (double)Wk.ra.ntile * LT);
    launch_round_a<TC, HYP>(C, Wk, Wk.ra, Wk.ra.tab, Wk.ra.nrow, 0, cdiv(C.n, LT), C.ra_bmin, false, !(g_opt_dbg & DBG_RA_ROWMAJOR));
}

// Windowed layer: the STANDARD heads of round A (rows with ctz == b < s, block [r - 2^b, r)) are the unconstrained scheme's
// round-A rows of the levels below s -- same blocks, same layer-independent counts: k_ra_cols computes them for all rows
// from the cache (60 B per candidate) and the generic round keeps the mirrored and common heads only.  The heads the layer
// reads are those make_round lists -- within 2^(b+1) of the row tile in plane b <= s: their blocks start at rlo - 3 * 2^s or later.
// `scope`: the stage's profile scope, opened here behind the table build and closed by the caller (the mirrored heads have always
// been enqueued inside it).
template <typename TC, bool HYP>
static void round_a_win_std(const LayerCtx<TC> &C, LayerWork<TC> &Wk, std::optional<ProfScope> &scope)
{
    hipStream_t s = C.s;
    const Geo &G = C.G;
    const int64_t n = C.n, rlo = C.rlo, rhi = C.rhi;
    if (!Wk.ra.built) { ProfScope ps(PROF_LINKS, s, 0.0); ra_build_std<TC>(C.A, Wk); }
    RATab T2 = Wk.ra.tab;
    T2.nbits = std::min<int32_t>(G.s, Wk.ra.tab.nbits);
    const int64_t nrow2 = T2.nbits > 9 ? Wk.ra.tab.rbase[T2.nbits] : 0;
    const int64_t c_lo = std::max<int64_t>(0, (rlo > 0 ? rlo : 0) - ((int64_t)4 << G.s)), c_hi = std::min<int64_t>(n, rhi);
    const int64_t tile0 = c_lo / LT, tile1 = cdiv(c_hi, LT);
    scope.emplace(PROF_RA, s, 60.0 * (double)(tile1 - tile0) * LT);
    // (the standard heads below LEAF_T are rows inside a leaf group: the leaf pass computes them; the MIRRORED heads of those
    //  levels include the multiples of 64 -- every row has a task in every plane -- and stay)
    launch_round_a<TC, HYP>(C, Wk, Wk.ra, T2, nrow2, tile0, tile1, C.ra_bmin, false, true);
}

// Windowed layer: the MIRRORED heads of round A the same way, from their own table (per level the tiles of the rows near the
// window); false: the table is empty, the heads stay generic tasks
template <typename TC, bool HYP>
static bool round_a_win_mir(const LayerCtx<TC> &C, LayerWork<TC> &Wk)
{
    hipStream_t s = C.s;
    const Geo &G = C.G;
    const int64_t n = C.n, rlo = C.rlo, rhi = C.rhi;
    if (!Wk.mir.built || Wk.mir.w != G.w) { ProfScope ps2(PROF_LINKS, s, 0.0); ra_build_mir<TC>(C.A, Wk); }
    if (Wk.mir.ntile <= 0) return false;
    RATab T3 = Wk.mir.tab;
    const int64_t r_lo = std::max<int64_t>(1, (rlo > 0 ? rlo : 0) - ((int64_t)4 << G.s)), r_hi = std::min<int64_t>(n, rhi);
    double elems = 0;
    for (int b = 0; b < T3.nbits; b++) {
        const int64_t u_lo = std::max<int64_t>(0, (r_lo >> (b + 1)) - 1), u_hi = r_hi >> (b + 1);        // rows u_lo .. u_hi - 1
        T3.tlo[b] = T3.tbase[b] + ((u_lo << b) / LT);
        T3.thi[b] = std::min<int64_t>(T3.tbase[b + 1], T3.tbase[b] + cdiv(std::max<int64_t>(u_hi, 0) << b, LT));
        elems += (double)std::max<int64_t>(0, T3.thi[b] - T3.tlo[b]) * LT;
    }
    // column-major like the standard heads (z = p + w + 1: the blocks of the rows r_lo .. r_hi lie in [r_lo, r_hi + 2^s)); the
    // row-major kernel reads 16 B per (candidate, level) instead of 4
    const bool mcols = !(g_opt_dbg & DBG_MIR_ROWMAJOR);
    const int64_t zt0 = r_lo / LT, zt1 = cdiv(std::min<int64_t>(n + G.w + 1, r_hi + ((int64_t)1 << G.s) + 1), LT);
    ProfScope ps2(PROF_RA, s, mcols ? 80.0 * (double)(zt1 - zt0) * LT : 16.0 * elems);
    launch_round_a<TC, HYP>(C, Wk, Wk.mir, T3, Wk.mir.nrow, zt0, zt1, 0, true, mcols);
    return true;
}

// cp_set_option("dbg", DBG_POISON [+ DBG_POISON_ZERO]): fills buffers a stage must write before it reads (null: not of this variant)
static void poison_fill(hipStream_t s, std::initializer_list<std::pair<void *, size_t>> bufs)
{
    if (!(g_opt_dbg & DBG_POISON)) return;
    const int pat = (g_opt_dbg & DBG_POISON_ZERO) ? 0x00 : 0x7F;
    for (const auto &b : bufs) if (b.first) CP_HIP(hipMemsetAsync(b.first, pat, b.second, s));
}

// ------------------------------------------------------------------ the stages of a round, each as the host function run_layer calls
// A stage function takes the layer's context, the work object, the round and its counts.
// the capacities a round's verdict checks its totals against: the buffers sized from the prediction (exact counts: no limit)
template <typename TC>
static void round_caps(const LayerCtx<TC> &C, const LayerWork<TC> &Wk, int64_t &capT, int64_t &capNT)
{
    const bool tiny = C.spec && (g_opt_dbg & DBG_TINY_BUFFERS);       // test: pretend the buffers sized from the prediction are too small
    capT = C.spec ? (tiny ? (int64_t)64 : (int64_t)Wk.fl.loc.n) : INT64_MAX;
    capNT = C.spec ? (tiny ? (int64_t)1 : (int64_t)Wk.ow.o_rec.n) : INT64_MAX;
}

// Set-up of a round: one lane per task finishes the short ones and lists the others.  ralloc (round_alloc): the launch also writes
// the lists' offsets and ends with the round's verdict -- the buffers the verdict checks against are sized before it
template <typename TC, bool HYP>
static void setup_tasks(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, int32_t own_min, bool cr_zero,
                        bool ralloc, bool want_items)
{
    int64_t capT, capNT;
    round_caps(C, Wk, capT, capNT);
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    // per task: four gathers from the plane arrays + the record; short tasks also step over their columns here
    ProfScope ps(PROF_SETUP, s, 29.0 * (double)R.ntask);
    const int sbs = (int)g_opt_setup_bs;          // lanes per block: one list atomic per block, but the block's waves meet at two barriers
    dim3 sgrid((unsigned)cdiv(R.ntask, sbs));
    if (!R.isA) {                                // one grid row per bit plane above tau
        int64_t mx = 1;
        for (int bb = R.tau + 1; bb < C.nbits; bb++) mx = std::max<int64_t>(mx, R.tbase[bb + 1] - R.tbase[bb]);
        sgrid = dim3((unsigned)cdiv(mx, sbs), (unsigned)std::max(1, C.nbits - R.tau - 1));
    }
    // (nlopt, crl, tS0l, o_tS0l and w_anch2 are read by the hyperedge variant only; null or stale for the other)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_setup_short<TC, HYP>), sgrid, dim3(sbs), 0, s, R, Wk.pl.opt.p, Wk.pl.nnopt.p, Wk.pl.nlopt.p, Wk.pl.cr.p, Wk.pl.crl.p, A->pos32.p,
                       A->next.p, if_hyp<HYP>(A->fpos32.p), if_hyp<HYP>(A->flast.p), C.W, C.M, C.alpha, Wk.tk.tdesc.p, Wk.tk.tb.p, Wk.tk.len.p, Wk.tk.tS0l.p, &rc->nlong,
                       (int32_t)g_opt_short_t, (int32_t)g_opt_short_e, C.own_tiles ? Wk.ow.o_tdesc.p : (int4 *)nullptr, Wk.ow.o_tb.p, Wk.ow.o_rlen.p, Wk.ow.o_ntl.p,
                       Wk.ow.o_tS0l.p, &rc->nown, &rc->own_steps, own_min,
                       (int32_t)std::min<size_t>(Wk.ow.o_ntl.n, (size_t)INT32_MAX), &rc->err, Wk.pl.fin.p, Wk.pl.last_s0.p,
                       (g_opt_dbg & DBG_COUNT_NONTRIVIAL) ? &rc->_pad : (int32_t *)nullptr, Wk.win.w_anch.p, Wk.win.w_anch2.p, C.pzp, C.oblk, cr_zero ? 1 : 0,
                       ralloc ? rc : (RoundCounts *)nullptr, Wk.tk.offs.p, Wk.ow.o_toffs.p, Wk.ow.o_ioffs.p, capT, capNT, want_items ? 1 : 0);
}

// Both scans of a round read their element count on the device; one launch holds them and the round's verdict
template <typename TC>
static void round_scans(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc)
{
    hipStream_t s = C.s;
    ProfScope ps(PROF_SCAN, s, 12.0 * (double)R.ntask);
    int64_t capT, capNT;
    round_caps(C, Wk, capT, capNT);
    const int64_t nm = std::min<int64_t>(R.ntask, (int64_t)Wk.ow.o_ntl.n);
    if (R.ntask <= LB_MAX) {
        launch_round_scans(rc, Wk.tk.len.p, Wk.tk.offs.p, R.ntask, Wk.ow.o_ntl.p, Wk.ow.o_toffs.p, nm, C.own_tiles, capT, capNT, Wk.sc.scanws, s);
    } else {
        // (single-launch scans take their block index from one counter: fine for a few hundred blocks, not for 27 000)
        exclusive_scan_i32_devn(Wk.tk.len.p, Wk.tk.offs.p, &rc->nlong, R.ntask, &rc->T, Wk.sc.scratch, s);
        if (C.own_tiles) exclusive_scan_i32_devn(Wk.ow.o_ntl.p, Wk.ow.o_toffs.p, &rc->nown, nm, &rc->NT, Wk.sc.scratch, s);
        hipLaunchKernelGGL(k_round_finish, dim3(1), dim3(1), 0, s, rc, capT, capNT);
    }
}

// ------------------------------------------------------------------ host side: the own-tile chain of a round
// Map and stream + evaluate.  split (run_layer): 0: whole columns; 1: every tile of the launch is of a plane >= SPLIT_BMIN, their
// number is NT; 2: the launch also holds tiles of the planes below -- the gap round tau = 6 with its plane-7 tiles, and every
// round below it with gap_tau < 6 -- and k_own_map counts: 1 600 same-address atomics per launch cost it 17 us at config 3.
// (windowed layers keep one tile per wave: their tiles stream whole columns, ten trips and more, and paired they ran 5 % slower)
template <bool HYP> static bool own_pairs(bool gap, bool win) { return !HYP && !gap && !win && g_opt_own_pair != 0; }

// cp_set_option("own_pack", 0 | 1): the split tiles of a launch take the packed words where the geometry keeps a tile inside one block
// (own_blk 1) and the pattern's offsets fit 16 bits -- except in a paired launch that also holds tiles of the planes below (gap_tau
// below 6): a wave's two tiles run one text.  Returns whether they did.
template <typename TC, bool HYP>
static bool own_stream(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P, bool gap, int split, bool ralloc)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    const int64_t n = C.n;
    const int oblk = C.oblk;
    const int64_t gNT = C.spec ? (int64_t)Wk.ow.o_rec.n : P.NT;      // (capacity >= the true NT, checked)
    poison_fill(s, {{Wk.ow.o_part.p, Wk.ow.o_part.bytes()}, {Wk.ow.o_tileS.p, Wk.ow.o_tileS.bytes()}, {Wk.ow.o_rec.p, Wk.ow.o_rec.bytes()}, {Wk.ow.o_srec.p, Wk.ow.o_srec.bytes()},
                    {if_hyp<HYP>(Wk.ow.o_tileS2.p), Wk.ow.o_tileS2.bytes()}, {Wk.ow.o_items.p, Wk.ow.o_items.bytes()}, {Wk.ow.o_item_of.p, Wk.ow.o_item_of.bytes()},
                    {Wk.ow.o_trec.p, Wk.ow.o_trec.bytes()}});
    const unsigned mgrid = (unsigned)std::min<int64_t>(cdiv(gNT, 256), 8192);
    if (split && !Wk.ow.split.built) {             // once per pattern, by the first round that streams them
        ProfScope ps(PROF_LINKS, s, 8.0 * (double)A->N + 16.0 * (double)(C.nbits - SPLIT_BMIN) * (double)(n + 1));
        split_build(A, Wk.ow.split, Wk.sc.scratch);
    }
    if (split) g_own_pack_wide = Wk.ow.split.packed ? 0 : 1;      // (of the pattern the last split launch ran on)
    const bool pair = own_pairs<HYP>(gap, C.G.win != 0);
    const bool pack = split && oblk && g_opt_own_pack && Wk.ow.split.packed && !(pair && split == 2);
    if (split && !pack) split_wide(A, Wk.ow.split);
    hipLaunchKernelGGL(k_own_map, dim3(mgrid), dim3(256), 0, s, rc, Wk.ow.o_toffs.p, Wk.ow.o_tdesc.p, Wk.ow.o_rlen.p, Wk.ow.o_rec.p, Wk.ow.o_task.p,
                       Wk.ow.o_tb.p, gap ? Wk.ow.o_hi.p : (int32_t *)nullptr, R.tau, n, oblk, oblk ? Wk.ow.b_cnt.p : (int32_t *)nullptr, Wk.ow.o_brank.p,
                       gap ? (int2 *)nullptr : Wk.ow.o_items.p, Wk.ow.o_item_of.p, split, ralloc ? Wk.ow.o_ioffs.p : (const int32_t *)nullptr);
    ProfScope ps(gap ? PROF_GAPSTREAM : PROF_OWN, s, C.own_bytes(Wk.ow.split, R.tau, pack ? 2 : split != 0, (double)P.own_steps));
    if (oblk) {                       // the tile ids by column block (counted in k_own_map): ~10^5 tiles, a counting sort
        exclusive_scan_i32_lb(Wk.ow.b_cnt.p, Wk.ow.b_start.p, Wk.ow.b_n.p, Wk.ow.b_nblk, nullptr, Wk.sc.scanws, s);
        hipLaunchKernelGGL(k_blk_order, dim3(mgrid), dim3(256), 0, s, rc, Wk.ow.o_rec.p, Wk.ow.o_brank.p, Wk.ow.b_start.p, Wk.ow.o_border.p, Wk.ow.o_srec.p, Wk.ow.b_cnt.p);
    }
    // cp_set_option("own_pair", 0 | 1): outside the gap rounds and the hyperedge costs a wave takes two slots of the run order
    // (the packed instantiations exist for the plain costs only: `pack` is never set for the hyperedge ones)
    auto kern = gap ? (pack ? k_lpass_own<TC, HYP, true, false, !HYP> : k_lpass_own<TC, HYP, true>)
              : pair ? (pack ? k_lpass_own<TC, HYP, false, !HYP, !HYP> : k_lpass_own<TC, HYP, false, !HYP>)
              : (pack ? k_lpass_own<TC, HYP, false, false, !HYP> : k_lpass_own<TC, HYP, false>);
    hipLaunchKernelGGL(kern,
                       dim3((unsigned)cdiv(pair ? cdiv(gNT, 2) : gNT, 4)), dim3(256), 0, s, R.isA, rc,
                       oblk ? Wk.ow.o_border.p : (const int32_t *)nullptr, A->pos32.p, A->next.p, if_hyp<HYP>(A->fpos32.p), if_hyp<HYP>(A->flast.p),
                       Wk.ow.o_tileS.p, Wk.ow.o_tileS2.p, Wk.ow.o_rec.p, Wk.ow.o_srec.p, C.W, C.M, C.alpha, recs<HYP>(Wk.ow.o_part), R.tau, Wk.ow.o_hi.p, Wk.ow.o_spec.p,
                       (int)((g_opt_dbg & DBG_GAP_ALL_SPECIAL) != 0), recs<HYP>(Wk.ow.o_sub), Wk.ow.o_spv.p, A->col.p, if_hyp<HYP>(A->ffirst.p),
                       split ? Wk.ow.split.vnext.p : (const int32_t *)nullptr, pack ? Wk.ow.split.vpk.p : Wk.ow.split.vpos.p,
                       pack ? reinterpret_cast<const int32_t *>(Wk.ow.split.vbase.p) : Wk.ow.split.vsa.p, (int64_t)(n + 1));
    return pack;
}

// The tail of the chain outside the gap rounds: one launch, a lane per task of up to FIX_SERIAL tiles, a block per listed trip
// of the longer ones
template <typename TC, bool HYP>
static void own_merge(const LayerCtx<TC> &C, LayerWork<TC> &Wk, RoundCounts *rc, const RoundCounts &P, bool ralloc)
{
    ProfScope ps(PROF_FIX, C.s, 24.0 * (double)P.NT);
    launch_fix_own<TC, HYP>(C.s, rc, Wk.ow.o_toffs.p, recs<HYP>(Wk.ow.o_part), Wk.ow.o_tdesc.p, Wk.ow.o_tb.p, if_hyp<HYP>(Wk.ow.o_tS0l.p), Wk.ow.o_tileS.p,
                            if_hyp<HYP>(Wk.ow.o_tileS2.p), C.M, Wk.pl.opt.p, Wk.pl.nnopt.p, if_hyp<HYP>(Wk.pl.nlopt.p), C.n, Wk.ow.o_items.p, Wk.ow.o_item_of.p, Wk.ow.o_trec.p,
                            Wk.ow.o_tick.p, C.spec ? grow_pred(P.NT) : P.NT, C.spec ? grow_pred(P.nown) : P.nown,
                            ralloc ? Wk.ow.o_ioffs.p : (const int32_t *)nullptr);
}

// ------------------------------------------------------------------ host side: the flattened chain of a round (the tasks' number: rc->nlong)
// the grid's tile count: the buffers' capacity in a speculative layer (>= the true tile count, checked by the round's verdict)
template <typename TC>
static int64_t flat_gtile(const LayerCtx<TC> &C, const LayerWork<TC> &Wk, const RoundCounts &P) { return C.spec ? (int64_t)Wk.fl.tileS.n : cdiv(P.T, LT); }

// tile table and stream
template <typename TC, bool HYP>
static void flat_stream(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    const int64_t gtile = flat_gtile(C, Wk, P);
    poison_fill(s, {{Wk.fl.loc.p, Wk.fl.loc.bytes()}, {if_hyp<HYP>(Wk.fl.loc2.p), Wk.fl.loc2.bytes()}, {Wk.fl.partL.p, Wk.fl.partL.bytes()}, {Wk.fl.partR.p, Wk.fl.partR.bytes()},
                    {Wk.fl.tileS.p, Wk.fl.tileS.bytes()}, {if_hyp<HYP>(Wk.fl.tileS2.p), Wk.fl.tileS2.bytes()}});
    hipLaunchKernelGGL(k_tile_t0, dim3((unsigned)cdiv(gtile, 256)), dim3(256), 0, s, rc, Wk.tk.offs.p, Wk.tk.tdesc.p, Wk.fl.tile_t0.p,
                       Wk.fl.tile_rec.p, (int)((g_opt_dbg & DBG_NO_INTERIOR) != 0), Wk.fl.taskR.p);
    // algorithmic bytes of one launch: per flattened step the stepped column's link
    // entries (4 B x N/n, plus 4 B x nonempty-rows/n for hyperedge costs), its colptr entry (8 B), the
    // candidate's previous-layer cost (8 B) and the task-descriptor share (offsets/B/anchor/row, amortised 8 B)
    ProfScope ps(PROF_EXPAND, s, (double)P.T * C.step_bytes);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lpass<TC, HYP>), dim3((unsigned)cdiv(gtile, 4)), dim3(256), 0, s, R, rc, Wk.tk.offs.p, Wk.tk.tdesc.p, Wk.tk.tS0l.p, Wk.tk.tb.p,
                       A->pos32.p, A->next.p, if_hyp<HYP>(A->fpos32.p), if_hyp<HYP>(A->flast.p), Wk.pl.opt.p, Wk.pl.nnopt.p, Wk.pl.nlopt.p, Wk.fl.loc.p, Wk.fl.loc2.p,
                       Wk.fl.tileS.p, Wk.fl.tileS2.p, Wk.fl.taskR.p, Wk.fl.tile_t0.p, Wk.fl.tile_rec.p, C.W, C.M, C.alpha, recs<HYP>(Wk.fl.partR), recs<HYP>(Wk.fl.partL));
}

// the tiles' carry, the tasks that span tiles, the merge
template <typename TC, bool HYP>
static void flat_finish(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P)
{
    hipStream_t s = C.s;
    cp_csr_s *A = C.A;
    const int64_t gtile = flat_gtile(C, Wk, P);
    {
        ProfScope ps(PROF_CARRY, s, 12.0 * (double)cdiv(P.T, LT));
        exclusive_scan_i32_lb(Wk.fl.tileS.p, Wk.fl.tilePS.p, &rc->ntile, (int64_t)Wk.fl.tileS.n, nullptr, Wk.sc.scanws, s);
        if (HYP) exclusive_scan_i32_lb(Wk.fl.tileS2.p, Wk.fl.tilePS2.p, &rc->ntile, (int64_t)Wk.fl.tileS.n, nullptr, Wk.sc.scanws, s);
    }
    unsigned wgrid = (unsigned)std::min<int64_t>(cdiv(gtile, 4), 8192);     // the wave kernels walk work lists
    {
        ProfScope ps(PROF_EVAL, s, 0.0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_span_short<TC, HYP>), dim3((unsigned)cdiv(gtile, 256)), dim3(256), 0, s, R, rc, Wk.tk.offs.p, Wk.tk.tdesc.p, Wk.tk.tS0l.p,
                           Wk.tk.tb.p, A->pos32.p, Wk.fl.loc.p, Wk.fl.loc2.p, Wk.fl.tile_t0.p, Wk.fl.taskR.p, Wk.fl.tileS.p, Wk.fl.tileS2.p, recs<HYP>(Wk.fl.partR), C.W, C.M, C.alpha,
                           Wk.pl.opt.p, Wk.pl.nnopt.p, if_hyp<HYP>(Wk.pl.nlopt.p), Wk.fl.open_list.p, Wk.fl.fix_list.p, Wk.fl.tile_rec.p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_open<TC, HYP>), dim3(wgrid), dim3(256), 0, s, R, rc, Wk.tk.offs.p, Wk.tk.tdesc.p, Wk.tk.tS0l.p, A->pos32.p, Wk.fl.loc.p,
                           Wk.fl.loc2.p, Wk.fl.tile_t0.p, Wk.fl.tilePS.p, if_hyp<HYP>(Wk.fl.tilePS2.p), C.W, C.M, C.alpha, recs<HYP>(Wk.fl.partL), Wk.fl.open_list.p);
    }
    {
        ProfScope ps(PROF_FIX, s, 8.0 * (double)cdiv(P.T, LT));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fix<TC, HYP>), dim3(wgrid), dim3(256), 0, s, rc, Wk.tk.offs.p, Wk.fl.taskR.p, recs<HYP>(Wk.fl.partL), recs<HYP>(Wk.fl.partR),
                           Wk.tk.tdesc.p, Wk.tk.tb.p, Wk.pl.opt.p, Wk.pl.nnopt.p, if_hyp<HYP>(Wk.pl.nlopt.p), C.n + 1, Wk.fl.fix_list.p, Wk.fl.tile_rec.p, Wk.fl.tilePS.p,
                           if_hyp<HYP>(Wk.fl.tilePS2.p), if_hyp<HYP>(Wk.tk.tS0l.p), C.M);
    }
    CP_HIP(hipGetLastError());
}

// Begins a layer ON THE STREAM and returns what it fixes once.  Enqueued here, in this order: the clear of the round counters, of
// the block counts and the tickets where they may be dirty, the poison fills (poison mode), and the clear of the `fin` plane when
// the layer's new stamp wraps; on the host the layer takes its `fin` stamp and `planes_full` is set.
template <typename TC, bool HYP>
static LayerCtx<TC> begin_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, LayerWork<TC> &Wk,
                                int64_t rlo, int64_t rhi, bool spec)
{
    hipStream_t s = A->stream;
    const int64_t n = A->n;
    const Geo G = Wk.G;
    const int nbits = G.win ? G.s + 1 : Wk.nbits;          // windowed layers: planes 0 .. s
    const double avg_deg = n > 0 ? (double)A->N / (double)n : 0.0;
    const double self_deg = (HYP && n > 0) ? (double)A->nrows_nonempty / (double)n : 0.0;
    // bytes a step of the streaming kernels moves: the stepped column's link entries (4 B each; hyperedge costs: plus the rows starting
    // in it), its 32-bit column pointer (4 B), the candidate's previous-layer cost (8 B), and the tile's record + partial
    // (16 B + 16 B per 256 steps).  (Round 1 priced a step at 4 deg + 24 B -- 8-byte column pointers and a per-step descriptor share
    // the kernels do not read -- which put the achieved rate above the box's copy rate.)
    const double step_bytes = 4.0 * (avg_deg + self_deg) + 12.0 + 32.0 / (double)LT;
    const bool own_tiles = !(g_opt_dbg & DBG_NO_OWN_TILES);      // (keep every long task in the flattened space)
    // cp_set_option("own_split", 0 | 1): outside round A the own tiles of the planes >= SPLIT_BMIN stream only their plane's variable
    // link entries (SplitLinks); the tiles of the gap rounds while "gap_split" is on too.  Not for hyperedge costs (the second list is not split) nor for windowed layers
    // (their blocks are not the Fenwick blocks).
    const bool split_layer = !HYP && !G.win && g_opt_own_split && nbits > SPLIT_BMIN;
    CP_HIP(hipMemsetAsync(Wk.sp.rc.p, 0, sizeof(RoundCounts) * (size_t)(nbits + 1), s));
    const bool gaps = own_tiles && g_opt_gap_tau >= 0;
    // cp_set_option("own_blk", 0 | 1): the tile geometry of the own-tiled tasks (see k_own_map).  Fixed for the whole layer: the
    // tile counts of setup depend on it.
    const int oblk = g_opt_own_blk ? 1 : 0;
    if (oblk) {
        const int64_t nblk = n / LT + 1;                 // the blocks of the columns 0 .. n
        if (Wk.ow.b_nblk != nblk || !Wk.ow.b_cnt.p) {
            Wk.ow.b_cnt.ensure((size_t)nblk); Wk.ow.b_start.ensure((size_t)nblk + 1); Wk.ow.b_n.ensure(1);
            CP_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(Wk.ow.b_n.p), (int)nblk, 1, s));
            Wk.ow.b_nblk = nblk;
            Wk.ow.b_dirty = true;
        }
        // b_cnt is zero between rounds (k_blk_order puts back what k_own_map counted): cleared when allocated.  The clear after a
        // layer that did not come to its end in order is a safeguard only: k_own_map and k_blk_order are enqueued as a pair and
        // walk the same tiles (a dropped round: none), so only an error thrown between the two could leave counts behind.
        if (Wk.ow.b_dirty) CP_HIP(hipMemsetAsync(Wk.ow.b_cnt.p, 0, Wk.ow.b_cnt.bytes(), s));
        Wk.ow.b_dirty = true;
    }
    // o_tick is zero between rounds the same way (the block that folds a task puts its ticket back): cleared when allocated and,
    // as a safeguard only, after a layer that did not come to its end in order
    if (Wk.ow.t_dirty) CP_HIP(hipMemsetAsync(Wk.ow.o_tick.p, 0, Wk.ow.o_tick.bytes(), s));
    Wk.ow.t_dirty = true;
    // cp_set_option("poison", 1) (tests): every layer starts from planes full of an out-of-range column; the kernels that turn
    // plane cells into addresses count and clamp what they read of it.  The invariant behind the speculative layers -- "whatever a
    // layer that is NOT redone has read was written by that layer" -- then reads: hits > 0 implies the layer is flagged for a redo.
    int32_t *pzp = nullptr;
    if (g_opt_poison) {
        Wk.pl.pz.ensure(2);
        pzp = Wk.pl.pz.p;
        CP_HIP(hipMemsetAsync(Wk.pl.pz.p, 0, sizeof(int32_t) * 2, s));
        CP_HIP(hipMemsetAsync(Wk.pl.opt.p, 0x7F, Wk.pl.opt.bytes(), s));
        CP_HIP(hipMemsetAsync(Wk.pl.nnopt.p, 0x7F, Wk.pl.nnopt.bytes(), s));
        if (HYP) CP_HIP(hipMemsetAsync(Wk.pl.nlopt.p, 0x7F, Wk.pl.nlopt.bytes(), s));
    }
    // the rounds tau < LEAF_T are one pass over groups of 64 rows (dp_total_leaf.hip); windowed layers: when the window spans a group
    // (s >= 6) and no per-block table is asked for
    const bool leaf = g_opt_leaf && (!G.win || (G.s >= LEAF_T && !g_opt_block_tables && Wk.win.leaf_anch.p));
    Wk.pl.planes_full = !leaf || g_opt_block_tables;
    // round A from the cached counts leaves the levels below LEAF_T to the leaf pass (DBG_RA_ALL_LEVELS: all levels, as without it)
    const int ra_bmin = (leaf && !Wk.pl.planes_full && !(g_opt_dbg & DBG_RA_ALL_LEVELS)) ? LEAF_T : 0;
    // `fin` flags hold the layer's stamp: no 240 MB clear per layer (every attempt of a layer -- a redo included -- takes a new stamp)
    if (++Wk.pl.fin_stamp > 255 || Wk.pl.fin_stamp <= 0) { CP_HIP(hipMemsetAsync(Wk.pl.fin.p, 0, Wk.pl.fin.bytes(), s)); Wk.pl.fin_stamp = 1; }
    // cp_set_option("cr_consume", 0 | 1): in a full layer the cells of cr / crl that a round's right pass adds into are the cells the
    // round's tasks read, the same from layer to layer (make_round and launch_rpass with rlo <= 1, rhi >= n: the rows with ctz == tau,
    // in the planes whose bit they have set).  Set-up zeroes what it reads (cr_zero), and while the planes are known to be clean
    // -- since allocation, or since a full layer that cleared and zeroed under the same rpass_ch -- the clearing launch is left out
    // (cr_consume).  Windowed and row-tiled layers add into rows next to their tile that no task of theirs reads: they keep the
    // clear and leave the planes dirty, like a layer that threw.
    const bool full = !G.win && rlo <= 1 && rhi >= n;
    if (Wk.pl.cr_ch != g_opt_rpass_ch) Wk.pl.cr_dirty = true;
    const bool cr_zero = g_opt_cr_consume && full;
    const bool cr_consume = cr_zero && !Wk.pl.cr_dirty;
    Wk.pl.cr_dirty = true; Wk.pl.cr_ch = g_opt_rpass_ch;
    return LayerCtx<TC>{A, s, M, alpha, W, cst_out, ptr_out, n, rlo, rhi, G, nbits, spec, own_tiles, gaps, split_layer, leaf, oblk, ra_bmin, pzp,
                        avg_deg, self_deg, step_bytes, cr_zero, cr_consume};
}

// Runs the rounds of one layer.  `spec`: the per-round counts of the PREVIOUS layer (Wk.sp.pred) size the grids, the buffers and
// decide which stages are launched; every kernel reads its true loop bounds from the device (RoundCounts) and walks them with
// grid strides, so a wrong prediction costs time, never correctness -- except a stage skipped or a buffer too small, which
// run_layer reports (false) after the layer and the caller redoes the layer with spec = false: one host sync per round brings
// the exact counts back before the dependent launches (the only mode of the first layer).
// run_layer is the loop over the rounds: it decides which stage runs and with which counts; each stage is enqueued by the stage
// function above.
template <typename TC, bool HYP>
static bool run_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, LayerWork<TC> &Wk,
                      int64_t rlo, int64_t rhi, bool spec, bool allow_force)
{
    const LayerCtx<TC> C = begin_layer<TC, HYP>(A, M, alpha, W, cst_out, ptr_out, Wk, rlo, rhi, spec);
    hipStream_t s = C.s;
    const int64_t n = C.n;
    const Geo G = C.G;
    const int nbits = C.nbits;
    int32_t *pzp = C.pzp;
    const int NR = nbits + 1;
    std::vector<RoundCounts> used((size_t)NR);          // what the host sized each round with
    memset(used.data(), 0, sizeof(RoundCounts) * (size_t)NR);
    struct Patch { size_t idx; int rd; int kind; int tau; int split; };          // (split: 0 whole columns, 1 split, 2 packed -- own_bytes)
    std::vector<Patch> patches;                          // profile records whose algorithmic bytes depend on the true counts
    auto note = [&](int rd, int kind, int slot, int tau = 0, int sp = 0) {
        if (prof_active(slot)) patches.push_back({g_prof_pending.size() - 1, rd, kind, tau, sp});
    };
    bool any_forced = false;
    std::vector<int8_t> split_mode((size_t)NR, 0);       // own_split per round (see own_stream)
    std::vector<int8_t> pair_mode((size_t)NR, 0);        // own_pair per round
    std::vector<int8_t> pack_mode((size_t)NR, 0);        // own_pack per round

    for (int rd = 0; rd <= nbits; rd++) {
        RoundDesc R;
        if (rd == 0) make_round(R, true, 0, nbits, n, rlo, rhi, G, Wk.win.aoff);
        else make_round(R, false, nbits - rd, nbits, n, rlo, rhi, G, Wk.win.aoff);
        R.fin_stamp = Wk.pl.fin_stamp;
        if (C.leaf && !R.isA && R.tau < LEAF_T) continue;
        if (rd == 0 && g_opt_ra_cache && rlo <= 1 && rhi >= n && n >= 1 && !G.win) {
            // a full layer: round A of the rows' lowest blocks from the cached counts; what is left of round A below is the
            // last row in its upper planes
            round_a_full<TC, HYP>(C, Wk);
            R.a_nmain = 0; R.ntask = R.nextra + R.nlast;
        }
        if (rd == 0 && g_opt_ra_cache && G.win && G.s >= 1 && n >= 1 && !(g_opt_dbg & DBG_WIN_NO_RA_CACHE)) {
            // a windowed layer: the standard heads of round A from the cache, and the mirrored ones from theirs; the generic round
            // keeps the common heads (and the mirrored ones where their table is empty or switched off)
            std::optional<ProfScope> scope;       // of the standard heads: open until the mirrored ones are enqueued, as ever
            round_a_win_std<TC, HYP>(C, Wk, scope);
            R.skip_std = 1;
            if (!(g_opt_dbg & DBG_WIN_NO_MIR_CACHE) && round_a_win_mir<TC, HYP>(C, Wk)) R.skip_mir = 1;
        }
        if (R.ntask <= 0) continue;
        CP_REQUIRE(R.ntask <= Wk.max_tasks, CP_EINTERNAL, "a DP round has more tasks than the task buffers hold");
        RoundCounts *rc = Wk.sp.rc.p + rd;
        const bool gap = C.gaps && !R.isA && R.tau <= g_opt_gap_tau;       // long tasks of this round finish all the rows of their gap
        // In the rounds above the gap rounds the flattened stage (tile table, stream, two scans, span / open / fix: six dependent
        // launches, ~40 us) typically serves three or four medium tasks.  Where the last layer that ran it saw at most force_max (1024), every task
        // that is not finished in setup gets tiles of its own instead, and the stage disappears from the round.
        const bool forced = allow_force && C.own_tiles && !gap && !R.isA && (size_t)rd < Wk.sp.force_own.size() && Wk.sp.force_own[(size_t)rd] &&
                            (rhi - rlo + 1) <= 2 * Wk.sp.force_rows && !(g_opt_dbg & DBG_NO_FORCE_OWN);
        any_forced |= forced;
        if (!R.isA) right_pass<TC, HYP>(C, Wk, R);
        if (R.isA && R.nlast > 0) last_row_counts<TC, HYP>(C, Wk, R);
        // cp_set_option("cr_consume", 0 | 1): where the chunks of a row add into cr / crl, set-up leaves the cells it reads zero
        const bool cr_zero = C.cr_zero && !R.isA && ((int64_t)1 << R.tau) > g_opt_rpass_ch;
        RoundCounts P;                                   // the counts this round is sized with (before set-up: its last block gives the verdict under round_alloc)
        if (spec) {
            P = Wk.sp.pred[(size_t)rd];
            if (Wk.sp.pred_scale != 1.0) {              // (windowed layers: the previous layer's tile had another number of rows)
                auto sc = [&](int64_t v) { return (int64_t)((double)v * Wk.sp.pred_scale) + (v > 0 ? 1 : 0); };
                P.nlong = (int32_t)sc(P.nlong); P.nown = (int32_t)sc(P.nown); P.T = sc(P.T); P.NT = sc(P.NT);
                P.own_steps = (unsigned long long)sc((int64_t)P.own_steps);
            }
            if ((g_opt_dbg & DBG_MISPREDICT) && (rd & 1)) { P.nown = 0; P.NT = 0; P.nlong = 0; P.T = 0; }      // test: a prediction that skips stages with work
            // buffers from the prediction (grown only here; the round's verdict, k_round_scans, checks the true totals against them)
            Wk.ow.ensure_own(Wk.hyp, (size_t)grow_pred(P.NT));
            Wk.fl.ensure_flat(Wk.hyp, (size_t)grow_pred(P.T));
        }
        // cp_set_option("round_alloc", 0 | 1): set-up reserves the lists' offsets with their slots and ends with the verdict, where
        // the packed words are wide enough (round_alloc_fits) and a single launch may scan the lists at all; elsewhere k_round_scans
        const int64_t own_min64 = forced ? 2 : gap ? g_opt_gap_min : g_opt_own_min;
        const int32_t own_min = (int32_t)own_min64;
        const bool ralloc = g_opt_round_alloc && C.own_tiles && R.ntask <= LB_MAX && round_alloc_fits(R.ntask, n, own_min64);
        setup_tasks<TC, HYP>(C, Wk, R, rc, own_min, cr_zero, ralloc, !gap);
        if (ralloc) g_round_alloc_rounds++;
        else round_scans<TC>(C, Wk, R, rc);
        if (!spec) {
            CP_HIP(hipMemcpyAsync(&P, rc, sizeof(P), hipMemcpyDeviceToHost, s));
            CP_HIP(hipStreamSynchronize(s));
            Wk.ow.ensure_own(Wk.hyp, (size_t)P.NT);
            Wk.fl.ensure_flat(Wk.hyp, (size_t)P.T);
        }
        used[(size_t)rd] = P;
        if (g_opt_dbg & DBG_PRINT_ROUNDS) fprintf(stderr, "round isA=%d tau=%d ntask=%lld %s long=%d own=%d T=%lld NT=%lld nontrivial=%d\n", R.isA, R.tau, (long long)R.ntask,
                                   spec ? "predicted" : "exact", P.nlong, P.nown, (long long)P.T, (long long)P.NT, P._pad);
        if (P.nown > 0 && P.NT > 0) {
            // ---- long tasks with tiles of their own: map, stream + evaluate, then the gap passes or the merge
            // (gap rounds: cp_set_option("gap_split", 0 | 1), effective while own_split is on)
            const int split = !(C.split_layer && !R.isA && (!gap || g_opt_gap_split)) ? 0 : R.tau + 1 >= SPLIT_BMIN ? 1 : 2;
            split_mode[(size_t)rd] = (int8_t)(gap ? -split : split);
            pair_mode[(size_t)rd] = own_pairs<HYP>(gap, G.win != 0);
            const bool pack = own_stream<TC, HYP>(C, Wk, R, rc, P, gap, split, ralloc);
            pack_mode[(size_t)rd] = pack;
            note(rd, 0, gap ? PROF_GAPSTREAM : PROF_OWN, R.tau, pack ? 2 : split != 0);
            if (gap) gap_finish<TC, HYP>(C, Wk, R, rc, P);
            else own_merge<TC, HYP>(C, Wk, rc, P, ralloc);
            CP_HIP(hipGetLastError());
        }
        if (P.nlong <= 0 || P.T <= 0) continue;
        // ---- from here on the round consists of the flattened tasks only (their number: rc->nlong)
        flat_stream<TC, HYP>(C, Wk, R, rc, P);
        note(rd, 1, PROF_EXPAND);
        flat_finish<TC, HYP>(C, Wk, R, rc, P);
    }
    if (C.leaf) leaf_pass<TC, HYP>(C, Wk);
    combine_rows<TC, HYP>(C, Wk);
    CP_HIP(hipGetLastError());
    // ---- the true counts of every round: the next layer's prediction, this layer's verdict
    std::vector<RoundCounts> got((size_t)NR);
    int32_t pz_hits[2] = {0, 0};
    CP_HIP(hipMemcpyAsync(got.data(), Wk.sp.rc.p, sizeof(RoundCounts) * (size_t)NR, hipMemcpyDeviceToHost, s));
    if (pzp) CP_HIP(hipMemcpyAsync(pz_hits, pzp, sizeof(pz_hits), hipMemcpyDeviceToHost, s));
    CP_HIP(hipStreamSynchronize(s));
    bool ok = true;
    for (int rd = 0; rd < NR; rd++) {
        const RoundCounts &g = got[(size_t)rd], &u = used[(size_t)rd];
        CP_REQUIRE(!(g.err && !spec && !any_forced), CP_EINTERNAL, "DP work list overflow");
        if (g.err) ok = false;                                                                  // a buffer was too small (the caller runs the layer again, plainly)
        if (g.nown > 0 && g.NT > 0 && !(u.nown > 0 && u.NT > 0)) ok = false;                    // a stage was skipped
        if (g.nlong > 0 && g.T > 0 && !(u.nlong > 0 && u.T > 0)) ok = false;
    }
    if (pzp) {
        g_poison_hits += pz_hits[0];
        CP_REQUIRE(!(ok && pz_hits[0] > 0), CP_EINTERNAL, "a DP layer that is not redone read plane cells nobody wrote (poison mode)");
    }
    if (ok) Wk.ow.b_dirty = false;
    Wk.pl.cr_dirty = !C.cr_zero;                            // (every right pass that was enqueued was followed by its set-up, also in a layer that is redone)
    Wk.ow.t_dirty = false;                                  // (every merge that was enqueued has run to its end, also in a layer that is redone)
    if (ok) for (int rd = 0; rd < NR; rd++) { g_fix_trips += got[(size_t)rd].n_trips; g_fix_edges |= got[(size_t)rd].n_edge; }
    if (ok) for (int rd = 0; rd < NR; rd++) {
        const RoundCounts &g = got[(size_t)rd];
        if (g.nown > 0 && g.NT > 0) {                   // (negative: a gap round)
            const int sm = split_mode[(size_t)rd];
            const int64_t nsp = std::abs(sm) == 1 ? g.NT : std::abs(sm) == 2 ? g.n_split : 0;
            (sm < 0 ? g_gap_split_tiles : g_own_split_tiles) += nsp;
            if (pack_mode[(size_t)rd]) g_own_pack_tiles += nsp;                  // (the split tiles of a packed launch, gap rounds included)
            if (pair_mode[(size_t)rd]) { g_own_pair_waves += g.NT / 2; g_own_pair_lone += g.NT & 1; }      // (own_pair_slots over the true NT)
        }
    }
    // (attempts that are redone included: a dropped round lists none; round_alloc reserves a round's items in set-up, so a round
    //  whose own-tile stage the host skipped on a wrong prediction holds a count nobody listed: not counted, as before)
    for (int rd = 0; rd < NR; rd++) if (used[(size_t)rd].nown > 0 && used[(size_t)rd].NT > 0) g_fix_items += got[(size_t)rd].n_items;
    if (ok) {
        for (auto &pt : patches) {
            const RoundCounts &g = got[(size_t)pt.rd];
            if (pt.idx < g_prof_pending.size())
                g_prof_pending[pt.idx].bytes = pt.kind == 0 ? C.own_bytes(Wk.ow.split, pt.tau, pt.split, (double)g.own_steps) : (double)g.T * C.step_bytes;
        }
        Wk.sp.pred = got; Wk.sp.pred_ok = true; Wk.sp.pred_rlo = rlo; Wk.sp.pred_rhi = rhi; Wk.sp.pred_win = G.win; Wk.sp.pred_w = G.w;
        if (allow_force && 2 * (rhi - rlo + 1) >= Wk.sp.force_rows) {
            Wk.sp.force_own.resize((size_t)NR, 0);
            Wk.sp.force_rows = rhi - rlo + 1;
            for (int rd = 1; rd < NR; rd++) {
                const RoundCounts &g = got[(size_t)rd];
                if (g.nlong > 0) Wk.sp.force_own[(size_t)rd] = g.nlong <= g_opt_force_max;         // (a forced round reports none: its flag stays)
            }
        }
    }
    return ok;
}

template <typename TC>
void dp_total_layer(cp_csr_s *A, const DevModel<TC> &M, TC alpha, const TC *W, TC *cst_out, int32_t *ptr_out, void *work_,
                    int64_t rlo, int64_t rhi, int64_t wwin)
{
    auto &Wk = *reinterpret_cast<LayerWork<TC> *>(work_);
    int64_t n = A->n;
    bool hyp = M.kind == CP_MODEL_HYPEREDGE_CUT;
    int nbits = 1;
    while (((int64_t)1 << nbits) <= n) nbits++;
    CP_REQUIRE(nbits <= NBMAX, CP_EINVAL, "n exceeds the bit-plane budget");
    if (Wk.n != n || Wk.hyp != hyp) {
        // (the shape is recorded only after every allocation succeeded: a hipMalloc failure leaves n == -1 and the next call starts over)
        Wk.n = -1; Wk.nbits = nbits; Wk.hyp = hyp;
        Wk.forget();                                // (the window anchors of a hyperedge model carry a second array)
        Wk.ow.o_rec.release(); Wk.fl.loc.release();       // (the per-tile arrays are re-made for the new shape on first use)
        size_t plane = (size_t)nbits * (size_t)(n + 1);
        Wk.pl.opt.alloc(plane); Wk.pl.nnopt.alloc(plane); Wk.pl.cr.alloc(plane);
        if (hyp) { Wk.pl.nlopt.alloc(plane); Wk.pl.crl.alloc(plane); }
        // The winners are zeroed once: a speculatively sized layer may skip a stage that turns out to have work (the layer is then
        // redone), and until the redo later rounds read plane cells nobody wrote.  Whatever they hold must be a valid column
        // index -- a stale winner of an earlier layer is, fresh device memory is not (a k_lpass_own wave once streamed from
        // column 13868 of a 3000-column matrix).
        CP_HIP(hipMemsetAsync(Wk.pl.opt.p, 0, Wk.pl.opt.bytes(), A->stream));
        CP_HIP(hipMemsetAsync(Wk.pl.nnopt.p, 0, Wk.pl.nnopt.bytes(), A->stream));
        CP_HIP(hipMemsetAsync(Wk.pl.cr.p, 0, Wk.pl.cr.bytes(), A->stream));
        if (hyp) { CP_HIP(hipMemsetAsync(Wk.pl.nlopt.p, 0, Wk.pl.nlopt.bytes(), A->stream)); CP_HIP(hipMemsetAsync(Wk.pl.crl.p, 0, Wk.pl.crl.bytes(), A->stream)); }
        int64_t mx = n;
        for (int tau = 0; tau < nbits; tau++) { RoundDesc R; make_round(R, false, tau, nbits, n, 0, n); if (R.ntask > mx) mx = R.ntask; }
        // windowed layers give every row of a round a task in EVERY plane above tau (up to nbits - 1 - tau of them), and round A
        // one per head: sum_b (n >> b) < 2 n
        for (int tau = 0; tau < nbits; tau++) mx = std::max<int64_t>(mx, ((n >> (tau + 1)) + 1) * (int64_t)(nbits - 1 - tau));
        mx = std::max<int64_t>(mx, 2 * n + nbits);
        Wk.max_tasks = mx > 0 ? mx : 1;
        size_t mt = (size_t)Wk.max_tasks;
        Wk.tk.tdesc.alloc(mt); Wk.tk.len.alloc(mt); Wk.tk.tb.alloc(mt); Wk.tk.offs.alloc(mt + 1);
        if (hyp) Wk.tk.tS0l.alloc(mt);
        // tasks with tiles of their own have >= own_min >= 64 candidates; the ranges of one plane and round overlap in their end
        // points only: at most n / 64 + (rectangles) of them per plane -- (n / 32 + 64) per plane is a safe cap (k_setup_short guards it)
        int64_t mmin = std::max<int64_t>(2, std::min(g_opt_own_min, g_opt_gap_tau >= 0 ? g_opt_gap_min : g_opt_own_min));
        size_t mo = (size_t)(2 * n / mmin + 64) * (size_t)nbits + 1024;
        if (mo > mt) mo = mt;
        Wk.ow.o_tdesc.alloc(mo); Wk.ow.o_tb.alloc(mo); Wk.ow.o_rlen.alloc(mo); Wk.ow.o_ntl.alloc(mo); Wk.ow.o_toffs.alloc(mo + 1); Wk.ow.o_tick.alloc(mo); Wk.ow.o_ioffs.alloc(mo);
        Wk.ow.t_dirty = true;
        if (hyp) Wk.ow.o_tS0l.alloc(mo);
        Wk.sp.rc.alloc((size_t)NBMAX + 2);
        Wk.pl.fin.alloc(plane); Wk.pl.last_s0.alloc(64); Wk.pl.fin_stamp = 255;      // (fresh memory: the first layer clears it)
        Wk.pl.cr_dirty = false; Wk.pl.cr_ch = g_opt_rpass_ch;      // (cr / crl: cleared above)
        Wk.n = n;
    }
    // geometry of this call: wwin > 0: candidates of row r are max(0, r - wwin) <= p <= r
    Geo G{0, 0, 0};
    if (wwin > 0) { G.win = 1; G.w = wwin; G.s = 0; while (((int64_t)2 << G.s) <= wwin) G.s++; if (G.s > nbits - 1) G.s = nbits - 1; }
    // (w >= 2^(nbits-1) > n/2: planes 0 .. nbits-1 with S = 2^(nbits-1) <= w still tile every window -- the common block just
    //  reaches further left than column 0 and is clamped)
    Wk.G = G;
    if (G.win && (!Wk.win.built || Wk.win.w != wwin)) win_build<TC>(A, Wk);
    bool spec = Wk.sp.pred_ok && !g_opt_nospec && Wk.sp.pred_win == G.win && Wk.sp.pred_w == G.w;
    Wk.sp.pred_scale = 1.0;
    if (spec && (Wk.sp.pred_rlo != rlo || Wk.sp.pred_rhi != rhi)) {
        // another row tile than the layer the counts come from: the unconstrained driver keeps its tile, the constrained one moves
        // a window over the rows -- take the prediction per row of the tile
        const double a = (double)(Wk.sp.pred_rhi - Wk.sp.pred_rlo + 1), b = (double)(rhi - rlo + 1);
        // (a much larger tile than the counts come from -- the one-row last layer of an earlier call on this handle -- would
        //  scale a handful of tasks into buffers of any size: such a layer takes its exact counts instead)
        if (!G.win || a < 1 || b < 1 || b > 2.0 * a) spec = false;
        else Wk.sp.pred_scale = b / a;
    }
    if (Wk.sp.pred_win != G.win || Wk.sp.pred_w != G.w || (int)Wk.sp.force_own.size() != (G.win ? G.s + 1 : Wk.nbits) + 1) { Wk.sp.force_own.clear(); Wk.sp.force_rows = 0; }      // (another geometry: other rounds)
    // the layer's variant is chosen here, once: everything below is instantiated for it
    auto run = [&](bool sp, bool allow_force) {
        return hyp ? run_layer<TC, true>(A, M, alpha, W, cst_out, ptr_out, Wk, rlo, rhi, sp, allow_force)
                   : run_layer<TC, false>(A, M, alpha, W, cst_out, ptr_out, Wk, rlo, rhi, sp, allow_force);
    };
    if (run(spec, true)) return;
    // the prediction missed (a stage that had been empty, or a buffer too small): the same layer again with exact counts
    g_spec_redo++;
    Wk.sp.force_own.clear(); Wk.sp.force_rows = 0;
    bool ok = run(false, false);
    CP_REQUIRE(ok, CP_EINTERNAL, "DP layer failed with exact counts");
}

// Table-level window on a finished layer (tests): the per-block winners the combine step merges.  For every bit plane b and
// every row r (0-based) with bit b set, opt_out[b * (n+1) + r] = 1-based j of the RIGHTMOST arg-min of W[p] + f(p, r) over the
// row's Fenwick block [r_b - 2^b, r_b) and nn_out / nl_out the net (self-net) count of that part; 0 where bit b is clear.
// Valid for the rows the last dp_total_layer call computed.
template <typename TC>
int dp_total_block_tables(cp_csr_s *A, void *work_, int64_t *opt_out, int64_t *nn_out, int64_t *nl_out)
{
    auto &Wk = *reinterpret_cast<LayerWork<TC> *>(work_);
    const int64_t n = A->n, n1 = n + 1;
    CP_REQUIRE(Wk.n == n && Wk.pl.opt.p, CP_EINVAL, "no layer has been computed by the O(n log^2 n) scheme on this handle");
    CP_REQUIRE(Wk.pl.planes_full, CP_EINVAL, "the last layer kept no per-block winners for its leaf rows: cp_set_option(\"block_tables\", 1) before the layer");
    const size_t plane = (size_t)Wk.nbits * (size_t)n1;
    std::vector<int32_t> ho(plane), hn(plane), hl;
    CP_HIP(hipMemcpyAsync(ho.data(), Wk.pl.opt.p, plane * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    CP_HIP(hipMemcpyAsync(hn.data(), Wk.pl.nnopt.p, plane * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream));
    if (Wk.hyp && nl_out) { hl.resize(plane); CP_HIP(hipMemcpyAsync(hl.data(), Wk.pl.nlopt.p, plane * sizeof(int32_t), hipMemcpyDeviceToHost, A->stream)); }
    CP_HIP(hipStreamSynchronize(A->stream));
    for (int b = 0; b < Wk.nbits; b++)
        for (int64_t r = 0; r <= n; r++) {
            const size_t o = (size_t)b * (size_t)n1 + (size_t)r;
            opt_out[o] = 0; nn_out[o] = 0; if (nl_out) nl_out[o] = 0;
            if (r == 0 || !((r >> b) & 1)) continue;
            int t = 0; while (!((r >> t) & 1)) t++;
            const size_t slot = (size_t)b * (size_t)n1 + (size_t)((n - (n >> t)) + (r >> (t + 1)));      // prow(r, n)
            opt_out[o] = (int64_t)ho[slot] + 1; nn_out[o] = hn[slot];
            if (nl_out && !hl.empty()) nl_out[o] = hl[slot];
        }
    return Wk.nbits;
}
template int dp_total_block_tables<int64_t>(cp_csr_s *, void *, int64_t *, int64_t *, int64_t *);
template int dp_total_block_tables<double>(cp_csr_s *, void *, int64_t *, int64_t *, int64_t *);

template <typename TC> void *dp_total_work_new() { return new LayerWork<TC>(); }
template <typename TC> void dp_total_work_free(void *w) { delete reinterpret_cast<LayerWork<TC> *>(w); }
template <typename TC> static void work_reset_fn(void *w) { reinterpret_cast<LayerWork<TC> *>(w)->forget(); }
template <typename TC> void *dp_total_work_get(cp_csr_s *A)
{
    const int i = sizeof(TC) == sizeof(double) && ((TC)0.5 != (TC)0) ? 1 : 0;
    if (!A->dp_work[i]) { A->dp_work[i] = new LayerWork<TC>(); A->dp_work_free_fn[i] = dp_total_work_free<TC>; A->dp_work_reset_fn[i] = work_reset_fn<TC>; }
    return A->dp_work[i];
}
template void *dp_total_work_get<int64_t>(cp_csr_s *);
template void *dp_total_work_get<double>(cp_csr_s *);

template void dp_total_layer<int64_t>(cp_csr_s *, const DevModel<int64_t> &, int64_t, const int64_t *, int64_t *, int32_t *, void *, int64_t, int64_t, int64_t);
template void dp_total_layer<double>(cp_csr_s *, const DevModel<double> &, double, const double *, double *, int32_t *, void *, int64_t, int64_t, int64_t);
template void *dp_total_work_new<int64_t>();
template void *dp_total_work_new<double>();
template void dp_total_work_free<int64_t>(void *);
template void dp_total_work_free<double>(void *);

}  // namespace cpk
