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
// Units: the right pass is dp_total_rpass.hip, the gap passes are dp_total_gap.hip, the leaf pass and the combine dp_total_leaf.hip,
// the own-tile chain of a round dp_total_own.hip, round A from the cached counts and the windowed anchors dp_total_rounda.hip;
// task set-up with the round allocator and the scans, the flattened stage and the layer driver are here.  What the units share:
// dp_total.hpp; with the own-tile unit also dp_total_own.hpp and the tile stream, dp_total_stream.hpp.
#include "dp_total_own.hpp"
#include "dp_total_stream.hpp"

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
void make_round(RoundDesc &R, bool isA, int tau, int nbits, int64_t n, int64_t rlo, int64_t rhi, const Geo &G, const int64_t *aoff)      // (defaults: dp_total.hpp)
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

constexpr int64_t LB_MAX = 1 << 20;      // largest scan (elements) done in a single launch

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
