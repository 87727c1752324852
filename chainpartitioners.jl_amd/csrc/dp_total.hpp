// dp_total.hpp -- what the units of the total-cost DP layer share (dp_total.hip, dp_total_own.hip, dp_total_rounda.hip,
// dp_total_rpass.hip, dp_total_gap.hip, dp_total_leaf.hip; nobody else includes it): the constants, the device helpers and
// kernel-argument records used by kernels of more than one unit, the work object of a handle (LayerWork, in groups by owner), the layer context (LayerCtx) and the stage functions
// the units offer the driver.  A device helper used by one unit stays in that unit.  No macros here.  The scheme: see dp_total.hip.
#pragma once
#include "csr.hpp"
#include "model.hpp"
#include "dp.hpp"
#include <algorithm>
#include <optional>

namespace cpk {

// The O(n log^2 n) scheme only admits the affine Work / Connectivity / HyperedgeCut models (fast_total_ok): its kernels evaluate
// costs through this three-way form, so the block-cost tables and pow() of the general dm_apply stay out of their registers.
template <typename TC>
__device__ __forceinline__ TC dm_apply_affine(const DevModel<TC> &m, TC alpha, int64_t nv, int64_t np, int64_t nn, int64_t nl)
{
    TC v = cadd(cadd(alpha, cmulc(nv, m.p[CP_P_VERTEX])), cmulc(np, m.p[CP_P_PIN]));       // (left to right, as the reference sums)
    if (m.kind == CP_MODEL_CONNECTIVITY) return cadd(v, cmulc(nn, m.p[CP_P_NET]));
    if (m.kind == CP_MODEL_HYPEREDGE_CUT) return cadd(cadd(v, cmulc(nl, m.p[CP_P_SELF_NET])), cmulc(nn - nl, m.p[CP_P_CUT_NET]));
    return v;
}

constexpr int LT = 256;          // steps per tile (one wave owns one tile)
constexpr int NBMAX = 31;        // bit planes (n < 2^30)
constexpr int SPLIT_BMIN = 8;     // own_split (SplitLinks): first plane whose own tiles stream only the plane's variable link entries (tiles are 256 columns: from here on a tile lies inside one block)
constexpr int SPLIT_NB = NBMAX - SPLIT_BMIN;      // ... and their number at most
constexpr int SMAX = 31;             // specials a tile of a gap round keeps (interior_stream<DET>); a tile with more is walked by the SLOW gap kernels
constexpr int FIX_SERIAL = 16;       // tasks of up to FIX_SERIAL tiles are merged by one lane
constexpr int FIX_U = 8;             // consecutive tiles per lane and trip of k_fix_own
constexpr int FIX_TRIP = 256 * FIX_U;
constexpr int FIX_REC_W = 5;         // what a trip leaves for the fold, as 8-byte words: {v, p | nn << 32, the trip's count, nl, the trip's second count}
constexpr int GAPSEG = 16;      // tiles one wave walks; longer tasks are walked by several waves (k_gap_seg) and merged (k_gap_merge)
constexpr int LEAF_T = 6;            // the rounds tau < LEAF_T are one leaf pass over groups of LEAF_G rows (dp_total_leaf.hip)
constexpr int LEAF_G = 1 << LEAF_T;
constexpr int LEAF_FEW = 12;             // local entries up to which the inner planes are one segmented scan (more: the column loop)
constexpr int LEAF_LIST = 1024;          // local link entries of a group kept in LDS; more: the columns are re-read from HBM

// Plane arrays (opt / nnopt / nlopt / cr / crl) hold row r of a bit plane at slot prow(r): rows are grouped by their level
// ctz(r) -- the rows one round reads and writes are then CONTIGUOUS in every plane (in row-major order they sit 2^(tau+1)
// entries apart and every round drags whole planes through HBM).  #rows in [1, n] with ctz < t is n - (n >> t).
__device__ __forceinline__ int64_t prow(int64_t r, int64_t n)
{
    int t = __ffsll((long long)r) - 1;
    return (n - (n >> t)) + (r >> (t + 1));
}

// Width-windowed layers (the ConstrainedCost DP, DynamicSplitter.jl:206-258 with a VertexCount weight; executable spec:
// tests/dc_model.py layer_windowed): candidates of row r are max(0, r - w) <= p <= r.  With s = floor(log2 w), S = 2^s, every row
// has a task in EVERY plane b <= s:
//   b < s, bit b of r set   : the standard Fenwick block [r_b - 2^b, r_b)
//   b == s                  : the common block [rho - w + S - 1, rho), rho = r with the bits below s cleared
//   b < s, bit b of r clear : the mirrored block [rho + 2^b - 1 - w, rho + 2^(b+1) - 1 - w), rho = r with the bits <= b cleared
// (clamped at column 0).  The rows sharing a block are always the aligned block of 2^b rows holding r -- full rectangles again.
struct Geo { int32_t win, s; int64_t w; };

// candidates [cs, ce) of row r in plane b; false: the row has no task in this plane (or the block is empty)
__host__ __device__ __forceinline__ bool geo_block(const Geo &G, int64_t r, int b, int64_t &cs, int64_t &ce)
{
    const int64_t lo = (r >> b) << b;
    if (!G.win) { cs = lo - ((int64_t)1 << b); ce = lo; return (r >> b) & 1; }
    if (b > G.s) return false;
    if (b == G.s) { cs = lo - G.w + ((int64_t)1 << b) - 1; ce = lo; }
    else if ((r >> b) & 1) { cs = lo - ((int64_t)1 << b); ce = lo; }
    else { cs = lo + ((int64_t)1 << b) - 1 - G.w; ce = cs + ((int64_t)1 << b); }
    if (cs < 0) cs = 0;
    if (ce < 0) ce = 0;
    return ce > cs;
}

// Per-round counters, on the device (one record per round, kept for the whole layer).  Kernels read their loop bounds from
// here, so the host can enqueue a whole layer without waiting for a count to come back (dp_total_layer).
struct RoundCounts {
    int32_t n_open, n_fix;            // work lists of k_span_short (tiles of long spans)
    int32_t nlong, nown;              // flattened tasks / tasks with tiles of their own (k_setup_short)
    unsigned long long own_steps;     // steps of the latter
    int64_t T, NT;                    // flattened steps / own tiles (scan totals)
    int32_t ntile, err;               // cdiv(T, LT); 1: a buffer sized from the prediction is too small (the layer is redone)
    int32_t n_items, _pad;            // (task, trip) items of the own-tiled tasks of more than FIX_SERIAL tiles (k_own_map -> k_fix_own)
    int32_t n_glong, n_gslots;        // gap tasks of more than GAPSEG tiles and their segment slots (k_gap_finish -> k_gap_seg)
    int32_t n_gslow, n_sslow;         // work items of k_gap_finish / k_gap_seg that met a tile with more than SMAX specials (redone by the SLOW variants)
    int32_t n_split, _pad2;           // own tiles that stream only their plane's variable link entries, where a launch mixes them with others (k_own_map, split == 2)
    int32_t n_trips, n_edge;          // what the merge met (cp_get_stat, tests): tasks of more than one trip (folded by k_fix_own); bit 0 / 1 / 2: a task of 1 / FIX_SERIAL / FIX_SERIAL + 1 tiles
    // round_alloc: what the blocks of k_setup_short have reserved of each list, slots << ALLOC_SH | units (steps of the flattened
    // tasks / tiles of the own-tiled ones), and the ticket its blocks draw when their records are written (zero between launches)
    unsigned long long alloc_l, alloc_o;
    uint32_t a_ticket, _pad3;
};
constexpr int ALLOC_SH = 40;                                          // a list's units fit 40 bits, its slots 24 (round_alloc_fits)
constexpr unsigned long long ALLOC_MASK = (1ull << ALLOC_SH) - 1ull;

// round_alloc: the packed words are wide enough for a round of `ntask` tasks whose flattened tasks have fewer than `own_min` steps
// and whose own-tiled ones at most n / 256 + 2 tiles; the wave-level prefix of the lengths is a 32-bit sum of 64 of them
inline bool round_alloc_fits(int64_t ntask, int64_t n, int64_t own_min)
{
    if (ntask < 0 || ntask >= ((int64_t)1 << 24) || own_min < 1 || own_min > ((int64_t)1 << 24)) return false;
    const int64_t lim = (int64_t)1 << ALLOC_SH;
    return ntask * (n / 256 + 2) < lim && ntask * own_min < lim;
}

// The tasks of a round, by value to every kernel that decodes them (make_round: dp_total.hip)
struct RoundDesc {
    int32_t isA, tau, nbits, nextra;
    Geo G;                      // G.win: nbits = s + 1 planes, every row takes part in each of them
    int64_t aoff[32];           // windowed round A: anchors of the mirrored head tasks of plane b start at aoff[b] (index r >> (b+1))
    int64_t n, ntask;
    int64_t tbase[36];          // tau rounds: tasks of bit plane b occupy [tbase[b], tbase[b+1])
    int64_t tskip[36];          // ... and start at linear index tskip[b] of that plane (row-tiled runs skip rows left of the tile)
    int64_t a_r0, a_nmain;      // round A: rows a_r0 .. a_r0 + a_nmain - 1, then the `extra` rows (ancestors outside the tile)
    int64_t extra[64];
    // round A also takes the LAST row n in every bit plane above its lowest one (tasks after the extra rows): no row lies to
    // its right, so nothing bounds the rows next to it from the left; with opt[b][n] known first, they start there instead of
    // at the block start -- which every round would otherwise re-scan (n is not a power of two: ~n steps per round)
    int32_t nlast, last_b[31];
    int32_t skip_std, skip_mir; // windowed round A: the standard / mirrored heads (bit b of the row set / clear, b < s) come from the cached counts
    int32_t fin_stamp;          // a cell of the `fin` plane is set iff it holds this layer's stamp (1 .. 255: the plane is cleared every 255 layers, not every layer)
};

__device__ __forceinline__ void decode_task(const RoundDesc &R, int64_t t, int64_t &r, int &b)
{
    if (R.G.win) {
        // plane-major.  Round A: plane b <= s holds the rows that are multiples of 2^b (the heads of its rectangles);
        // round tau: every plane b in (tau, s] holds all rows with ctz == tau
        int bb = R.isA ? 0 : R.tau + 1;
        while (t >= R.tbase[bb + 1]) bb++;
        const int64_t l = t - R.tbase[bb] + R.tskip[bb];
        r = R.isA ? ((l + 1) << bb) : (((l << 1) | 1) << R.tau);
        b = bb;
        return;
    }
    if (R.isA) {
        if (t >= R.a_nmain + R.nextra) { r = R.n; b = R.last_b[t - R.a_nmain - R.nextra]; return; }
        r = t < R.a_nmain ? R.a_r0 + t : R.extra[t - R.a_nmain]; b = __ffsll((long long)r) - 1; return;
    }
    int bb = R.tau + 1;
    while (t >= R.tbase[bb + 1]) bb++;
    int64_t l = t - R.tbase[bb] + R.tskip[bb];
    int sh = bb - R.tau - 1;
    int64_t base = l >> sh, v = l & (((int64_t)1 << sh) - 1);
    r = (base << (bb + 1)) | ((int64_t)1 << bb) | (((v << 1) | 1) << R.tau);
    b = bb;
}

// the record of a candidate: value, column, counts (helpers: below, behind the shuffles; scans: dp_total_stream.hpp)
template <typename TC, bool HYP> struct Best;
template <typename TC> struct Best<TC, false> { TC v; int32_t p; int32_t nn; };                         // 16 bytes
template <typename TC> struct Best<TC, true> { TC v; int32_t p; int32_t nn; int32_t nl; int32_t _pad; };

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int o)
{
    int lo = __shfl_up((int)(v & 0xffffffffll), o), hi = __shfl_up((int)(v >> 32), o);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ double shfl_up64(double v, int o) { return __longlong_as_double((long long)shfl_up64((int64_t)__double_as_longlong(v), o)); }
__device__ __forceinline__ int64_t shfl64(int64_t v, int src)
{
    int lo = __shfl((int)(v & 0xffffffffll), src), hi = __shfl((int)(v >> 32), src);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ double shfl64(double v, int src) { return __longlong_as_double((long long)shfl64((int64_t)__double_as_longlong(v), src)); }


// wave-uniform lane index: one v_readlane instead of a ds_bpermute
__device__ __forceinline__ int32_t rdl(int32_t v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ int64_t rdl64(int64_t v, int src)
{
    return ((int64_t)__builtin_amdgcn_readlane((int)(v >> 32), src) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), src);
}
__device__ __forceinline__ double rdl64(double v, int src) { return __longlong_as_double((long long)rdl64((int64_t)__double_as_longlong(v), src)); }

template <typename TC> __device__ __forceinline__ void best_clear(Best<TC, false> &b) { b.v = (TC)0; b.p = -1; b.nn = 0; }
template <typename TC> __device__ __forceinline__ void best_clear(Best<TC, true> &b) { b.v = (TC)0; b.p = -1; b.nn = 0; b.nl = 0; b._pad = 0; }
template <typename TC> __device__ __forceinline__ int32_t best_nl(const Best<TC, false> &) { return 0; }
template <typename TC> __device__ __forceinline__ int32_t best_nl(const Best<TC, true> &b) { return b.nl; }
template <typename TC> __device__ __forceinline__ void best_set_nl(Best<TC, false> &, int32_t) {}
template <typename TC> __device__ __forceinline__ void best_set_nl(Best<TC, true> &b, int32_t v) { b.nl = v; }

// (member-wise selects on values: returning `cond ? b : a` through references makes the compiler select between the two
//  ADDRESSES -- one of them often a global-memory record -- and keeps the local operand in private memory: 24-96 B of scratch
//  per lane and 0.5 GB of HBM writes per launch of the streaming kernel in round 1's profile)
template <typename TC>
__device__ __forceinline__ Best<TC, false> best_sel(bool tb, const Best<TC, false> a, const Best<TC, false> b)
{
    Best<TC, false> r; r.v = tb ? b.v : a.v; r.p = tb ? b.p : a.p; r.nn = tb ? b.nn : a.nn; return r;
}
template <typename TC>
__device__ __forceinline__ Best<TC, true> best_sel(bool tb, const Best<TC, true> a, const Best<TC, true> b)
{
    Best<TC, true> r; r.v = tb ? b.v : a.v; r.p = tb ? b.p : a.p; r.nn = tb ? b.nn : a.nn; r.nl = tb ? b.nl : a.nl; r._pad = 0; return r;
}
template <typename TC, bool HYP>
__device__ __forceinline__ Best<TC, HYP> better(const Best<TC, HYP> a, const Best<TC, HYP> b)   // a is earlier (larger p): wins ties
{
    const bool tb = a.p < 0 || (b.p >= 0 && b.v < a.v);
    return best_sel<TC>(tb, a, b);
}

// ------------------------------------------------------------------ tile geometry of the tasks with tiles of their own (see k_own_map)
__host__ __device__ __forceinline__ int32_t own_ntiles(int blk, int64_t B, int64_t L)
{
    return blk ? (int32_t)(B / LT - (B - L + 1) / LT + 1) : (int32_t)((L + LT - 1) / LT);
}
// tile kt of a task with head B and L steps: steps 0 .. tl of the tile are the columns pf .. pf - tl (the tile is the task's head
// tile iff kt == 0: its step 0 is the candidate B itself, no column stepped over)
__device__ __forceinline__ void own_tile_geo(int blk, int32_t B, int32_t L, int32_t kt, int32_t &pf, int32_t &tl)
{
    if (blk) {
        const int32_t a = B - L + 1;
        pf = kt == 0 ? B : (B / LT - kt) * LT + (LT - 1);
        const int32_t c0 = pf - pf % LT;
        tl = pf - (a > c0 ? a : c0);
    } else {
        pf = B - kt * LT;
        const int32_t rest = L - kt * LT;                // steps of the task from this tile on
        tl = (rest < LT ? rest : LT) - 1;
    }
}

// ------------------------------------------------------------------ a cached round-A table (layout: dp_total_rounda.hip, round A from cached counts)
struct RATab { int32_t nbits, _pad; int64_t n; int64_t tbase[33]; int64_t rbase[33]; int64_t mir_w; int64_t aoff[33]; int64_t tlo[33], thi[33]; };


// ------------------------------------------------------------------ the link entries split by plane (own_split)
// A left step of a task (row r, plane b) over column p counts the entries of p with next >= r.  The task's columns lie in the
// Fenwick block [r_b - 2^b, r_b), r in [r_b, r_b + 2^b).  With h = the highest bit in which p and x = next[q] differ (-1: none):
//   h < b: x lies in p's own block, below r_b: no row of the rectangle counts the entry;
//   h > b: x >= r_b + 2^b: every row counts it -- a constant of (column, plane);
//   h == b: x lies in the sibling block: the only entries whose contribution depends on r ("variable in plane b").
// Every entry is variable in exactly one plane.  For the planes b = SPLIT_BMIN .. nbits - 1 (nb of them, index b - SPLIT_BMIN):
//   vnext: the variable entries' next values, plane-major, column-major inside a plane, entry order inside a column (+ 8 of slack);
//   vpos[b][p], p = 0 .. n: where column p's plane-b entries start in vnext (vpos[b][n] = vpos[b + 1][0]; one word more: the total);
//   vsa[b][p]: #{entries of the columns < p with h > b}.
// They depend on the pattern only: built once per partition, by the first layer that uses them (split_build).
// own_pack: vpos and vsa only enter a tile as differences inside its 256-column block (own_blk 1: a tile lies inside one block), so
// with c0 = p & ~255 one word per (plane, column) and one base pair per (plane, block) carry them:
//   vpk[b][p] = (vpos[b][p] - vpos[b][c0]) | (vsa[b][p] - vsa[b][c0]) << 16, stride n + 1;
//   vbase[b][k] = {vpos[b][256 k], vsa[b][256 k]}, k = 0 .. nblk - 1, stride nblk + 1; vbase[b][nblk] = {the end of the plane's entries, 0}.
// Both offsets grow with p inside a block; the build keeps the largest of each (vmax).  packed: both fit 16 bits.  Where they do not,
// and for the tiles that straddle blocks (own_blk 0), the wide vsa is made from vpos when it is first asked for (split_wide).
struct SplitLinks {
    bool built = false, packed = false, has_wide = false;
    int nb = 0;
    int64_t stride = 0;                        // n + 1
    int64_t nblk = 0;                          // 256-column blocks of a plane: cdiv(n + 1, 256)
    int64_t tot[SPLIT_NB + 1] = {0};           // variable entries per plane; [nb]: all of them
    int32_t max_off[2] = {0, 0};               // the largest in-block offset of vpos / of vsa
    DBuf<int32_t> vnext, vpos, vsa, vpk, vmax; // (vpk: the counts until the scatter writes it; vsa: empty until split_wide)
    DBuf<int2> vbase;
};

// items a round of `nt` own tiles can list: one per FIX_TRIP tiles and at most one partial trip per task of more than FIX_SERIAL tiles
inline size_t fix_items_cap(size_t nt) { return nt / FIX_TRIP + nt / (FIX_SERIAL + 1) + 2; }
// ... and the items of one task of `ntl` tiles: one per trip where a block merges it (the rule k_own_map lists its trip starts by)
__host__ __device__ __forceinline__ int32_t fix_items_of(int64_t ntl) { return ntl > FIX_SERIAL ? (int32_t)((ntl + FIX_TRIP - 1) / FIX_TRIP) : 0; }

// ================================================================== host side
// The work object of a handle: the shape, and one group of members per owner.

// The planes and what marks them: per (plane, row) the winner, its counts and the right-part counts, at slot prow(r).
struct Planes {
    DBuf<int32_t> opt, nnopt, cr;
    DBuf<int32_t> nlopt, crl;                           // hyperedge-cut: second (self-net) count
    DBuf<uint8_t> fin;                                  // rows already final (per plane slot) ...
    int fin_stamp = 255;                                // ... iff the cell holds the current layer's stamp (run_layer; 255: cleared before the next layer)
    DBuf<int32_t> last_s0;                              // anchors of the last row's round-A tasks ([b], [32 + b])
    bool cr_dirty = true;                               // cr / crl may hold counts nobody will consume (cr_consume: the next full layer clears as before)
    int64_t cr_ch = 0;                                  // the rpass_ch the planes were left clean under (another value: other rounds add in chunks)
    DBuf<int32_t> pz;                                   // poison mode: cells read that nobody wrote
    bool planes_full = false;                           // the last layer stored every per-block winner (cp_dp_block_tables)
};

// The task records of set-up: the round's flattened tasks (k_setup_short appends, k_round_scans turns len into offs).
struct SetupTasks {
    DBuf<int4> tdesc;                                   // per task {B, anchor count, row r, pos32[r]}
    DBuf<uint8_t> tb;
    DBuf<int32_t> len, tS0l;                            // (tS0l: hyperedge-cut)
    DBuf<int64_t> offs;
};

// Scratch of the scans, shared by the stages (one stream: never two users at a time).
struct ScanScratch {
    DBuf<int64_t> scratch;
    DBuf<int64_t> ra_G;                                 // prefix sums while the counts of a round-A table are built
    ScanWS scanws;                                      // single-launch scans of the rounds
};

// The flattened stage: per-step and per-tile arrays (k_tile_t0 -> k_lpass -> k_span_short / k_open / k_fix).
template <typename TC>
struct FlatStage {
    DBuf<int32_t> loc, tileS;
    DBuf<int32_t> loc2, tileS2;                         // hyperedge-cut: second (self-net) count
    DBuf<int64_t> taskR, tilePS, tilePS2, tile_t0;
    DBuf<Best<TC, true>> partL, partR;                  // sized for the larger record; reinterpreted per variant
    DBuf<int32_t> open_list, fix_list;                  // tiles of long spans (k_span_short -> k_open / k_fix)
    DBuf<int4> tile_rec;                                // {first column, row, -, interior?} per tile (k_tile_t0)
    // (loc is the size witness of the group: released first and allocated LAST, so a hipMalloc failure in the middle leaves the
    //  witness empty and the next call allocates the whole group again)
    void ensure_flat(bool hyp, size_t T) {
        if (loc.n >= T && loc.n > 0) return;
        size_t c = T > 0 ? T : 1, nt = (c + LT - 1) / LT;
        loc.release();
        if (hyp) loc2.alloc(c);
        tileS.alloc(nt); tilePS.alloc(nt + 1); tile_t0.alloc(nt); partL.alloc(nt); partR.alloc(nt); taskR.alloc(nt);
        open_list.alloc(nt); fix_list.alloc(nt); tile_rec.alloc(nt);
        if (hyp) { tileS2.alloc(nt); tilePS2.alloc(nt + 1); }
        loc.alloc(c);
    }
};

// The tasks with tiles of their own (k_own_map -> k_blk_order -> k_lpass_own -> k_fix_own, or the gap kernels).
template <typename TC>
struct OwnTiles {
    DBuf<int4> o_tdesc, o_rec;
    DBuf<uint8_t> o_tb;
    DBuf<int32_t> o_rlen, o_ntl, o_tS0l, o_task, o_tileS, o_tileS2, o_hi;
    DBuf<int64_t> o_toffs, o_tilePS, o_tilePS2;
    DBuf<int32_t> o_ioffs;                              // round_alloc: per task, its first merge item (trip j: o_ioffs[t] + j)
    DBuf<Best<TC, true>> o_part;
    // the merge of the own tiles (k_fix_own): its items {task, first tile} and each trip-start tile's item (k_own_map), one record per
    // item, one ticket per task (zero between rounds: the folder of a task puts it back)
    DBuf<int2> o_items; DBuf<int32_t> o_item_of; DBuf<unsigned long long> o_trec; DBuf<uint32_t> o_tick;
    bool t_dirty = true;                                // o_tick may hold tickets (run_layer clears it before its first round)
    DBuf<Best<TC, true>> o_sub;                         // gap passes: segment winners of the tiles with specials, [tile][SMAX + 1]
    DBuf<int32_t> o_spv;                                // ... and the specials between them
    DBuf<uint8_t> o_spec;                               // ... and the flagged tiles
    // own_blk: the tiles sorted by 256-column block (k_own_map -> scan -> k_blk_order)
    DBuf<int32_t> b_cnt, b_n, o_brank, o_border;        // tiles per block, the block count (device); per tile: rank in its block, tile ids in block order
    DBuf<int4> o_srec;                                  // ... and the tiles' records (o_rec) in block order
    DBuf<int64_t> b_start;
    int64_t b_nblk = 0;
    bool b_dirty = true;                                // b_cnt may hold counts (run_layer clears it before its first round)
    SplitLinks split;                                   // the link entries by plane (own_split): built by the first layer that uses them
    // (o_rec is the size witness of the per-tile arrays, like FlatStage::loc)
    void ensure_own(bool hyp, size_t NT) {
        if (o_rec.n >= NT && o_rec.n > 0) return;
        size_t c = NT > 0 ? NT : 1;
        o_rec.release();
        o_task.alloc(c); o_tileS.alloc(c); o_tilePS.alloc(c + 1); o_part.alloc(c); o_hi.alloc(c); o_spec.alloc(c); o_brank.alloc(c); o_border.alloc(c); o_srec.alloc(c);
        o_item_of.alloc(c); o_items.alloc(fix_items_cap(c)); o_trec.alloc(fix_items_cap(c) * FIX_REC_W);
        o_sub.alloc(c * (SMAX + 1)); o_spv.alloc(c * (SMAX + 1));
        if (hyp) { o_tileS2.alloc(c); o_tilePS2.alloc(c + 1); }
        o_rec.alloc(c);
    }
};

// The gap passes (k_gap_finish -> k_gap_seg -> k_gap_merge).
struct GapPass {
    DBuf<int2> g_slot;                                  // segment slot -> {task, segment}
    DBuf<int2> g_list;                                  // gap tasks of more than GAPSEG tiles: {task, first segment slot}
    DBuf<char> g_seg;                                   // their segment records (GapSegRec)
    DBuf<int32_t> g_slow, g_sslow;                      // work items of k_gap_finish / k_gap_seg left to the SLOW variants
};

// The window anchors: anchors of the mirrored head tasks of the windowed layers, cached per (pattern, w) (win_build).
struct WinAnchors {
    bool built = false; int64_t w = -1, nitems = 0, aoff[33];
    DBuf<int32_t> w_anch, w_anch2, w_tot, w_hist;
    DBuf<int32_t> leaf_anch, leaf_anch2;                // leaf pass of windowed layers: nets / self nets of [64 g + 62 - w, 64 g) per group
    DBuf<int64_t> w_E;
};

// A cached round-A table with its counts (ra_build): once for the unconstrained scheme's round A (w = 0; the windowed layers'
// standard heads are its levels below s), once for the mirrored heads of a window width w.
template <typename TC>
struct RaCache {
    bool built = false; RATab tab; int64_t ntile = 0, nrow = 0, w = 0;
    DBuf<int32_t> c, c2;
    DBuf<Best<TC, true>> part;                          // partials of the rows of more than LT candidates
};

// The speculation state: the counts of the current layer and what the last one says about the next (run_layer).
struct SpecState {
    DBuf<RoundCounts> rc;                               // per-round counters of the current layer (device)
    std::vector<RoundCounts> pred;                      // ... of the previous layer (host): sizes the next one
    bool pred_ok = false; int64_t pred_rlo = 0, pred_rhi = 0; double pred_scale = 1.0; int pred_win = 0; int64_t pred_w = 0;
    // rounds whose flattened stage served a handful of tasks in the last layer that ran it: their medium tasks get tiles of their
    // own from then on and the stage (six dependent launches, ~40 us) is skipped -- see run_layer
    std::vector<uint8_t> force_own;
    int64_t force_rows = 0;               // rows of the layer the flags come from (a one-row last layer says nothing about a full one)
};

template <typename TC>
struct LayerWork {
    int64_t n = -1; int nbits = 0; bool hyp = false;    // the shape the buffers are made for
    Geo G{0, 0, 0};                                     // windowed layers: geometry of the current call
    int64_t max_tasks = 0;
    Planes pl;
    SetupTasks tk;
    ScanScratch sc;
    FlatStage<TC> fl;
    OwnTiles<TC> ow;
    GapPass gp;
    WinAnchors win;
    RaCache<TC> ra, mir;                                // the standard table; the mirrored heads of a window width (mir.w)
    SpecState sp;
    // what the pattern's cached tables and the last layer's counts say no longer holds (another pattern, another shape)
    void forget() { ra.built = false; ow.split.built = false; sp.pred_ok = false; win.built = false; mir.built = false; sp.force_own.clear(); sp.force_rows = 0; }
};

// What a layer fixes once; every stage function takes it.  begin_layer (dp_total.hip) returns it after enqueuing the clears in front
// of the first round and taking the layer's `fin` stamp.  Self-contained: the model is held by value.
template <typename TC>
struct LayerCtx {
    cp_csr_s *A; hipStream_t s;
    DevModel<TC> M; TC alpha; const TC *W;      // the model and the previous layer's costs
    TC *cst_out; int32_t *ptr_out;
    int64_t n, rlo, rhi;                                // rows [rlo, rhi] of 0 .. n are computed
    Geo G; int nbits;                                   // windowed layers: planes 0 .. s
    bool spec;                                          // sized from the previous layer's counts (false: exact counts, one host sync per round)
    bool own_tiles, gaps, split_layer, leaf;            // stages the layer may use
    int oblk;                                           // the tile geometry of the own-tiled tasks (own_tile_geo)
    int ra_bmin;                                        // round A from the cache starts at this level
    int32_t *pzp;                                       // poison mode: the hit counters (null: off)
    double avg_deg, self_deg, step_bytes;               // link entries per column; bytes a step of the streaming kernels moves
    bool cr_zero, cr_consume;                           // set-up zeroes the cr / crl cells it reads; ... and the planes are clean: no clearing launch (begin_layer)
    // bytes the own-tile stream moves: split tiles read two column pointers and a prefix sum per step (20 B with the cost; sp == 2,
    // own_pack: the plane's pointer and prefix sum are one word, 16 B) and the variable entries of the round's planes, at most what
    // the columns hold.  (Tiles of planes below SPLIT_BMIN in the same launch --
    // the plane-7 tiles of the gap round tau = 6 -- are priced like the others.)
    double own_bytes(const SplitLinks &S, int tau, int sp, double steps) const {
        if (!sp) return steps * step_bytes;
        double var = 0;
        for (int b = std::max(tau + 1, SPLIT_BMIN); b < nbits && b - SPLIT_BMIN < S.nb; b++) var += (double)S.tot[b - SPLIT_BMIN];
        return steps * ((sp == 2 ? 16.0 : 20.0) + 32.0 / (double)LT) + 4.0 * std::min(var, avg_deg * steps);
    }
};

inline int64_t grow_pred(int64_t v) { return v + (v >> 2) + 1024; }     // head room over a predicted count

// A layer's variant (HYP: hyperedge costs, with the second count) is fixed when the layer starts: run_layer<TC, HYP> and what it
// calls see the work buffers through these two.
// the record buffers are sized for the larger record and read as the variant's own
template <bool HYP, typename TC> inline Best<TC, HYP> *recs(const DBuf<Best<TC, true>> &b) { return reinterpret_cast<Best<TC, HYP> *>(b.p); }
// the arrays of the second (self-net) count: the kernels of the other variant get null
template <bool HYP, typename T> inline T *if_hyp(T *p) { return HYP ? p : nullptr; }

// ---- the stage functions of the other units: defined there, external, instantiated for TC in {int64_t, double} x HYP (a unit's
// kernels are named in that unit only; nothing calls across units on the device)
// dp_total_rpass.hip: the right pass
template <typename TC, bool HYP> void right_pass(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R);
template <typename TC, bool HYP> void last_row_counts(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R);
// dp_total_gap.hip: the gap passes
template <typename TC, bool HYP> void gap_finish(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P);
// dp_total_leaf.hip: the leaf pass and the combine
template <typename TC, bool HYP> void leaf_pass(const LayerCtx<TC> &C, LayerWork<TC> &Wk);
template <typename TC, bool HYP> void combine_rows(const LayerCtx<TC> &C, LayerWork<TC> &Wk);
// dp_total_rounda.hip: the window anchors (instantiated for TC; dp_total_layer builds them) and round A from the cached tables
// (`scope`: opened by round_a_win_std, closed by run_layer behind round_a_win_mir)
template <typename TC> void win_build(cp_csr_s *A, LayerWork<TC> &Wk);
template <typename TC, bool HYP> void round_a_full(const LayerCtx<TC> &C, LayerWork<TC> &Wk);
template <typename TC, bool HYP> void round_a_win_std(const LayerCtx<TC> &C, LayerWork<TC> &Wk, std::optional<ProfScope> &scope);
template <typename TC, bool HYP> bool round_a_win_mir(const LayerCtx<TC> &C, LayerWork<TC> &Wk);
// dp_total.hip: the tasks of a round (win_build lists the mirrored heads with it)
void make_round(RoundDesc &R, bool isA, int tau, int nbits, int64_t n, int64_t rlo, int64_t rhi, const Geo &G = Geo{0, 0, 0}, const int64_t *aoff = nullptr);

}  // namespace cpk
