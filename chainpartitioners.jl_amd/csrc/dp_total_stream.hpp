// dp_total_stream.hpp -- the TILE STREAM of the total-cost DP layer (scheme: dp_total.hip): the device primitives of the kernels that
// stream the link array one 256-step tile per wave -- the segmented wave scans, the cooperative column counts and the uniform tile's
// stream, whole (interior_stream) and in parts (tile_head_loads .. tile_trips).  Included by exactly the units that stream tiles:
// dp_total_own.hip (k_lpass_own) and dp_total.hip (the flattened stage's k_lpass).
#pragma once
#include "dp_total.hpp"

namespace cpk {

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

}  // namespace cpk
