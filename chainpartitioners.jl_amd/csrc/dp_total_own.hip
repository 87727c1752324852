// dp_total_own.hip -- the OWN-TILE CHAIN of a round of the total-cost DP layer (scheme: dp_total.hip): the tasks long enough for
// tiles of their own are mapped to tiles (k_own_map, k_blk_order), streamed and evaluated one wave per tile or pair of tiles
// (k_lpass_own, on the tile stream of dp_total_stream.hpp; its GAP form feeds the gap passes of dp_total_gap.hip) and merged
// (k_fix_own); with the link entries split by plane (SplitLinks) and the test entries of this code.
#include "dp_total_own.hpp"
#include "dp_total_stream.hpp"

namespace cpk {

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

// ------------------------------------------------------------------ host side: the own-tile chain of a round
// Map and stream + evaluate.  split (run_layer): 0: whole columns; 1: every tile of the launch is of a plane >= SPLIT_BMIN, their
// number is NT; 2: the launch also holds tiles of the planes below -- the gap round tau = 6 with its plane-7 tiles, and every
// round below it with gap_tau < 6 -- and k_own_map counts: 1 600 same-address atomics per launch cost it 17 us at config 3.
// cp_set_option("own_pack", 0 | 1): the split tiles of a launch take the packed words where the geometry keeps a tile inside one block
// (own_blk 1) and the pattern's offsets fit 16 bits -- except in a paired launch that also holds tiles of the planes below (gap_tau
// below 6): a wave's two tiles run one text.  Returns whether they did.
template <typename TC, bool HYP>
bool own_stream(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P, bool gap, int split, bool ralloc)
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
void own_merge(const LayerCtx<TC> &C, LayerWork<TC> &Wk, RoundCounts *rc, const RoundCounts &P, bool ralloc)
{
    ProfScope ps(PROF_FIX, C.s, 24.0 * (double)P.NT);
    launch_fix_own<TC, HYP>(C.s, rc, Wk.ow.o_toffs.p, recs<HYP>(Wk.ow.o_part), Wk.ow.o_tdesc.p, Wk.ow.o_tb.p, if_hyp<HYP>(Wk.ow.o_tS0l.p), Wk.ow.o_tileS.p,
                            if_hyp<HYP>(Wk.ow.o_tileS2.p), C.M, Wk.pl.opt.p, Wk.pl.nnopt.p, if_hyp<HYP>(Wk.pl.nlopt.p), C.n, Wk.ow.o_items.p, Wk.ow.o_item_of.p, Wk.ow.o_trec.p,
                            Wk.ow.o_tick.p, C.spec ? grow_pred(P.NT) : P.NT, C.spec ? grow_pred(P.nown) : P.nown,
                            ralloc ? Wk.ow.o_ioffs.p : (const int32_t *)nullptr);
}

#define CP_INST(TC, HYP) \
    template bool own_stream<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, const RoundDesc &, RoundCounts *, const RoundCounts &, bool, int, bool); \
    template void own_merge<TC, HYP>(const LayerCtx<TC> &, LayerWork<TC> &, RoundCounts *, const RoundCounts &, bool);
CP_INST(int64_t, false) CP_INST(int64_t, true) CP_INST(double, false) CP_INST(double, true)
#undef CP_INST

}  // namespace cpk

