// dp_total_own.hpp -- what dp_total.hip shares with the own-tile unit (dp_total_own.hip; nobody else includes it): the two host
// helpers both use, and the stage functions of the own-tile chain of a round.
#pragma once
#include "dp_total.hpp"

namespace cpk {

// (windowed layers keep one tile per wave: their tiles stream whole columns, ten trips and more, and paired they ran 5 % slower)
template <bool HYP> static bool own_pairs(bool gap, bool win) { return !HYP && !gap && !win && g_opt_own_pair != 0; }

// cp_set_option("dbg", DBG_POISON [+ DBG_POISON_ZERO]): fills buffers a stage must write before it reads (null: not of this variant)
static void poison_fill(hipStream_t s, std::initializer_list<std::pair<void *, size_t>> bufs)
{
    if (!(g_opt_dbg & DBG_POISON)) return;
    const int pat = (g_opt_dbg & DBG_POISON_ZERO) ? 0x00 : 0x7F;
    for (const auto &b : bufs) if (b.first) CP_HIP(hipMemsetAsync(b.first, pat, b.second, s));
}

// ---- dp_total_own.hip: the own-tile chain of a round (defined there, external, instantiated for TC in {int64_t, double} x HYP)
template <typename TC, bool HYP>
bool own_stream(const LayerCtx<TC> &C, LayerWork<TC> &Wk, const RoundDesc &R, RoundCounts *rc, const RoundCounts &P, bool gap, int split, bool ralloc);
template <typename TC, bool HYP> void own_merge(const LayerCtx<TC> &C, LayerWork<TC> &Wk, RoundCounts *rc, const RoundCounts &P, bool ralloc);

}  // namespace cpk
