// lws_plan.hpp -- the launch plan of one unconstrained total-cost layer on the rectangle engine (lws_rect.hpp): the decomposition of
// the triangle lo <= p <= min(r, hi), rlo <= r <= rhi (lws_decomp.hpp) grouped by the depth of the column tree.  It depends on the
// layer geometry and the engine's limits only, not on the cost: sym_total.hip and plaid_total.hip share it.
//
// Every block [ja, jb] of the column tree owns at most one rectangle, the rows [jb, the parent's jb - 1]: the rectangles found at one
// depth have pairwise disjoint rows and pairwise disjoint columns, and so have the partial rows of its leaves.  A depth is therefore
// ONE launch sequence -- the levels of its large rectangles together (LwsBatch), one scan launch for its small rectangles, one for
// its partial rows: at most D (4 L + 2) launches per layer for D depths and L = ceil(log2(n + 1)) levels.  A rectangle's rows and a
// leaf's partial rows of the same depth may coincide, which is why those two are separate launches.
#pragma once
#include "lws_rect.hpp"
#include "lws_decomp.hpp"
#include <cstring>
#include <memory>
#include <vector>

namespace cpk {

// the two staircases in closed form: a(r) = lo, b(r) = min(r, hi)
struct LwsTriStairs {
    int64_t lo, hi;
    int64_t first_b_ge(int64_t x, int64_t y, int64_t v) const
    {
        if (v > hi) return y + 1;
        const int64_t r = std::max(x, v);
        return r > y ? y + 1 : r;
    }
    int64_t last_a_le(int64_t x, int64_t y, int64_t v) const { return lo <= v ? y : x - 1; }
};

// per depth of the column tree: the large rectangles with the prefixes of their row counts level by level, the small rectangles and
// the partial rows with the prefixes of their rows; all descriptors in one device array, all prefixes in another
struct LwsPlan {
    static constexpr int NKEY = 7;
    int64_t key[NKEY];                           // rlo, rhi, lo, hi, stair_cols, scan_cells, scan_cols
    struct Rows { int64_t rd, pre, nr, rows; };
    struct Level { int64_t h, pre, cnt, cap; };
    struct Depth { int64_t rd, nr; std::vector<Level> levels; Rows small, stair; };
    std::vector<Depth> depths;
    std::vector<LwsRectD> hrd;                   // (the host copies live as long as the plan: the upload reads them)
    std::vector<int32_t> hpre;
    DBuf<LwsRectD> rd;
    DBuf<int32_t> pre;
};

struct LwsPlanSink {
    struct Lists { std::vector<LwsRectD> big, small, stair; };
    std::vector<Lists> d;
    int64_t scan_cells, scan_cols;
    Lists &at(int depth)
    {
        if ((size_t)depth >= d.size()) d.resize((size_t)depth + 1);
        return d[(size_t)depth];
    }
    void rect(int depth, int64_t ja, int64_t jb, int64_t ra, int64_t rb)
    {
        const int64_t m = rb - ra + 1, cols = jb - ja + 1;
        const bool whole = cols <= scan_cols && m * cols <= scan_cells;      // (LwsRect::rect's rule)
        (whole ? at(depth).small : at(depth).big).push_back({(int32_t)ra, (int32_t)m, (int32_t)ja, (int32_t)jb});
    }
    void stair(int depth, int64_t ja, int64_t jb, int64_t ra, int64_t m, int64_t ra2, int64_t m2)
    {
        if (m > 0) at(depth).stair.push_back({(int32_t)ra, (int32_t)m, (int32_t)ja, (int32_t)jb});
        if (m2 > 0) at(depth).stair.push_back({(int32_t)ra2, (int32_t)m2, (int32_t)ja, (int32_t)jb});
    }
};

// cap: the engine's chunk capacity (LwsRect::cap)
inline std::unique_ptr<LwsPlan> lws_plan_build(const int64_t *key, int64_t cap, hipStream_t s)
{
    std::unique_ptr<LwsPlan> P(new LwsPlan());
    memcpy(P->key, key, sizeof(P->key));
    const int64_t rlo = key[0], rhi = key[1], lo = key[2], hi = key[3];
    LwsPlanSink sink;
    sink.scan_cells = key[5]; sink.scan_cols = key[6];
    const LwsTriStairs st{lo, hi};
    stair_decompose(st, sink, key[4], lo, hi, rlo, rhi);
    auto add_rows = [&](const std::vector<LwsRectD> &v, LwsPlan::Rows &R) {
        R.rd = (int64_t)P->hrd.size(); R.nr = (int64_t)v.size(); R.pre = (int64_t)P->hpre.size();
        int64_t run = 0;
        for (const LwsRectD &x : v) { P->hpre.push_back((int32_t)run); run += x.m; }
        P->hpre.push_back((int32_t)run);
        R.rows = run;
        P->hrd.insert(P->hrd.end(), v.begin(), v.end());
    };
    for (const LwsPlanSink::Lists &L : sink.d) {
        LwsPlan::Depth D;
        D.rd = (int64_t)P->hrd.size(); D.nr = (int64_t)L.big.size();
        P->hrd.insert(P->hrd.end(), L.big.begin(), L.big.end());
        int64_t hmax = 0;
        for (const LwsRectD &x : L.big) { int64_t h = 1; while (2 * h <= x.m) h *= 2; hmax = std::max(hmax, h); }
        for (int64_t h = hmax; h >= 1; h /= 2) {                       // rows h - 1 (+ 2h u) of every rectangle with m >= h
            LwsPlan::Level lv;
            lv.h = h; lv.pre = (int64_t)P->hpre.size();
            int64_t cnt = 0, chunks = 0;
            for (const LwsRectD &x : L.big) {
                P->hpre.push_back((int32_t)cnt);
                const int64_t c = lws_level_rows(x.m, h);
                cnt += c;
                if (c > 0) chunks += lws_level_chunks((int64_t)x.jb - x.ja + 1, c);
            }
            P->hpre.push_back((int32_t)cnt);
            lv.cnt = cnt; lv.cap = std::min(cap, chunks);
            D.levels.push_back(lv);
        }
        add_rows(L.small, D.small);
        add_rows(L.stair, D.stair);
        P->depths.push_back(std::move(D));
    }
    P->rd.alloc(std::max<size_t>(P->hrd.size(), 1)); P->pre.alloc(std::max<size_t>(P->hpre.size(), 1));
    if (!P->hrd.empty()) CP_HIP(hipMemcpyAsync(P->rd.p, P->hrd.data(), sizeof(LwsRectD) * P->hrd.size(), hipMemcpyHostToDevice, s));
    if (!P->hpre.empty()) CP_HIP(hipMemcpyAsync(P->pre.p, P->hpre.data(), sizeof(int32_t) * P->hpre.size(), hipMemcpyHostToDevice, s));
    return P;
}

// the plans a caller keeps: a K-layer run has two geometries, the full layers and the last row
struct LwsPlanCache {
    std::vector<std::unique_ptr<LwsPlan>> plans;
    const LwsPlan &get(const int64_t *key, int64_t cap, hipStream_t s)
    {
        for (const auto &P : plans) if (!memcmp(P->key, key, sizeof(P->key))) return *P;
        if (plans.size() >= 8) {                 // (plans of other option settings: wait for the launches that read them, then drop them)
            CP_HIP(hipStreamSynchronize(s));
            plans.clear();
        }
        plans.push_back(lws_plan_build(key, cap, s));
        return *plans.back();
    }
    // the batched launches of one layer on the engine E (whose argument block is set)
    template <typename ENGINE> void run(ENGINE &E, const LwsPlan &P) const
    {
        for (const LwsPlan::Depth &D : P.depths) {
            for (const LwsPlan::Level &lv : D.levels) {
                const LwsBatch B{P.rd.p + D.rd, P.pre.p + lv.pre, D.nr, lv.h, lv.cnt, lv.cap};
                E.level(B);
            }
            E.rows(P.rd.p + D.small.rd, P.pre.p + D.small.pre, D.small.nr, D.small.rows);
            E.rows(P.rd.p + D.stair.rd, P.pre.p + D.stair.pre, D.stair.nr, D.stair.rows);
        }
    }
};

}  // namespace cpk
