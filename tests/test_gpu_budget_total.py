"""GPU parity of the total-cost DP under a pin- or work-weighted part budget on the two-staircase divide and conquer of
csrc/dp_total_budget.hip: DynamicTotal{Splitter,Chunker}(ConstrainedCost(f, AffineWorkModel(alpha, b_v, b_p), w_max)).  Tables
bit-exact against the oracle's literal sweep in both cost types, at default thresholds and with the thresholds shrunk so that small
matrices run rectangles, levels and stair scans; sizes that engage the default thresholds; the one-wave literal kernel as a second
opinion; routing of every pair outside the gate; and a sanity run at n = 2 * 10^5."""
import contextlib
import functools
import math

import numpy as np
import pytest

from util import cp, suitesparse_shaped
from test_gpu_bottleneck import WEIGHTS, mats

pytestmark = pytest.mark.gpu

MODELS = [cp.AffineConnectivityModel(0, 0, 0, 1), cp.AffineConnectivityModel(0, 3, 1, 3), cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0),
          cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[5, 1, 9, 2, 7, 3, 8, 4]), cp.AffineWorkModel(-3, 1, 0),
          cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3)]
PINS = cp.AffineWorkModel(0, 0, 1)
SHRUNK = {"budget_scan_cells": 8, "budget_scan_cols": 4, "budget_stair_cols": 4}
DEFAULT = {"budget_scan_cells": 1 << 20, "budget_scan_cols": 1024, "budget_stair_cols": 1024}


def prof(hip):
    """launches the profile slot of dp_total_budget.hip has seen since the last profiled() began"""
    return hip.prof_get()["dp_budget"]["launches"]


@contextlib.contextmanager
def profiled(hip):
    hip.prof_reset(); hip.prof_enable(True)
    try:
        yield
    finally:
        hip.prof_enable(False)


@functools.lru_cache(maxsize=None)
def matrices():
    """that file's matrices, built once: every case of every parameter runs on the same objects (and device handles)"""
    return tuple(mats())


def cases(wgt):
    """(A, K, wmax): the budget fractions {1/K, 1.5/K, 0.5, 1, 0} of the whole weight, as tests/test_gpu_bottleneck.py draws them"""
    a0, bv, bp = wgt._params()
    for A in matrices():
        for K in (1, 2, 5, 8):
            full = a0 + bv * A.n + bp * A.nnz
            for frac in (1.0 / K, 1.5 / K, 0.5, 1.0, 0.0):
                wmax = a0 + (full - a0) * frac + (1 if frac else 0)
                yield A, K, (int(wmax) if wgt.dtype == cp.models.CP_I64 else float(wmax))


def methods(mdl):
    # (the chunker loop order passes no part index: the reference has no such call for a per-part alpha)
    return (cp.DynamicTotalSplitter,) if mdl.alpha_k is not None else (cp.DynamicTotalSplitter, cp.DynamicTotalChunker)


# what an oracle-only run of the 420 cases counts, per weight: (feasible cases whose split vector has more than two distinct entries,
# infeasible cases) -- the same for each of the six models
ORACLE_COUNTS = [(128, 136), (120, 173), (154, 100), (120, 173)]


@pytest.fixture(scope="module")
def references(orc):
    """the oracle's answers, computed once per (weight, model) and shared by the two threshold settings"""
    memo = {}

    def get(wi, mi):
        if (wi, mi) not in memo:
            wgt, mdl = WEIGHTS[wi], MODELS[mi]
            out = []
            for A, K, wmax in cases(wgt):
                tab = orc.dynamic_tables_constrained(A, K, 0, mdl.marshal(), None, wgt.marshal(), int(wmax), float(wmax))
                f = cp.ConstrainedCost(mdl, wgt, wmax)
                out.append((tab, [cp.partition_stripe(A, K, meth(f), backend=orc) for meth in methods(mdl)]))
            memo[(wi, mi)] = out
        return memo[(wi, mi)]
    return get


@pytest.mark.parametrize("opts", [DEFAULT, SHRUNK], ids=["default", "shrunk"])
@pytest.mark.parametrize("mi", range(len(MODELS)))
@pytest.mark.parametrize("wi", range(len(WEIGHTS)))
def test_budget_total_tables_bit_exact(hip, references, wi, mi, opts):
    """default thresholds, and 8 cells / 4 columns / 4 stair columns so that the n <= 2100 matrices run levels and stair scans"""
    wgt, mdl = WEIGHTS[wi], MODELS[mi]
    want_all = references(wi, mi)
    nondeg = infeasible = 0
    try:
        for name, v in opts.items():
            hip.set_option(name, v)
        hip.set_option("stat_reset", 0)
        for (A, K, wmax), (tab, parts) in zip(cases(wgt), want_all):
            rc2, lo2, hi2, p2, c2 = tab
            rc1, lo1, hi1, p1, c1 = hip.dynamic_tables_constrained(A, K, mdl.marshal(), wmax, combine=0, wm=wgt.marshal())
            assert rc1 == rc2, (A, K, wmax, hip.last_error())
            assert np.array_equal(lo1, lo2) and np.array_equal(hi1, hi2), (A, K, wmax)
            infeasible += rc2 != 0
            if rc2 == 0:
                assert np.array_equal(p1, p2), (A, K, wmax, wi, mi)
                assert np.array_equal(c1, c2), (A, K, wmax, wi, mi)
            f = cp.ConstrainedCost(mdl, wgt, wmax)
            for meth, want in zip(methods(mdl), parts):
                assert cp.partition_stripe(A, K, meth(f), backend=hip) == want, (A, K, wmax, wi, mi, meth.__name__)
            nondeg += int(rc2 == 0 and len(set(parts[0].spl.tolist())) > 2)
        assert hip.get_stat("budget_layers") > 0
    finally:
        for name, v in DEFAULT.items():
            hip.set_option(name, v)
    assert nondeg >= ORACLE_COUNTS[wi][0] and infeasible >= ORACLE_COUNTS[wi][1], (nondeg, infeasible)


def pins_per_part(A, part):
    pos = np.asarray(A.colptr, dtype=np.int64)
    spl = np.asarray(part.spl, dtype=np.int64)
    return pos[spl[1:] - 1] - pos[spl[:-1] - 1]


def test_default_thresholds_engaged(hip, orc):
    """windows of 3 100 - 3 600 columns at the looser budgets: past the 1024-column and 2^20-cell scan limits, so the level kernels and
    the recursion run as shipped"""
    mdl = cp.AffineConnectivityModel(0, 3, 1, 3)
    for (n, seed, K) in ((12000, 5, 5), (20000, 6, 6)):
        A = suitesparse_shaped(n, 8, seed)
        free = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=orc)
        for wgt, budget in ((PINS, int(1.02 * A.nnz / K)), (PINS, int(1.3 * A.nnz / K)), (cp.AffineWorkModel(0, 2, 1), int(1.005 * (2 * A.n + A.nnz) / K))):
            rc2, lo2, hi2, p2, c2 = orc.dynamic_tables_constrained(A, K, 0, mdl.marshal(), None, wgt.marshal(), budget, float(budget))
            with profiled(hip):
                rc1, lo1, hi1, p1, c1 = hip.dynamic_tables_constrained(A, K, mdl.marshal(), budget, combine=0, wm=wgt.marshal())
            assert rc1 == 0 and rc2 == 0, hip.last_error()
            assert prof(hip) > 0
            assert np.array_equal(lo1, lo2) and np.array_equal(hi1, hi2)
            assert np.array_equal(p1, p2) and np.array_equal(c1, c2), (n, budget)
            f = cp.ConstrainedCost(mdl, wgt, budget)
            got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
            assert got == cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=orc)
            if wgt is PINS:
                assert got != free                                      # the budget decides the answer
                assert pins_per_part(A, got).max() <= budget


@pytest.mark.parametrize("mdl", [cp.AffineConnectivityModel(0, 10, 1, 100), cp.AffineConnectivityModel(0.0, 10.0, 1.0, 100.0)], ids=["i64", "f64"])
def test_against_the_literal_kernel(hip, mdl):
    A = suitesparse_shaped(1500, 8, 5)
    K = 6
    budget = int(1.3 * A.nnz / K)
    f = cp.ConstrainedCost(mdl, PINS, budget)
    with profiled(hip):
        got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
    assert prof(hip) > 0
    rc, lo, hi, ptr, cst = hip.dynamic_tables_constrained(A, K, mdl.marshal(), budget, combine=0, wm=PINS.marshal())
    assert rc == 0
    hip.set_option("force_brute", 1)
    try:
        with profiled(hip):
            want = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
        assert prof(hip) == 0
    finally:
        hip.set_option("force_brute", 0)
    assert got == want and len(set(got.spl.tolist())) > 2
    assert cst[A.n, K - 1] == cp.total_value(A, got, mdl, backend=hip)


def test_routing(hip, orc):
    A = suitesparse_shaped(300, 6, 9)
    K = 4
    budget = int(1.3 * A.nnz / K)
    conn = cp.AffineConnectivityModel(0, 3, 1, 3)

    def run(f, expect_budget, option=None):
        hip.set_option("stat_reset", 0)
        if option:
            hip.set_option(*option)
        try:
            with profiled(hip):
                got = [cp.partition_stripe(A, K, meth(f), backend=hip) for meth in (cp.DynamicTotalSplitter, cp.DynamicTotalChunker)]
        finally:
            if option:
                hip.set_option(option[0], 1 - option[1])
        want = [cp.partition_stripe(A, K, meth(f), backend=orc) for meth in (cp.DynamicTotalSplitter, cp.DynamicTotalChunker)]
        assert got == want, f
        assert (prof(hip) > 0) == expect_budget and (hip.get_stat("budget_layers") > 0) == expect_budget, f
        return got[0]

    # admitted: both cost types, a work weight with a vertex term, a hyperedge-cut and a work cost
    for mdl in (conn, cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0), cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3), cp.AffineWorkModel(-3, 1, 0)):
        run(cp.ConstrainedCost(mdl, PINS, budget), True)
    run(cp.ConstrainedCost(conn, cp.AffineWorkModel(2, 3, 1), 2 + 3 * A.n // 3 + budget), True)
    run(cp.ConstrainedCost(conn, cp.AffineWorkModel(0.5, 0.0, 0.25), 0.5 + 0.25 * budget), True)
    # outside the gate: today's path, today's answers
    run(cp.ConstrainedCost(conn, PINS, budget), False, ("budget_total", 0))
    run(cp.ConstrainedCost(conn, PINS, budget), False, ("force_brute", 1))
    run(cp.ConstrainedCost(cp.ColumnBlockComponentCostModel(3, lambda x: 1 + x), PINS, budget), False)
    # (a per-part weight has no device form at all: the entry refuses it before any path is chosen, as it always has)
    hip.set_option("stat_reset", 0)
    with profiled(hip), pytest.raises(AssertionError, match="weight must be VertexCount or an AffineWorkModel"):
        cp.partition_stripe(A, K, cp.DynamicTotalSplitter(cp.ConstrainedCost(conn, cp.AffineWorkModel(0, 0, 1, alpha_k=[1, 0, 2, 0]), budget + 2)), backend=hip)
    assert prof(hip) == 0 and hip.get_stat("budget_layers") == 0
    run(cp.ConstrainedCost(cp.AffineConnectivityModel(0, 1 << 58, 1, 3), PINS, budget), False)
    run(cp.ConstrainedCost(cp.AffineConnectivityModel(0.5, 0.25, 0.0, 1.5), PINS, budget), False)
    # a width weight stays on the windowed dp_total path
    run(cp.ConstrainedCost(conn, cp.VertexCount(), A.n // 3), False)
    run(cp.ConstrainedCost(conn, cp.AffineWorkModel(0, 1, 0), A.n // 3), False)
    # an infeasible budget: the same return code and degenerate vector on both paths
    tight = int(A.nnz / K) - 50
    deg = run(cp.ConstrainedCost(conn, PINS, tight), False)
    assert deg.spl.tolist() == [1] * K + [A.n + 1]
    rcs = []
    for brute in (0, 1):
        hip.set_option("force_brute", brute)
        try:
            if brute == 0:
                rcs.append(hip.dynamic_tables_constrained(A, K, conn.marshal(), tight, combine=0, wm=PINS.marshal())[0])
            assert cp.partition_stripe(A, K, cp.DynamicTotalSplitter(cp.ConstrainedCost(conn, PINS, tight)), backend=hip) == deg
        finally:
            hip.set_option("force_brute", 0)
    assert rcs == [cp.models.CP_INFEASIBLE]


def test_scale_sanity(hip):
    """n = 2 * 10^5 on the bench generator: the optimum lies between the unconstrained optimum and any feasible partition's value"""
    A = suitesparse_shaped(200_000, 10, 1, nnz=2_000_000)
    K = 8
    mdl = cp.AffineConnectivityModel(0, 0, 0, 1)
    budget = math.ceil(1.3 * A.nnz / K)
    f = cp.ConstrainedCost(mdl, PINS, budget)
    with profiled(hip):
        got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
    assert prof(hip) > 0
    rc, lo, hi, ptr, cst = hip.dynamic_tables_constrained(A, K, mdl.marshal(), budget, combine=0, wm=PINS.marshal())
    assert rc == 0
    assert pins_per_part(A, got).max() <= budget
    total = cp.total_value(A, got, mdl, backend=hip)
    assert cst[A.n, K - 1] == total
    feasible = cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(f), backend=hip)
    assert pins_per_part(A, feasible).max() <= budget
    assert total <= cp.total_value(A, feasible, mdl, backend=hip)
    assert total >= cp.total_value(A, cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip), mdl, backend=hip)
