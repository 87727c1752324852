"""GPU tests of the plaid edge-cut models (kinds 13 / 14): oracle, Step, objective and bound entry points, the four Bisect
splitters, the K-part DP by the candidate sweep and by the prefix-min scan, its tables, and the plaid caller -- bit for bit
against tests/plaid_cut_model.py (definitions and the reference's loops in pure Python).

Shapes: empty columns and one column of 400 entries (longer than a 256-thread block); n + 1 in 1023, 1024, 1025 (one tile of the
scan, and the first size with a second level); n + 1 just above 1024 * 1024 (more block aggregates than the second level holds in
one strip); a MapPartition in no order with an empty part."""
import contextlib
import functools

import numpy as np
import pytest

import plaid_cut_model as pc
from util import cp, sprand, suitesparse_shaped

pytestmark = pytest.mark.gpu
PRIM, SEC = cp.AffinePrimaryEdgeCutModel, cp.AffineSecondaryEdgeCutModel


def _from_dense(D):
    m, n = D.shape
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


@functools.lru_cache(maxsize=None)
def pattern(m, n, seed, dens=0.08):
    """seeded pattern with empty columns and one full column"""
    rng = np.random.default_rng(seed)
    D = rng.random((m, n)) < dens
    D[:, rng.random(n) < 0.3] = False
    D[:, n // 3] = True
    return _from_dense(D)


def split(seed, n, K):
    rng = np.random.default_rng(seed)
    return cp.SplitPartition(K, np.concatenate([[1], np.sort(rng.integers(1, n + 2, K - 1)), [n + 1]]).astype(np.int64))


def scattered(seed, m, K, empty):
    """a MapPartition in no order whose part `empty` owns nothing"""
    asg = np.random.default_rng(seed).integers(1, K + 1, m)
    asg[asg == empty] = 1
    return cp.MapPartition(K, asg.astype(np.int64))


@contextlib.contextmanager
def force_brute(hip):
    hip.set_option("force_brute", 1)
    try:
        yield
    finally:
        hip.set_option("force_brute", 0)


def scan_layers(hip, call):
    hip.set_option("stat_reset", 0)
    out = call()
    return out, hip.get_stat("cut_scan_layers")


def dyn(hip, A, K, mdl, Pi, total=True):
    return cp.partition_stripe(A, K, (cp.DynamicTotalSplitter if total else cp.DynamicBottleneckSplitter)(mdl), Pi, backend=hip).spl


MODELS = [PRIM(3, 2, 1, 7), SEC(3, 2, 9, 4), PRIM(1.0, 2.0, 3.0, 4.0), SEC(0.0, 1.0, 2.0, 6.0), PRIM(0.1, 0.3, 0.7, 1.1), SEC(0.25, 0.1, 1.7, 0.9),
          PRIM(0, 1, 2, 5, alpha_k=[4, 0, 9, 1, 7]), SEC(0.5, 1.0, 2.0, 5.0, alpha_k=[4.0, 0.5, 9.0, 1.0, 7.0])]


def is_sec(mdl):
    return isinstance(mdl, SEC)


# ---------------------------------------------------------------- oracle / step / objective / bounds
@pytest.mark.parametrize("mi", range(len(MODELS)))
def test_eval_step_objective_bounds(hip, mi):
    mdl = MODELS[mi]
    A = pattern(400, 60, 1)
    n = A.n
    parts = [split(2, A.m, 5)] + ([] if is_sec(mdl) else [scattered(3, A.m, 5, 3)])
    a, b = np.meshgrid(np.arange(1, n + 2), np.arange(1, n + 2), indexing="ij")
    keep = a <= b
    j, jp = a[keep].astype(np.int64), b[keep].astype(np.int64)
    for Pi in parts:
        C = pc.Cut(A, Pi, mdl)
        ocl = cp.oracle_stripe(cp.StepHint(), mdl, A, Pi, backend=hip)
        for k in (1, 3, 5):
            assert np.array_equal(ocl(j, jp, k), C.table(k)[j - 1, jp - 1]), (mi, k)
        moves = [(cp.Jump(5), cp.Jump(20), 2), (cp.Same(5), cp.Next(21), 2), (cp.Next(6), cp.Same(21), 2), (cp.Prev(5), cp.Prev(20), 4),
                 (cp.Jump(1), cp.Jump(n + 1), 5)]
        want = [C.f(m[0].arg, m[1].arg, m[2]) for m in moves]
        assert cp.Step(ocl).walk(moves).tolist() == want
        for K in (1, 3, 5):
            Phi = split(10 + K, n, K)
            assert cp.total_value(A, Phi, mdl, Pi, backend=hip) == pc.objective(C, Phi.spl, "sum")
            assert cp.bottleneck_value(A, Phi, mdl, Pi, backend=hip) == pc.objective(C, Phi.spl, "max")
            if is_sec(mdl):
                assert cp.bound_stripe(A, K, mdl, Pi, backend=hip) == pc.bound_secondary_model(A, K, Pi, mdl)
            else:
                assert cp.bound_stripe(A, K, mdl, Pi, backend=hip) == cp.bound_stripe(A, K, mdl, backend=hip) == pc.bound_primary(A, K, mdl)


# ---------------------------------------------------------------- the Bisect splitters (they start from the oracle form of the bound)
@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("mdl", [PRIM(1, 1, 2, 3), SEC(1, 1, 1, 4), SEC(1, 2, 5, 2), PRIM(0.5, 0.25, 1.5, 2.75)], ids=["prim", "sec_lt", "sec_gt", "prim_f64"])
def test_bisect_splitters_match_the_reference_loops(hip, K, mdl):
    A = pattern(90, 70, 4)
    Pi = split(5, A.m, 7)
    C = pc.Cut(A, Pi, mdl)
    lo, hi = pc.bisect_bounds(C, K)
    for flip in (0, 1):
        for eps in (0.1, 0.001):
            meth = (cp.FlipBisectCostBottleneckSplitter if flip else cp.BisectCostBottleneckSplitter)(mdl, eps)
            got = cp.partition_stripe(A, K, meth, Pi, backend=hip).spl
            assert np.array_equal(got, pc.bisect_cost(C.f, A.n, K, eps, lo, hi, flip)), (flip, eps)
        meth = (cp.FlipBisectIndexBottleneckSplitter if flip else cp.BisectIndexBottleneckSplitter)(mdl)
        got = cp.partition_stripe(A, K, meth, Pi, backend=hip).spl
        assert np.array_equal(got, pc.bisect_index(C.f, A.n, K, lo, hi, flip)), flip


@pytest.mark.parametrize("mdl,K,flip,eps", [(SEC(1, 0, 3, 2), 2, 0, 0.1), (SEC(1, 0, 3, 2), 3, 0, 0.01), (SEC(1, 1, 1, 4), 2, 1, 0.01), (SEC(1, 1, 1, 4), 3, 1, 0.1)],
                         ids=["self_gt_cut_K2", "self_gt_cut_K3", "parts_1_to_K_K2", "parts_1_to_K_K3"])
def test_bisect_cost_starts_from_the_oracle_form_of_the_secondary_bound(hip, mdl, K, flip, eps):
    """cases where the model form (all parts of Pi, b_self_pin below, b_cut_pin above) and the oracle form (parts 1..K, min / max of
    the two betas) lead BisectCost to different split vectors: the device must give the oracle form's"""
    A = pattern(90, 70, 4)
    Pi = split(6, A.m, 7)
    C = pc.Cut(A, Pi, mdl)
    bo, bm = pc.bound_secondary_oracle(A, K, Pi, mdl), pc.bound_secondary_model(A, K, Pi, mdl)
    want = pc.bisect_cost(C.f, A.n, K, eps, *bo, flip)
    assert bo != bm and not np.array_equal(want, pc.bisect_cost(C.f, A.n, K, eps, *bm, flip))
    meth = (cp.FlipBisectCostBottleneckSplitter if flip else cp.BisectCostBottleneckSplitter)(mdl, eps)
    assert np.array_equal(cp.partition_stripe(A, K, meth, Pi, backend=hip).spl, want)
    assert cp.bound_stripe(A, K, mdl, Pi, backend=hip) == bm                     # (what bound_stripe itself returns is the model form)


# ---------------------------------------------------------------- the DP: sweep
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_sweep_matches_the_literal_dp(hip, K):
    A = pattern(120, 200, 6, 0.05)
    Pi = split(7, A.m, 8)
    for mdl in (PRIM(3, 2, 1, 7), SEC(3, 2, 9, 4), PRIM(2, -1, 5, -3), PRIM(0.1, 0.3, 0.7, 1.1), SEC(0.25, 0.1, 1.7, 0.9)):
        C = pc.Cut(A, Pi, mdl)
        integral = mdl.dtype == cp.models.CP_I64
        for total in (True, False):
            want = pc.dp(C, K, "sum" if total else "max")[0]
            if integral and total:
                with force_brute(hip):
                    got, layers = scan_layers(hip, lambda: dyn(hip, A, K, mdl, Pi, total))
            else:
                got, layers = scan_layers(hip, lambda: dyn(hip, A, K, mdl, Pi, total))
            assert layers == 0
            assert np.array_equal(got, want), (type(mdl).__name__, mdl._params(), total)


# ---------------------------------------------------------------- the DP: scan
SCAN_MODELS = [PRIM(3, 2, 1, 7), SEC(3, 2, 9, 4), PRIM(1, 0, 0, 0), SEC(1, 0, 0, 0), PRIM(2, -1, 5, -3), PRIM(1.0, 2.0, 3.0, 4.0),
               SEC(0.0, 1.0, 2.0, 6.0), PRIM(0, 1, 2, 5, alpha_k=[4, 0, 9, 1, 7, 3, 3, 8]), SEC(0, 1, 5, 2, alpha_k=[4, 0, 9, 1, 7, 3, 3, 8])]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_scan_matches_the_literal_dp(hip, K):
    A = pattern(150, 300, 8, 0.04)
    few = _from_dense(np.pad(np.random.default_rng(9).random((150, 5)) < 0.3, ((0, 0), (100, 195))))      # 5 columns that can hold entries
    for B in (A, few):
        parts = [split(11, B.m, 8), scattered(12, B.m, 9, 4)]
        for mdl in SCAN_MODELS:
            for Pi in parts[:1] if is_sec(mdl) else parts:
                want = pc.dp(pc.Cut(B, Pi, mdl), K, "sum")[0]
                got, layers = scan_layers(hip, lambda: dyn(hip, B, K, mdl, Pi))
                assert layers == K - 1
                assert np.array_equal(got, want), (type(mdl).__name__, mdl._params())


def test_int64_bound_past_2_60_takes_the_sweep(hip):
    A = pattern(60, 90, 13)
    Pi = split(14, A.m, 8)
    mdl = PRIM(2 ** 58, 0, 1, 3)                                   # K * alpha = 2^61
    got, layers = scan_layers(hip, lambda: dyn(hip, A, 8, mdl, Pi))
    assert layers == 0
    assert np.array_equal(got, pc.dp(pc.Cut(A, Pi, mdl), 8, "sum")[0])
    got, layers = scan_layers(hip, lambda: dyn(hip, A, 3, mdl, Pi))      # 3 * 2^58 + ... stays below 2^60
    assert layers == 2
    assert np.array_equal(got, pc.dp(pc.Cut(A, Pi, mdl), 3, "sum")[0])


@pytest.mark.parametrize("n", [1022, 1023, 1024, 2047, 2048, 20011])
def test_scan_matches_the_sweep(hip, n):
    """n + 1 one below, at and one above the scan's tile of 1024 values -- the second level starts with the second tile -- around
    two tiles, and one pattern of many tiles"""
    A = suitesparse_shaped(n, 6, 21, m=500)
    K = 8 if n > 10000 else 5
    parts = [split(22, A.m, 8), scattered(23, A.m, 8, 2)]
    for mdl in (PRIM(3, 2, 1, 7), SEC(3, 2, 9, 4), PRIM(1, 0, 0, 0), PRIM(0.0, 1.0, 2.0, 6.0), SEC(0, 1, 5, 2, alpha_k=[4, 0, 9, 1, 7, 3, 3, 8])):
        for Pi in parts[:1] if is_sec(mdl) else parts:
            got, layers = scan_layers(hip, lambda: dyn(hip, A, K, mdl, Pi))
            assert layers == K - 1
            with force_brute(hip):
                want, layers = scan_layers(hip, lambda: dyn(hip, A, K, mdl, Pi))
            assert layers == 0
            assert np.array_equal(got, want), (n, type(mdl).__name__, mdl._params())


def test_scan_with_more_tiles_than_one_strip_of_the_second_level(hip):
    """n + 1 > 1024 * 1024: the block aggregates are scanned in two strips with a carry.  The sweep cannot run here; the scan
    restated in numpy is the check."""
    n, m = 1024 * 1024 + 2, 1000
    rng = np.random.default_rng(31)
    rows = np.stack([rng.integers(1, m // 2 + 1, n), m // 2 + rng.integers(1, m // 2 + 1, n)], axis=1).reshape(-1)
    A = cp.SparseMatrixCSC(m, n, 1 + 2 * np.arange(n + 1, dtype=np.int64), rows.astype(np.int64))
    Pi = scattered(32, m, 4, 3)
    for mdl in (PRIM(5, 1, 1, 3), PRIM(1, 0, 0, 0)):
        got, layers = scan_layers(hip, lambda: dyn(hip, A, 3, mdl, Pi))
        assert layers == 2
        assert np.array_equal(got, pc.dp_scan(A, Pi, mdl, 3)[0])


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("total", [True, False])
def test_dynamic_tables_match_the_literal_dp(hip, total):
    A = pattern(80, 100, 15)
    Pi = split(16, A.m, 4)
    K = 4
    rp, keep = cp.api._rowpart(Pi)
    for mdl in (PRIM(3, 2, 1, 7), SEC(3, 2, 9, 4), PRIM(0.1, 0.3, 0.7, 1.1)):
        _, csts, ptrs = pc.dp(pc.Cut(A, Pi, mdl), K, "sum" if total else "max")
        rc, ptr, cst = hip.dynamic_tables(A, K, 0 if total else 1, mdl.marshal(), rp)
        assert rc == 0
        for k in range(K):
            rows = slice(A.n, A.n + 1) if k == K - 1 else slice(0, A.n + 1)      # layer K: row n + 1 only
            assert np.array_equal(ptr[rows, k], ptrs[k][rows] + 1), (k, type(mdl).__name__)
            assert np.array_equal(cst[rows, k], csts[k][rows]), (k, type(mdl).__name__)
        assert np.all(ptr[:A.n, K - 1] == 0)


# ---------------------------------------------------------------- two independent counters
def test_primary_with_one_partition_agrees_with_kind_12_on_the_device(hip):
    A = sprand(130, 130, 0.06, np.random.default_rng(17))
    for K in (1, 3, 6):
        Phi = split(18 + K, A.n, K)
        for p in ((0, 0, 0, 1), (0, 0, 1, 1), (1, 1, 1, 1), (2, 1, 7, 3), (0.5, 0.1, 1.7, 0.9)):
            for val in (cp.bottleneck_value, cp.total_value):
                assert val(A, Phi, PRIM(*p), Phi, backend=hip) == val(A, Phi, cp.AffineSymmetricEdgeCutModel(*p), backend=hip)


# ---------------------------------------------------------------- the plaid caller, refusals
def test_partition_plaid_alternation(hip):
    A = sprand(150, 150, 0.05, np.random.default_rng(19))
    K = 4
    work, sec, prim = cp.AffineWorkModel(2, 1, 3), SEC(1, 1, 2, 6), PRIM(1, 1, 2, 6)
    meth = cp.AlternatingPartitioner(cp.DynamicTotalSplitter(work), cp.DynamicTotalSplitter(sec), cp.DynamicTotalSplitter(prim))
    Pi, Phi = cp.partition_plaid(A, K, meth, backend=hip)
    # the same alternation through the checker; the work cost is the edge-cut cost with both pin prices equal, under any Pi
    T = cp.adjointpattern(A, backend=hip)
    one = cp.SplitPartition(K, [1] + [A.m + 1] * K)                    # (K parts, the first owns every row)
    phi = cp.SplitPartition(K, pc.dp(pc.Cut(A, one, PRIM(2, 1, 3, 3)), K, "sum")[0])
    pi = cp.SplitPartition(K, pc.dp(pc.Cut(T, phi, sec), K, "sum")[0])
    phi = cp.SplitPartition(K, pc.dp(pc.Cut(A, pi, prim), K, "sum")[0])
    assert np.array_equal(Pi.spl, pi.spl) and np.array_equal(Phi.spl, phi.spl)


def test_refusals(hip):
    A = pattern(40, 30, 20)
    Pi = split(21, A.m, 3)
    prim, sec = PRIM(1, 1, 2, 3), SEC(1, 1, 2, 3)
    for mdl in (prim, sec):
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(cp.ConstrainedCost(mdl, cp.VertexCount(), 20)), Pi, backend=hip)
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, 2, cp.DynamicTotalChunker(mdl), Pi, backend=hip)
        with pytest.raises(AssertionError):
            cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(mdl), None, backend=hip)
        with pytest.raises(AssertionError):
            cp.partition_stripe(A, 2, cp.BisectCostBottleneckSplitter(mdl, 0.1), None, backend=hip)
        with pytest.raises(AssertionError):                                       # (the reference asserts on models that are not connectivity models)
            cp.partition_stripe(A, 2, cp.LazyBisectCostBottleneckSplitter(mdl, 0.1), backend=hip)
    for mdl in (sec, prim):                                                       # K > Pi.K: part K is no part of Pi, for either model
        for meth in (cp.DynamicTotalSplitter(mdl), cp.DynamicBottleneckSplitter(mdl), cp.BisectCostBottleneckSplitter(mdl, 0.1),
                     cp.FlipBisectIndexBottleneckSplitter(mdl)):
            with pytest.raises(AssertionError):
                cp.partition_stripe(A, 4, meth, Pi, backend=hip)
        with pytest.raises(AssertionError):
            cp.oracle_stripe(cp.NoHint(), mdl, A, Pi, backend=hip)(1, 2, 4)
    with pytest.raises(AssertionError):
        cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(sec), scattered(22, A.m, 3, 2), backend=hip)      # no SplitPartition
    for mdl in (PRIM(1, 1, -2, 3), SEC(1, -1, 2, 3), SEC(1.0, 1.0, 2.0, -0.5)):
        with pytest.raises(AssertionError):
            cp.bound_stripe(A, 2, mdl, Pi, backend=hip)
    with pytest.raises(NotImplementedError):
        cp.bound_stripe(A, 2, sec, backend=hip)                                   # the reference has no method without Pi
