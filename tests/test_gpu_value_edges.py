"""GPU parity at the edges of the value range, where the fast paths' exactness gates decide.

Every fast path (O(n log^2 n) total DP, windowed DP, bottleneck valley search, (min,+) chunk scan) relies on exact arithmetic:
inverse-Monge or monotone costs and reassociated sums.  Julia's Int64 wraps and Float64 rounds above 2^53, and then none of
that holds; the reference still computes its literal recurrence on the wrapped / rounded values, and so does the oracle
(pinned against brute force under wrap by test_oracle_wrap.py).  So every entry point must either match the oracle bit for
bit or refuse: models whose reachable totals leave the exact range (model_exact_on, csrc/model.hpp) go to the literal
kernels, and with brute_max_n = 0 -- no literal sweep allowed -- the unconstrained DP must answer CP_EUNSUPPORTED for them
while a model just inside the bound still answers (so the routing is observable without a new statistic).
"""
import numpy as np
import pytest

from util import cp, sprand, golden_matrices

pytestmark = pytest.mark.gpu

EUNSUPPORTED = cp.models.CP_EUNSUPPORTED
I64 = cp.models.CP_I64
HYPER = cp.models.CP_MODEL_HYPEREDGE_CUT
DEFAULT_BRUTE_MAX_N = 200000


def mats():
    rng = np.random.default_rng(0xDEADBEEF)
    out = [sprand(m, n, p, rng) for (m, n, p) in [(3, 2, 0.5), (5, 7, 0.4), (8, 16, 0.3), (10, 23, 0.2), (6, 33, 0.3), (20, 40, 0.1),
                                                  (9, 64, 0.2), (9, 65, 0.2), (40, 100, 0.05)]]
    return out + [golden_matrices()["LPnetlib/lpi_itest6"], golden_matrices()["HB/can_292"]]


MATS = mats()


def params(mdl):
    a, bv, bp = mdl.alpha, mdl.beta_vertex, mdl.beta_pin
    bn = max(abs(getattr(mdl, "beta_net", 0)), abs(getattr(mdl, "beta_self_net", 0)), abs(getattr(mdl, "beta_cut_net", 0)))
    amax = max([abs(a)] + [abs(x) for x in (getattr(mdl, "alpha_k", None) or [])])
    return amax, abs(bv), abs(bp), bn


def reach(mdl, A, K):
    """the largest reachable |total| of a K-part partition, as model_exact_on bounds it"""
    amax, bv, bp, bn = params(mdl)
    return amax * max(K, 1) + bv * A.n + (bp + bn) * A.nnz


def exact_on(mdl, A, K):
    if mdl.dtype == I64:
        return reach(mdl, A, K) < 2 ** 60
    vals = list(mdl._params()) + list(getattr(mdl, "alpha_k", None) or [])
    return all(float(v).is_integer() and abs(v) <= 9e15 for v in vals) and reach(mdl, A, K) < 2 ** 53


def fast_sum(mdl, A, K):          # every model here is inside the inverse-Monge class but for its magnitude
    return exact_on(mdl, A, K) and (mdl.kind != HYPER or mdl.beta_self_net <= mdl.beta_cut_net)


def fast_max(mdl, A, K):          # ... and monotone when b_self >= b_cut
    if mdl.kind == HYPER and mdl.beta_self_net < mdl.beta_cut_net:
        return False
    return exact_on(mdl, A, K) or (mdl.dtype != I64 and mdl.kind != HYPER)


def i64_wrap():
    return [cp.AffineConnectivityModel(0, 1, 1, 3 * 2 ** 61), cp.AffineConnectivityModel(0, 1, 1, 2 ** 62 + 99),
            cp.AffineWorkModel(0, 1, 2 ** 62 + 1),
            cp.AffineHyperedgeCutModel(0, 1, 1, 2 ** 62 + 5, 2 ** 61 + 3),      # b_self >= b_cut: the bottleneck's class
            cp.AffineHyperedgeCutModel(0, 1, 1, 2 ** 61 + 3, 2 ** 62 + 5),      # b_self <= b_cut: the total's class
            cp.AffineConnectivityModel(0, 1, 1, 5, alpha_k=[2 ** 62, -2 ** 62, 3, 2 ** 62 + 1, -2 ** 62 - 7, 2 ** 62 - 1, 11, -2 ** 62])]


def i64_inside(A, K):
    """Connectivity / Work models whose reachable total is just under 2^60 on A (the largest b_net / b_pin that fits)"""
    N = max(A.nnz, 1)
    bn = (2 ** 60 - 1 - 3 * K - A.n - A.nnz) // N
    bp = (2 ** 60 - 1 - 3 * K - A.n) // N
    out = [cp.AffineConnectivityModel(3, 1, 1, bn), cp.AffineWorkModel(3, 1, bp)]
    assert all(exact_on(m, A, K) for m in out)
    if A.nnz:
        assert not exact_on(cp.AffineConnectivityModel(3, 1, 1, bn + 1), A, K) and not exact_on(cp.AffineWorkModel(3, 1, bp + 1), A, K)
    return out


def f64_edge(A, K):
    """integral Float64 Connectivity models with odd b_net just under and just over the 2^53 bound, and one whose products
    round (b_net = 2^52 + 1: 3 * b_net needs 54 bits)"""
    N = max(A.nnz, 1)
    room = 2 ** 53 - 1 - 3 * K - A.n - A.nnz
    under = room // N
    under -= 1 - under % 2                      # odd, still under
    over = under + 2
    out = [cp.AffineConnectivityModel(3.0, 1.0, 1.0, float(under)), cp.AffineConnectivityModel(3.0, 1.0, 1.0, float(over)),
           cp.AffineConnectivityModel(0.0, 1.0, 1.0, float(2 ** 52 + 1)),
           cp.AffineHyperedgeCutModel(3.0, 1.0, 1.0, float(under), float(under)), cp.AffineHyperedgeCutModel(3.0, 1.0, 1.0, float(over), float(over))]
    assert exact_on(out[0], A, K) and not exact_on(out[1], A, K)
    return out


NONDYADIC = [cp.AffineConnectivityModel(0.1, 0.7, 0.3, 1.3), cp.AffineWorkModel(0.1, 0.7, 0.3),
             cp.AffineConnectivityModel(0.1, 0.7, 0.3, 1.3, alpha_k=[0.1, 2.7, 0.3, 1.9, 0.7, 3.1, 0.2, 0.9]),
             cp.AffineHyperedgeCutModel(0.3, 0.1, 0.0, 0.3, 0.3)]


class brute_max_n:
    """set_option("brute_max_n", v) for a block, restored in finally"""

    def __init__(self, hip, v):
        self.hip, self.v = hip, v

    def __enter__(self):
        assert self.hip.set_option("brute_max_n", self.v) == 0

    def __exit__(self, *a):
        self.hip.set_option("brute_max_n", DEFAULT_BRUTE_MAX_N)


def outcome(f):
    """the split vector, or the exception type (wrapped costs may violate a bisection's precondition on both sides)"""
    try:
        return tuple(f().spl.tolist())
    except (AssertionError, NotImplementedError) as e:
        return type(e).__name__


def tables_case(hip, orc, A, K, g, mdl):
    mm = mdl.marshal()
    rc2, p2, c2 = orc.dynamic_tables(A, K, g, mm, None)
    assert rc2 == 0
    rc1, p1, c1 = hip.dynamic_tables(A, K, g, mm, None)
    assert rc1 == 0, hip.last_error()
    assert np.array_equal(p1, p2), (A, K, g, mdl.kind, mdl._params())
    assert np.array_equal(c1, c2), (A, K, g, mdl.kind, mdl._params())
    fast = fast_sum(mdl, A, K) if g == 0 else fast_max(mdl, A, K)
    with brute_max_n(hip, 0):
        rc1, p1, c1 = hip.dynamic_tables(A, K, g, mm, None)
        if fast:
            assert rc1 == 0, (A, K, g, mdl._params(), hip.last_error())
            assert np.array_equal(p1, p2) and np.array_equal(c1, c2), (A, K, g, mdl._params())
        else:
            assert rc1 == EUNSUPPORTED, (A, K, g, mdl._params(), rc1)
            meth = (cp.DynamicTotalSplitter if g == 0 else cp.DynamicBottleneckSplitter)(mdl)
            with pytest.raises(NotImplementedError):
                cp.partition_stripe(A, K, meth, backend=hip)
    return fast


def splitter_cases(hip, orc, A, K, mdl):
    """unconstrained and width-constrained Dynamic{Total,Bottleneck}Splitter / Chunker, at the default brute_max_n and at 0
    (the constrained literal kernel has no size gate: it must answer in both)"""
    for lim in (DEFAULT_BRUTE_MAX_N, 0):
        with brute_max_n(hip, lim):
            for w in sorted({max(1, -(-A.n // K)), max(1, -(-3 * A.n // (2 * K)))}):
                fc = cp.ConstrainedCost(mdl, cp.VertexCount(), w)
                for meth in (cp.DynamicTotalSplitter(fc), cp.DynamicBottleneckSplitter(fc), cp.DynamicTotalChunker(fc)):
                    want = outcome(lambda: cp.partition_stripe(A, K, meth, backend=orc))
                    got = outcome(lambda: cp.partition_stripe(A, K, meth, backend=hip))
                    assert got == want, (A, K, w, lim, type(meth).__name__, mdl._params())
            if lim:
                for meth in (cp.DynamicTotalSplitter(mdl), cp.DynamicBottleneckSplitter(mdl), cp.DynamicTotalChunker(mdl)):
                    assert cp.partition_stripe(A, K, meth, backend=hip) == cp.partition_stripe(A, K, meth, backend=orc), \
                        (A, K, type(meth).__name__, mdl._params())


def windowed_tables_case(hip, orc, A, K, mdl, combine, wm=None, wmax=None):
    """cp_dynamic_tables_constrained: the tables of the windowed path, or CP_EUNSUPPORTED where it must not be taken"""
    w = wmax if wmax is not None else max(1, -(-3 * A.n // (2 * K)))
    mm = mdl.marshal()
    rc2, lo2, hi2, p2, c2 = orc.dynamic_tables_constrained(A, K, combine, mm, None, (wm or cp.VertexCount()).marshal(), int(w), float(w))
    rc1, lo1, hi1, p1, c1 = hip.dynamic_tables_constrained(A, K, mm, w, combine=combine, wm=wm.marshal() if wm else None)
    takes = fast_sum(mdl, A, K) if combine == 0 else (mdl.dtype == I64 and fast_max(mdl, A, K))
    if not takes:
        assert rc1 == EUNSUPPORTED, (A, K, combine, mdl._params(), rc1)
        return
    assert rc1 == rc2, (A, K, combine, mdl._params(), hip.last_error())
    if rc2 == 0:
        assert np.array_equal(lo1, lo2) and np.array_equal(hi1, hi2)
        assert np.array_equal(p1, p2), (A, K, combine, mdl._params())
        assert np.array_equal(c1, c2), (A, K, combine, mdl._params())


def chunker_cases(hip, orc, A, mdl):
    for w in (1, 3, 8, 16):
        fc = cp.ConstrainedCost(mdl, cp.VertexCount(), w)
        want = cp.pack_stripe(A, cp.DynamicTotalChunker(fc), backend=orc)
        assert cp.pack_stripe(A, cp.DynamicTotalChunker(fc), backend=hip) == want, (A, w, mdl._params(), "scan")
        assert cp.pack_stripe(A, cp.ConvexTotalChunker(fc), backend=hip) == cp.pack_stripe(A, cp.ConvexTotalChunker(fc), backend=orc), \
            (A, w, mdl._params(), "convex")
    for meth in (cp.ConvexTotalChunker(mdl), cp.DynamicTotalChunker(mdl)):
        assert cp.pack_stripe(A, meth, backend=hip) == cp.pack_stripe(A, meth, backend=orc), (A, type(meth).__name__, mdl._params())


def bisect_cases(hip, orc, A, mdl):
    for K in (2, 5):
        meths = [cp.BisectCostBottleneckSplitter(mdl, 0.1), cp.BisectCostBottleneckSplitter(mdl, 0.01), cp.BisectIndexBottleneckSplitter(mdl)]
        if mdl.kind == cp.models.CP_MODEL_CONNECTIVITY and getattr(mdl, "alpha_k", None) is None:
            meths.append(cp.LazyBisectCostBottleneckSplitter(mdl, 0.01))
        for meth in meths:
            want = outcome(lambda: cp.partition_stripe(A, K, meth, backend=orc))
            got = outcome(lambda: cp.partition_stripe(A, K, meth, backend=hip))
            assert got == want, (A, K, type(meth).__name__, mdl._params())


# ---------------------------------------------------------------- Int64 wrap

@pytest.mark.parametrize("mi", range(6))
def test_int64_wrap_dynamic_tables(hip, orc, mi):
    mdl = i64_wrap()[mi]
    refused = 0
    for A in MATS:
        for K in (1, 2, 5):
            for g in (0, 1):
                refused += not tables_case(hip, orc, A, K, g, mdl)
    assert refused > 0          # the wrapped model is refused by the fast paths somewhere (every matrix with a pin)


@pytest.mark.parametrize("mi", range(6))
def test_int64_wrap_splitters_and_windowed_tables(hip, orc, mi):
    mdl = i64_wrap()[mi]
    for A in MATS:
        for K in (2, 3, 5):
            splitter_cases(hip, orc, A, K, mdl)
            for combine in (0, 1):
                windowed_tables_case(hip, orc, A, K, mdl, combine)


@pytest.mark.parametrize("mi", [0, 1, 2, 3, 5])
def test_int64_wrap_pin_weighted_bottleneck(hip, orc, mi):
    """ConstrainedCost(f, AffineWorkModel(0, 0, 1), w_max): the valley search with the weight's j0 array (dp_driver.hip) or the literal kernel"""
    mdl = i64_wrap()[mi]
    wgt = cp.AffineWorkModel(0, 0, 1)
    for A in MATS:
        for K in (2, 5):
            for wmax in (-(-A.nnz // K) + 1, -(-3 * A.nnz // (2 * K)) + 1):
                windowed_tables_case(hip, orc, A, K, mdl, 1, wm=wgt, wmax=wmax)
                f = cp.ConstrainedCost(mdl, wgt, wmax)
                for meth in (cp.DynamicBottleneckSplitter(f), cp.DynamicBottleneckChunker(f)):
                    want = outcome(lambda: cp.partition_stripe(A, K, meth, backend=orc))
                    assert outcome(lambda: cp.partition_stripe(A, K, meth, backend=hip)) == want, (A, K, wmax, mdl._params())


@pytest.mark.parametrize("mi", range(6))
def test_int64_wrap_chunkers(hip, orc, mi):
    mdl = i64_wrap()[mi]
    for A in MATS:
        chunker_cases(hip, orc, A, mdl)


def test_int64_wrap_convex_chunker_batch(hip, orc):
    for A in MATS[3:]:
        meths = [cp.ConvexTotalChunker(cp.ConstrainedCost(m, cp.VertexCount(), w)) for m in i64_wrap()[:3] for w in (1, 4, 15)]
        meths += [cp.ConvexTotalChunker(cp.ConstrainedCost(cp.AffineConnectivityModel(2, 3, 1, 5), cp.VertexCount(), 4))]
        got = cp.pack_stripe_batch(A, meths, backend=hip)
        for m, g in zip(meths, got):
            assert g == cp.pack_stripe(A, m, backend=orc), (A, m.f.f._params(), m.f.w_max)


@pytest.mark.parametrize("mi", range(6))
def test_int64_wrap_bisect(hip, orc, mi):
    mdl = i64_wrap()[mi]
    for A in MATS:
        bisect_cases(hip, orc, A, mdl)


def test_int64_just_inside_the_bound_keeps_the_fast_paths(hip, orc):
    """b_net / b_pin as large as the bound allows: still exact, still answered with brute_max_n = 0"""
    for A in MATS:
        for K in (1, 2, 5):
            for mdl in i64_inside(A, K):
                for g in (0, 1):
                    assert tables_case(hip, orc, A, K, g, mdl), (A, K, g, mdl._params())
                for combine in (0, 1):
                    windowed_tables_case(hip, orc, A, K, mdl, combine)
        for mdl in i64_inside(A, A.n + 1):
            for w in (3, 16):
                fc = cp.ConstrainedCost(mdl, cp.VertexCount(), w)
                assert cp.pack_stripe(A, cp.DynamicTotalChunker(fc), backend=hip) == cp.pack_stripe(A, cp.DynamicTotalChunker(fc), backend=orc)


# ---------------------------------------------------------------- Float64 at 2^53

def test_float64_at_2_53(hip, orc):
    for A in MATS:
        if A.nnz == 0:
            continue
        for K in (1, 2, 5):
            edge = f64_edge(A, K)
            for mdl in edge:
                for g in (0, 1):
                    tables_case(hip, orc, A, K, g, mdl)
                for combine in (0, 1):
                    windowed_tables_case(hip, orc, A, K, mdl, combine)
            splitter_cases(hip, orc, A, K, edge[0])
            splitter_cases(hip, orc, A, K, edge[2])
        for mdl in f64_edge(A, A.n + 1)[:3]:
            chunker_cases(hip, orc, A, mdl)


# ---------------------------------------------------------------- non-dyadic Float64

@pytest.mark.parametrize("mi", range(len(NONDYADIC)))
def test_float64_non_dyadic(hip, orc, mi):
    """coefficients whose sums depend on their order: the literal kernels must add in the reference's order"""
    mdl = NONDYADIC[mi]
    for A in MATS:
        for K in (1, 2, 5, 8):
            for g in (0, 1):
                tables_case(hip, orc, A, K, g, mdl)
            splitter_cases(hip, orc, A, K, mdl)
            if getattr(mdl, "alpha_k", None) is None:
                for meth in (cp.ConvexTotalSplitter(mdl), cp.ConcaveTotalSplitter(mdl)):
                    assert outcome(lambda: cp.partition_stripe(A, K, meth, backend=hip)) == \
                        outcome(lambda: cp.partition_stripe(A, K, meth, backend=orc)), (A, K, type(meth).__name__)
        if getattr(mdl, "alpha_k", None) is None:
            chunker_cases(hip, orc, A, mdl)
            for w in (None, 4):
                f = mdl if w is None else cp.ConstrainedCost(mdl, cp.VertexCount(), w)
                assert outcome(lambda: cp.pack_stripe(A, cp.ConcaveTotalChunker(f), backend=hip)) == \
                    outcome(lambda: cp.pack_stripe(A, cp.ConcaveTotalChunker(f), backend=orc)), (A, w, "concave")
