"""GPU tests of the symmetric cost family: the dianet / selfpin counters, the three model kinds on the oracle, objective, bound and
DP entry points, BisectCost / BisectIndex / LazyBisectCost with the monotonized model, and the plaid caller -- all bit for bit
against tests/sym_model.py (definitions and the reference's loops in pure Python).

Shapes: n in 63, 64, 65, 255, 256, 257, all just past a change of the wavelet level count (H = cllog2(n + 2) grows from n = 2^H - 2,
where the top key n + 1 is 2^H - 1, to n = 2^H - 1: 62 -> 63, 254 -> 255; tests/test_gpu_count_edges.py has both sides of that
edge); diagonals full, empty and partial; empty
columns; one dense row; and one pattern with nnz + n > 2 * 16384 so the lazy stream crosses chunk boundaries and restarts inside a
chunk after a split.

Those sizes keep the dense tables of sym_model.py in reach.  At n = 20 011 (15 wavelet levels, more than ten 2048-key blocks of the
counter builds) the two counters and the oracle of every kind are compared with sm.Sym instead: whole rows and columns of the count
and cost tables from the entry list, about 7.5 * 10^5 pairs per counter.  The DP engines count with these structures on both sides
of their own comparisons at size, so this is where a miscount that appears only at size would show."""
import functools

import numpy as np
import pytest

import bellman_audit as ba
import sym_model as sm
from test_gpu_plaid_lazy import deg15_17, deg16
from util import cp, sprand, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu
M = cp.models
SIZES = [1, 2, 63, 64, 65, 255, 256, 257]


def _from_dense(D):
    n = D.shape[0]
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, rows.astype(np.int64) + 1)


@functools.lru_cache(maxsize=None)
def pattern(n, variant):
    """seeded square patterns: 'partial' (random diagonal), 'full' / 'empty' diagonal, 'holes' (empty columns, partial diagonal),
    'dense' (one dense row)"""
    rng = np.random.default_rng(1000 * n + len(variant))
    D = rng.random((n, n)) < min(0.5, 6.0 / max(n, 1))
    if variant == "full":
        D |= np.eye(n, dtype=bool)
    elif variant == "empty":
        D &= ~np.eye(n, dtype=bool)
    elif variant == "holes":
        D[:, rng.random(n) < 0.3] = False
    elif variant == "dense":
        D[n // 2, :] = True
    return _from_dense(D)


VARIANTS = ["partial", "full", "empty", "holes", "dense"]


@functools.lru_cache(maxsize=None)
def tables(n, variant):
    return sm.Tables(pattern(n, variant))


@functools.lru_cache(maxsize=None)
def big():
    A = suitesparse_shaped(3000, 12, 11)                      # nnz + n > 2 * 16384
    assert A.m == A.n and A.nnz + A.n > 2 * 16384
    return A


def squares():
    g = golden_matrices()
    return [g["HB/west0132"], g["Pajek/GD99_c"], g["HB/can_292"]]


def pairs(n, rng, count=2000):
    if n <= 65:
        a, b = np.meshgrid(np.arange(1, n + 2), np.arange(1, n + 2), indexing="ij")
        k = a <= b
        return a[k].astype(np.int64), b[k].astype(np.int64)
    j = rng.integers(1, n + 2, count); jp = rng.integers(1, n + 2, count)
    return np.minimum(j, jp).astype(np.int64), np.maximum(j, jp).astype(np.int64)


MODELS_I = [cp.AffineSymmetricConnectivityModel(3, 2, 1, 5, 40), cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2),
            cp.AffineSymmetricEdgeCutModel(1, 2, 3, 7)]
MODELS_F = [cp.AffineSymmetricConnectivityModel(0.5, 0.1, 0.3, 1.7, 2.9), cp.AffineMonotonizedSymmetricConnectivityModel(0.25, 0.1, 0.7, 3.3, 1.0),
            cp.AffineSymmetricEdgeCutModel(0.1, 0.3, 0.7, 1.1)]


# ---------------------------------------------------------------- counters
@pytest.mark.parametrize("n", SIZES)
def test_counters_match_definitions(hip, n):
    rng = np.random.default_rng(n)
    for v in VARIANTS:
        A = pattern(n, v)
        T = tables(n, v)
        j, jp = pairs(n, rng)
        assert np.array_equal(cp.dianetcount(A, backend=hip)(j, jp), T.get("dianet")[j - 1, jp - 1]), v
        assert np.array_equal(cp.selfpincount(A, backend=hip)(j, jp), T.get("selfpin")[j - 1, jp - 1]), v


def test_counters_on_reference_matrices_and_reproducible(hip):
    rng = np.random.default_rng(3)
    for A in squares():
        T = sm.Tables(A)
        j, jp = pairs(A.n, rng)
        d1 = cp.dianetcount(A, backend=hip)(j, jp); s1 = cp.selfpincount(A, cp.StepHint(), backend=hip)(j, jp)
        assert np.array_equal(d1, T.get("dianet")[j - 1, jp - 1]) and np.array_equal(s1, T.get("selfpin")[j - 1, jp - 1])
        hip.reset_cache(A)
        assert np.array_equal(cp.dianetcount(A, backend=hip)(j, jp), d1) and np.array_equal(cp.selfpincount(A, backend=hip)(j, jp), s1)


@functools.lru_cache(maxsize=None)
def at_size():
    """the pattern of the audits of test_gpu_sym_total.py at n = 20 011, 64 fixed ends j' and 16 fixed starts j (1, 2, n, n + 1, columns
    where colptr crosses a multiple of 2048, random) and the (j, j') pairs of their whole columns and rows"""
    from test_gpu_sym_total import holed, check_holed
    A = holed(20_011, 3)
    check_holed(A)
    n = A.n
    assert (n + 2).bit_length() == 15 and A.nnz + n > 10 * 2048               # H = cllog2(n + 2) = 15 wavelet levels
    rng = np.random.default_rng(2011)
    ends, starts = ba.fixed_ends(A, rng, 64), ba.fixed_ends(A, rng, 16)
    j, jp = ba.line_pairs(n, ends, starts)
    assert j.size >= 700_000 and {1, 2, n, n + 1} <= set(ends.tolist())
    return A, ends, starts, j, jp


def lines(ends, starts, column, row):
    return np.concatenate([column(int(e)) for e in ends] + [row(int(s)) for s in starts])


def test_counters_match_definitions_at_20011(hip):
    A, ends, starts, j, jp = at_size()
    S = sm.Sym(A)
    for name, count in (("dianet", cp.dianetcount), ("selfpin", cp.selfpincount)):
        want = lines(ends, starts, lambda e: S.count_column(name, e), lambda b: S.count_row(name, b))
        got = count(A, backend=hip)(j, jp)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, j[bad[:5]], jp[bad[:5]], got[bad[:5]], want[bad[:5]])


AT_SIZE_MODELS = [(MODELS_I[0], None), (MODELS_I[1], None), (MODELS_I[2], None), (cp.AffineSymmetricConnectivityModel(3.0, 2.0, 1.0, 5.0, 40.0), None),
                  (cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 3, 1, alpha_k=[5, 7, 11]), 1),
                  (cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 3, 1, alpha_k=[5, 7, 11]), 3)]


@pytest.mark.parametrize("which", range(len(AT_SIZE_MODELS)), ids=["sym_conn", "mono_sym", "edge_cut", "float64", "alpha_k_1", "alpha_k_3"])
def test_oracle_eval_matches_formulas_at_20011(hip, which):
    A, ends, starts, j, jp = at_size()
    mdl, k = AT_SIZE_MODELS[which]
    S = sm.Sym(A, mdl)
    want = lines(ends, starts, lambda e: S.column(e, k), lambda b: S.row(b, k))
    ocl = cp.oracle_stripe(cp.NoHint(), mdl, A, backend=hip)
    got = ocl(j, jp) if k is None else ocl(j, jp, k)
    bad = np.nonzero(got != want)[0]
    assert got.dtype == want.dtype and bad.size == 0, (mdl._params(), k, j[bad[:5]], jp[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_non_square_is_a_violated_precondition(hip):
    A = sprand(7, 9, 0.4, np.random.default_rng(2))
    for f in (cp.dianetcount, cp.selfpincount):
        with pytest.raises(AssertionError):
            f(A, backend=hip)
    for mdl in MODELS_I:
        with pytest.raises(AssertionError):
            cp.oracle_stripe(cp.NoHint(), mdl, A, backend=hip)(1, 2)
        with pytest.raises(AssertionError):
            cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(mdl), backend=hip)
    with pytest.raises(AssertionError):
        cp.bound_stripe(A, 2, MODELS_I[1], backend=hip)


# ---------------------------------------------------------------- oracle / step / objective / bound
@pytest.mark.parametrize("n", SIZES)
def test_oracle_eval_matches_formulas(hip, n):
    rng = np.random.default_rng(10 + n)
    for v in ("partial", "holes", "dense"):
        A, T = pattern(n, v), tables(n, v)
        j, jp = pairs(n, rng, 500)
        for mdl in MODELS_I + MODELS_F:
            got = cp.oracle_stripe(cp.NoHint(), mdl, A, backend=hip)(j, jp)
            want = sm.cost_table(T, mdl)[j - 1, jp - 1]
            assert got.dtype == want.dtype and np.array_equal(got, want), (v, type(mdl).__name__)
    f = cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 3, 1, alpha_k=[5, 7, 11])
    A, T = pattern(n, "partial"), tables(n, "partial")
    j, jp = pairs(n, rng, 300)
    for k in (1, 3):
        assert np.array_equal(cp.oracle_stripe(cp.NoHint(), f, A, backend=hip)(j, jp, k), sm.cost_table(T, f, k)[j - 1, jp - 1])


def test_int64_costs_wrap_like_julia(hip):
    A, T = pattern(65, "partial"), tables(65, "partial")
    j, jp = pairs(65, None)
    for mdl in (cp.AffineSymmetricConnectivityModel(2**62, 2**61, 3, -2**60, 2**59), cp.AffineSymmetricEdgeCutModel(-2**62, 2**62, 2**61, 5),
                cp.AffineMonotonizedSymmetricConnectivityModel(2**62, 2**60, 2**61, 2**59, 1)):
        assert np.array_equal(cp.oracle_stripe(cp.NoHint(), mdl, A, backend=hip)(j, jp), sm.cost_table(T, mdl)[j - 1, jp - 1])


def test_non_integral_delta_pins_is_refused(hip):
    with pytest.raises(AssertionError):
        cp.oracle_stripe(cp.NoHint(), cp.AffineMonotonizedSymmetricConnectivityModel(0.0, 0.0, 1.0, 2.0, 1.5), pattern(64, "partial"), backend=hip)(1, 3)


def test_oracle_step_walk(hip):
    A, T = pattern(65, "partial"), tables(65, "partial")
    n = A.n
    for mdl in MODELS_I + MODELS_F[:1]:
        F = sm.cost_table(T, mdl)
        st = cp.Step(cp.oracle_stripe(cp.StepHint(), mdl, A, backend=hip))
        moves = [(cp.Jump(1), cp.Jump(1))] + [(cp.Same(1), cp.Next(jp)) for jp in range(2, n + 2)]
        moves += [(cp.Next(j), cp.Same(n + 1)) for j in range(2, n + 2)] + [(cp.Prev(j), cp.Prev(j + 3)) for j in range(n, 20, -1) if j + 3 <= n + 1]
        moves = moves[:n + 1 + n] + [(cp.Jump(5), cp.Jump(40)), (cp.Prev(4), cp.Next(41)), (cp.Same(4), cp.Prev(40))]
        got = st.walk(moves)
        want = np.array([F[a.arg - 1, b.arg - 1] for a, b in moves])
        assert np.array_equal(got, want)
        with pytest.raises(AssertionError):
            st.walk([(cp.Jump(3), cp.Jump(9)), (cp.Next(5), cp.Same(9))])


def test_objective(hip):
    rng = np.random.default_rng(8)
    for n in (64, 257):
        A, T = pattern(n, "holes"), tables(n, "holes")
        for K in (1, 5):
            cut = np.sort(rng.integers(1, n + 2, K - 1))
            Phi = cp.SplitPartition(K, np.concatenate([[1], cut, [n + 1]]).astype(np.int64))
            for mdl in MODELS_I + MODELS_F + [cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 3, 1, alpha_k=[5, 7, 11, 2, 3])]:
                assert cp.total_value(A, Phi, mdl, backend=hip) == sm.objective(T, mdl, Phi.spl, "sum")
                assert cp.bottleneck_value(A, Phi, mdl, backend=hip) == sm.objective(T, mdl, Phi.spl, "max")


def test_bound_stripe(hip):
    for n, v in ((63, "partial"), (256, "holes"), (2, "empty")):
        A, T = pattern(n, v), tables(n, v)
        for mdl in (MODELS_I[1], MODELS_F[1], cp.AffineMonotonizedSymmetricConnectivityModel(4, 1, 2, 3, 0)):
            for K in (1, 3, 32):
                assert cp.bound_stripe(A, K, mdl, backend=hip) == sm.bound_stripe_model(A, K, mdl), (n, K)
        f = cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 3, 1, alpha_k=[5, 700000, 11])
        assert cp.bound_stripe(A, 3, f, backend=hip) == sm.bound_stripe_funky(T, 3, f)
        with pytest.raises(AssertionError):                                   # a negative beta: the reference asserts
            cp.bound_stripe(A, 2, cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, -1, 3, 0), backend=hip)
        for mdl in (MODELS_I[0], MODELS_I[2]):                                # no bound_stripe method in the reference
            with pytest.raises(NotImplementedError):
                cp.bound_stripe(A, 2, mdl, backend=hip)
            with pytest.raises(NotImplementedError):
                cp.partition_stripe(A, 2, cp.BisectCostBottleneckSplitter(mdl, 0.1), backend=hip)
            with pytest.raises(NotImplementedError):
                cp.partition_stripe(A, 2, cp.BisectIndexBottleneckSplitter(mdl), backend=hip)


def test_methods_without_the_new_kinds_refuse(hip):
    A = pattern(64, "partial")
    for mdl in MODELS_I:
        with pytest.raises(NotImplementedError):
            cp.pack_stripe(A, cp.DynamicTotalChunker(mdl), backend=hip)
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, 3, cp.ConvexTotalSplitter(mdl), backend=hip)
        with pytest.raises(NotImplementedError):
            cp.pack_stripe(A, cp.ConcaveTotalChunker(mdl), backend=hip)
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, 3, cp.DynamicTotalSplitter(cp.ConstrainedCost(mdl, cp.VertexCount(), 30)), backend=hip)
        mm = mdl.marshal()
        assert hip.dynamic_tables_constrained(A, 3, mm, 30)[0] == M.CP_EUNSUPPORTED
        with pytest.raises(RuntimeError):
            hip.dp_begin(A, 3, 0, 0, mm, 1, A.n + 2)
    rc, _ = hip.partition_bisect_cost_batch(A, [3], [MODELS_I[1].marshal()], [0.1], [0])
    assert rc == M.CP_EUNSUPPORTED
    rc, _ = hip.pack_convex_batch(A, [MODELS_I[1].marshal()], [4], A.n)
    assert rc == M.CP_EUNSUPPORTED


# ---------------------------------------------------------------- the dynamic programme
METHODS = {("sum", "splitter"): cp.DynamicTotalSplitter, ("max", "splitter"): cp.DynamicBottleneckSplitter,
           ("sum", "chunker"): cp.DynamicTotalChunker, ("max", "chunker"): cp.DynamicBottleneckChunker}


@pytest.mark.parametrize("n", SIZES)
def test_dynamic_equals_the_literal_dp(hip, n):
    v = VARIANTS[n % len(VARIANTS)]
    A, T = pattern(n, v), tables(n, v)
    models = MODELS_I + ([MODELS_F[n % 3]] if n <= 65 else [])
    for mdl in models:
        for K in (1, 2, 7, n + 3):
            for g in ("sum", "max"):
                want, _ = sm.dp_partition(T, mdl, K, g)                        # (no per-part alpha: both loop orders fill the same tables)
                for order in ("splitter", "chunker"):
                    got = cp.partition_stripe(A, K, METHODS[(g, order)](mdl), backend=hip)
                    assert np.array_equal(got.spl, want), (type(mdl).__name__, K, g, order)


def test_dynamic_per_part_alpha_and_tables(hip):
    A, T = pattern(65, "partial"), tables(65, "partial")
    f = cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 30, 1, alpha_k=[50, 7, 110, 2, 3, 900, 1])
    for g in ("sum", "max"):
        for order in ("splitter", "chunker"):
            want, _ = sm.dp_partition(T, f, 7, g, order)
            assert np.array_equal(cp.partition_stripe(A, 7, METHODS[(g, order)](f), backend=hip).spl, want), (g, order)
    for mdl in MODELS_I:
        rc, ptr, cst = hip.dynamic_tables(A, 3, M.CP_COMBINE_SUM, mdl.marshal(), None)
        assert rc == 0
        F = sm.cost_table(T, mdl)
        c1 = F[0, :]
        c2, p2 = sm.brute.layer(c1, F)
        assert np.array_equal(cst[:, 0], c1) and np.array_equal(cst[:, 1], c2) and np.array_equal(ptr[:, 1], p2 + 1)


@pytest.mark.parametrize("n", [257, 1000])
def test_valley_search_equals_the_sweep_and_the_literal_dp(hip, n):
    """kind 11 under max: the default call runs the valley search (counted by the bn_sym_layers stat), force_brute the sweep; both
    give the literal DP's split vector and tables (n = 1000 is no multiple of 64)"""
    A = pattern(n, "partial")
    T = sm.Tables(A)
    for mdl, K in ((MODELS_I[1], 7), (MODELS_F[1], 4), (cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 30, 1, alpha_k=[50, 7, 110, 2, 3]), 5)):
        want, _ = sm.dp_partition(T, mdl, K, "max")
        hip.set_option("stat_reset", 0)
        got = cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(mdl), backend=hip)
        assert hip.get_stat("bn_sym_layers") == K - 1                     # every layer after the first went through the valley search
        rc, ptr, cst = hip.dynamic_tables(A, K, M.CP_COMBINE_MAX, mdl.marshal(), None)
        assert rc == 0
        hip.set_option("force_brute", 1)
        hip.set_option("stat_reset", 0)
        try:
            forced = cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(mdl), backend=hip)
            rc2, ptr2, cst2 = hip.dynamic_tables(A, K, M.CP_COMBINE_MAX, mdl.marshal(), None)
            assert hip.get_stat("bn_sym_layers") == 0
        finally:
            hip.set_option("force_brute", 0)
        assert np.array_equal(got.spl, want) and np.array_equal(forced.spl, want)
        # the value tables agree everywhere; the argmins on every row of the layers before the last (layer K holds row n + 1 only)
        assert rc2 == 0 and np.array_equal(cst[:, :K - 1], cst2[:, :K - 1]) and np.array_equal(ptr[:, :K - 1], ptr2[:, :K - 1])
        assert cst[n, K - 1] == cst2[n, K - 1] and ptr[n, K - 1] == ptr2[n, K - 1]


def test_valley_search_gate(hip):
    """a negative beta or an Int64 model whose totals could wrap stays on the sweep; the total-cost objective always does"""
    A, T = pattern(257, "partial"), tables(257, "partial")
    for mdl, g in ((cp.AffineMonotonizedSymmetricConnectivityModel(0, -1, 2, 30, 1), "max"), (cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 2**58, 1), "max"),
                   (MODELS_I[1], "sum")):
        hip.set_option("stat_reset", 0)
        got = cp.partition_stripe(A, 5, METHODS[(g, "splitter")](mdl), backend=hip)
        assert hip.get_stat("bn_sym_layers") == 0
        assert np.array_equal(got.spl, sm.dp_partition(T, mdl, 5, g)[0])


# ---------------------------------------------------------------- bisection splitters
@pytest.mark.parametrize("n", [2, 64, 257])
def test_bisect_cost_equals_the_literal_chain(hip, n):
    A, T = pattern(n, "partial"), tables(n, "partial")
    for mdl in (MODELS_I[1], MODELS_F[1], cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 30, 1, alpha_k=list(range(40, 8, -1)))):
        for K in (1, 2, 32):
            for eps in (0.01, 0.5):
                want, _ = sm.bisect_cost(T, K, mdl, eps)
                got = cp.partition_stripe(A, K, cp.BisectCostBottleneckSplitter(mdl, eps), backend=hip)
                assert np.array_equal(got.spl, want), (K, eps)


@pytest.mark.parametrize("n", [2, 63, 256, 257])
def test_bisect_index_equals_the_literal_chain(hip, n):
    """the split vector of the literal BisectIndex chain, and (the cost grows with its part) the DP optimum as its value"""
    A, T = pattern(n, "holes"), tables(n, "holes")
    for mdl in (MODELS_I[1], MODELS_F[1], cp.AffineMonotonizedSymmetricConnectivityModel(2, 1, 2, 30, 0),
                cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 30, 1, alpha_k=list(range(40, 8, -1))),
                cp.AffineMonotonizedSymmetricConnectivityModel(0.5, 0.25, 1.5, 2.75, 1.0, alpha_k=[0.5 * v for v in range(40, 8, -1)])):
        for K in (1, 2, 7, 32):
            want, _ = sm.bisect_index(T, K, mdl)
            got = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(mdl), backend=hip)
            assert np.array_equal(got.spl, want), (type(mdl).__name__, K)
            if mdl.alpha_k is None and mdl.dtype == M.CP_I64:
                assert sm.objective(T, mdl, got.spl, "max") == sm.dp_partition(T, mdl, K, "max")[1], K


def _lazy(hip, A, K, mdl, eps):
    rc, spl, probes = hip.partition_lazy_bisect_cost_probes(A, K, mdl.marshal(), eps)
    assert rc == 0, hip.last_error()
    assert np.array_equal(cp.partition_stripe(A, K, cp.LazyBisectCostBottleneckSplitter(mdl, eps), backend=hip).spl, spl)
    return spl, probes


@pytest.mark.parametrize("n", SIZES)
def test_lazy_equals_the_literal_loop(hip, n):
    for v in ("partial", "full", "empty", "holes", "dense"):
        A = pattern(n, v)
        for mdl in (MODELS_I[1], MODELS_F[1], cp.AffineMonotonizedSymmetricConnectivityModel(0, 1, 2, 30, 1, alpha_k=list(range(40, 8, -1)))):
            for K in (1, 2, 32):
                for eps in (0.01, 0.5):
                    want, wp = sm.lazy_bisect(A, K, mdl, eps)
                    spl, probes = _lazy(hip, A, K, mdl, eps)
                    assert np.array_equal(spl, want) and probes == wp, (v, type(mdl).__name__, K, eps)


def test_lazy_on_reference_matrices_and_the_headline_model(hip):
    sym_model = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)          # bin/test_table_bottleneck.jl:22
    for A in squares():
        for mdl in (sym_model, MODELS_I[1]):
            for K in (2, 32):
                want, wp = sm.lazy_bisect(A, K, mdl, 0.01)
                spl, probes = _lazy(hip, A, K, mdl, 0.01)
                assert np.array_equal(spl, want) and probes == wp


@pytest.mark.parametrize("pat, K", [pytest.param(big, 1, id="1"), pytest.param(big, 2, id="2"), pytest.param(big, 32, id="32"),
                                    pytest.param(deg16, 5, id="deg16"), pytest.param(deg15_17, 5, id="deg15_17")])
def test_lazy_across_chunk_boundaries(hip, pat, K):
    A = pat()
    for mdl, eps in ((MODELS_I[1], 0.01), (cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 9), 0.5)):
        want, wp = sm.lazy_bisect(A, K, mdl, eps)
        spl, probes = _lazy(hip, A, K, mdl, eps)
        assert np.array_equal(spl, want) and probes == wp
    assert wp > 0 or K == 1


def test_lazy_without_a_probe(hip):
    """c_lo * (1 + eps) >= c_hi from the start: no probe runs and the initial spl_hi = [1, n+1, ..., n+1] comes back"""
    A = pattern(64, "partial")
    mdl = cp.AffineMonotonizedSymmetricConnectivityModel(10**9, 0, 1, 1, 0)
    want, wp = sm.lazy_bisect(A, 3, mdl, 0.5)
    spl, probes = _lazy(hip, A, 3, mdl, 0.5)
    assert wp == 0 and probes == 0 and np.array_equal(spl, want) and list(spl) == [1, 65, 65, 65]


def test_plaid_symmetric_partitioner(hip):
    sym_model = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)
    for A in squares()[:2] + [pattern(257, "partial")]:
        Pi, Phi = cp.partition_plaid(A, 8, cp.SymmetricPartitioner(cp.LazyBisectCostBottleneckSplitter(sym_model, 0.01)), backend=hip)
        want, _ = sm.lazy_bisect(A, 8, sym_model, 0.01)
        assert np.array_equal(Pi.spl, Phi.spl) and np.array_equal(Pi.spl, want)
