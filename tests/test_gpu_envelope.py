"""GPU tests of the envelope cost family (kind 15): rowenvelope's tree and queries, the oracle, Step, objective and bound entry
points, the K-part DP by the valley search and by the candidate sweep with every table cell, the two Bisect splitters, the
permuting and alternating callers, the gates and the refusals -- bit for bit against tests/envelope_model.py.

Shapes: n = 1 (H = 0, one node), 3 (one padded leaf), powers of two and one past; n in 257, 1025 (a tree level of more than one
block); DP rows n + 1 in 2, 64, 65, 257 (one lane, a full wave, a wave with one live lane, more than one block); n = 70 000 for
the valley search where the literal tables are out of reach."""
import contextlib
import functools

import numpy as np
import pytest

import envelope_model as em
from util import cp, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu
ENV = cp.AffineEnvelopeModel
SUM, MAX = 0, 1


def _from_dense(D):
    m, n = D.shape
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


@functools.lru_cache(maxsize=None)
def pattern(m, n, seed, dens=0.08, full=True):
    """seeded pattern with empty columns and (full) one full column"""
    rng = np.random.default_rng(seed)
    D = rng.random((m, n)) < dens
    D[:, rng.random(n) < 0.3] = False
    if full:
        D[:, n // 3] = True
    return _from_dense(D)


def split(seed, n, K):
    rng = np.random.default_rng(seed)
    return cp.SplitPartition(K, np.concatenate([[1], np.sort(rng.integers(1, n + 2, K - 1)), [n + 1]]).astype(np.int64))


@contextlib.contextmanager
def option(hip, name, value, restore):
    hip.set_option(name, value)
    try:
        yield
    finally:
        hip.set_option(name, restore)


def valley_layers(hip, call):
    hip.set_option("stat_reset", 0)
    out = call()
    return out, hip.get_stat("env_valley_layers")


def tables(hip, A, K, combine, mdl):
    rc, ptr, cst = hip.dynamic_tables(A, K, combine, mdl.marshal(), None)
    assert rc == 0, hip.last_error()
    return ptr, cst


def model_tree(A):
    H, tree = em.build_tree(A)
    return H, tree, np.array(tree[1:], dtype=np.int64)


# ---------------------------------------------------------------- the structure
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 64, 65])
def test_tree_and_all_pairs(hip, n):
    A = pattern(n + 3, n, 100 + n, dens=0.2, full=False)
    env = cp.rowenvelope(A, backend=hip)
    H, tree, nodes = model_tree(A)
    assert (env.H, env.m, env.n) == (H, A.m, n) and env.shape == (n + 1, n + 1)
    assert env.tree.shape == ((2 << H) - 1, 2) and np.array_equal(env.tree, nodes)
    a, b = np.meshgrid(np.arange(1, n + 2), np.arange(1, n + 2), indexing="ij")
    j, jp = a[a <= b].astype(np.int64), b[a <= b].astype(np.int64)
    lo, hi = env.query(j, jp)
    want = [em.definition(A, int(x), int(y)) for x, y in zip(j, jp)]
    assert list(zip(lo.tolist(), hi.tolist())) == want
    assert want == [em.getindex(H, A.m, tree, int(x), int(y)) for x, y in zip(j, jp)]
    assert env[1, 1] == env[n + 1, n + 1] == (A.m + 1, 0) and env[1, n + 1] == em.definition(A, 1, n + 1)


@pytest.mark.parametrize("n", [257, 1025])
def test_tree_levels_of_more_than_one_block(hip, n):
    A = pattern(300, n, 200 + n, dens=0.02, full=False)
    env = cp.rowenvelope(A, backend=hip)
    H, tree, nodes = model_tree(A)
    assert env.H == H and np.array_equal(env.tree, nodes)
    rng = np.random.default_rng(n)
    j = rng.integers(1, n + 2, 2000).astype(np.int64)
    jp = np.array([rng.integers(x, n + 2) for x in j], dtype=np.int64)
    lo, hi = env.query(j, jp)
    assert list(zip(lo.tolist(), hi.tolist())) == [em.getindex(H, A.m, tree, int(x), int(y)) for x, y in zip(j, jp)]
    hip.reset_cache(A)                                         # the tree is rebuilt on the next call
    lo2, hi2 = env.query(j, jp)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)


def test_one_row_and_patterns_without_entries(hip):
    one = _from_dense(np.array([[1, 0, 1, 1, 0, 0, 1]], dtype=bool))
    empty = cp.SparseMatrixCSC(5, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))
    for A in (one, empty):
        env = cp.rowenvelope(A, backend=hip)
        H, tree, nodes = model_tree(A)
        assert np.array_equal(env.tree, nodes)
        for j in range(1, A.n + 2):
            for jp in range(j, A.n + 2):
                assert env[j, jp] == em.definition(A, j, jp)
    with pytest.raises(AssertionError):
        cp.rowenvelope(cp.SparseMatrixCSC(3, 0, np.ones(1, dtype=np.int64), np.zeros(0, dtype=np.int64)), backend=hip)
    with pytest.raises(AssertionError):
        cp.rowenvelope(one, backend=hip).query([2], [1])


# ---------------------------------------------------------------- oracle / step / objective / bounds
MODELS = [ENV(0, 10, 1, 100), ENV(3, 0, 2, 1), ENV(0.5, 0.25, 0.1, 1.7), ENV(1, 1, 2, 3, alpha_k=[4, -2, 9, 0, 7]),
          ENV(0.5, 1.0, 2.0, 0.25, alpha_k=[4.0, -0.5, 9.0, 1.0, 7.5])]


@pytest.mark.parametrize("mi", range(len(MODELS)))
def test_eval_step_objective_bounds(hip, mi):
    mdl = MODELS[mi]
    A = pattern(400, 60, 1)
    n = A.n
    E = em.Env(A, mdl)
    a, b = np.meshgrid(np.arange(1, n + 2), np.arange(1, n + 2), indexing="ij")
    j, jp = a[a <= b].astype(np.int64), b[a <= b].astype(np.int64)
    Pi = split(2, A.m, 5)                                      # a row partition passes through and is ignored
    for rows in (None, Pi):
        ocl = cp.oracle_stripe(cp.StepHint(), mdl, A, rows, backend=hip)
        for k in (1, 3, 5):
            assert np.array_equal(ocl(j, jp, k), E.table(k)[j - 1, jp - 1]), (mi, k)
    moves = [(cp.Jump(5), cp.Jump(20), 2), (cp.Same(5), cp.Next(21), 2), (cp.Next(6), cp.Same(21), 2), (cp.Prev(5), cp.Prev(20), 4),
             (cp.Jump(1), cp.Jump(n + 1), 5)]
    assert cp.Step(ocl).walk(moves).tolist() == [E.f(m[0].arg, m[1].arg, m[2]) for m in moves]
    rng = np.random.default_rng(3)
    for K in (1, 3, 5):
        Phi = split(10 + K, n, K)
        asg = rng.integers(1, K + 1, n)
        if K > 1:
            asg[asg == 2] = 1                                  # an unordered map with an empty part
        Map = cp.MapPartition(K, asg.astype(np.int64))
        Dom = cp.DomainPartition(K, rng.permutation(n).astype(np.int64) + 1, Phi.spl)
        for val, g in ((cp.total_value, "sum"), (cp.bottleneck_value, "max")):
            assert val(A, Phi, mdl, backend=hip) == val(A, Phi, mdl, Pi, backend=hip) == em.objective_split(E, Phi.spl, g)
            dm = cp.to_domain(Map)
            assert val(A, Map, mdl, backend=hip) == em.objective_domain(E, dm.prm, dm.spl, g)
            assert val(A, Dom, mdl, backend=hip) == em.objective_domain(E, Dom.prm, Dom.spl, g)
        assert cp.bound_stripe(A, K, mdl, backend=hip) == cp.bound_stripe(A, K, mdl, Pi, backend=hip) == em.bound_stripe(A, K, mdl)


def test_bound_stripe_preconditions(hip):
    A = pattern(40, 30, 5)
    for bad in (ENV(0, -1, 1, 1), ENV(0, 1, -1, 1), ENV(0.0, 1.0, 1.0, -0.5)):
        with pytest.raises(AssertionError, match="beta >= 0"):
            cp.bound_stripe(A, 3, bad, backend=hip)
    empty = cp.SparseMatrixCSC(5, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))
    with pytest.raises(AssertionError, match="AffineEnvelopeModel"):
        cp.bound_stripe(empty, 2, ENV(0, 1, 1, 1), backend=hip)


# ---------------------------------------------------------------- the DP, every cell
def _dp_models(K):
    ak = [int(v) for v in np.random.default_rng(K).integers(-3, 6, K)]
    return [ENV(0, 10, 1, 100), ENV(0.5, 0.25, 0.1, 1.7), ENV(1, 1, 2, 3, alpha_k=ak), ENV(0, 0, 0, 0), ENV(0, 1, -1, 2)]


@pytest.mark.parametrize("n", [1, 63, 64, 256])
def test_dynamic_tables_match_the_literal_dp(hip, n):
    A = pattern(50, n, 300 + n, dens=0.1)
    for K in (1, 2, 5, n + 3):
        for mdl in _dp_models(K)[::1 if K <= 5 or n < 64 else 2]:      # (K = n + 3 at the two larger sizes: the Int64, per-part and negative models)
            E = em.Env(A, mdl)
            gated = min(mdl.beta_vertex, mdl.beta_pin, mdl.beta_net) >= 0
            for combine, g in ((SUM, "sum"), (MAX, "max")):
                spl, cst, ptr = em.dp_literal(E, K, g)
                (gp, gc), layers = valley_layers(hip, lambda: tables(hip, A, K, combine, mdl))
                assert layers == (K - 1 if combine == MAX and gated else 0), (n, K, g, mdl._params())
                assert np.array_equal(gp, ptr) and np.array_equal(gc, cst), (n, K, g, mdl._params())
                with option(hip, "force_brute", 1, 0):
                    (gp, gc), layers = valley_layers(hip, lambda: tables(hip, A, K, combine, mdl))
                assert layers == 0
                assert np.array_equal(gp, ptr) and np.array_equal(gc, cst), ("brute", n, K, g, mdl._params())
                meth = (cp.DynamicTotalSplitter if combine == SUM else cp.ReferenceBottleneckSplitter)(mdl)
                assert np.array_equal(cp.partition_stripe(A, K, meth, backend=hip).spl, spl)


def test_int64_bound_past_2_60_takes_the_sweep(hip):
    A = pattern(50, 64, 364, dens=0.1)
    big = ENV(2 ** 58, 1, 1, 1)                                # K * alpha = 2^60 at K = 4
    for K, want in ((4, 0), (3, 2)):
        (gp, gc), layers = valley_layers(hip, lambda: tables(hip, A, K, MAX, big))
        _, cst, ptr = em.dp_literal(em.Env(A, big), K, "max")
        assert layers == want and np.array_equal(gp, ptr) and np.array_equal(gc, cst)


@pytest.mark.parametrize("mdl", [ENV(0, 10, 1, 100), ENV(0.5, 0.25, 0.1, 1.7)], ids=["i64", "f64"])
def test_valley_search_past_the_literal_tables(hip, mdl):
    n, K = 70_000, 4
    A = suitesparse_shaped(n, 6, 41)
    (ptr, cst), layers = valley_layers(hip, lambda: tables(hip, A, K, MAX, mdl))
    assert layers == K - 1
    with option(hip, "force_brute", 1, 0):
        (bptr, bcst), layers = valley_layers(hip, lambda: tables(hip, A, K, MAX, mdl))
    assert layers == 0
    assert np.array_equal(ptr, bptr) and np.array_equal(cst, bcst)
    E = em.Env(A, mdl, tables=False)
    rng = np.random.default_rng(42)
    cells = [(K, n + 1)] + [(int(rng.integers(2, K)), int(rng.integers(1, n + 2))) for _ in range(63)]
    for k, jp in cells:
        v = np.maximum(cst[:jp, k - 2], E.column(jp, k))
        i = v.size - 1 - int(np.argmin(v[::-1]))
        assert cst[jp - 1, k - 1] == v[i] and ptr[jp - 1, k - 1] == i + 1, (k, jp)
    assert np.array_equal(ptr[:, 0], np.ones(n + 1, dtype=np.int64)) and np.array_equal(cst[:, 0], E.row(1, 1))


# ---------------------------------------------------------------- the gates
def test_gates(hip):
    A = pattern(40, 200, 6, dens=0.1)
    ok, neg = ENV(0, 10, 1, 100), ENV(0, 1, -1, 2)
    with option(hip, "brute_max_n", 100, 200000):
        with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
            cp.partition_stripe(A, 3, cp.DynamicTotalSplitter(ok), backend=hip)
        with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
            cp.partition_stripe(A, 3, cp.DynamicBottleneckSplitter(neg), backend=hip)
        with option(hip, "force_brute", 1, 0):
            with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
                cp.partition_stripe(A, 3, cp.DynamicBottleneckSplitter(ok), backend=hip)
        got = cp.partition_stripe(A, 3, cp.DynamicBottleneckSplitter(ok), backend=hip).spl
    assert np.array_equal(got, em.dp_literal(em.Env(A, ok), 3, "max")[0])
    assert np.array_equal(cp.partition_stripe(A, 3, cp.DynamicTotalSplitter(ok), backend=hip).spl, em.dp_literal(em.Env(A, ok), 3, "sum")[0])


# ---------------------------------------------------------------- the Bisect splitters
@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("mdl", [ENV(1, 1, 2, 3), ENV(0.5, 0.25, 1.5, 2.75), ENV(0, 10, 1, 100)], ids=["i64", "f64", "net"])
def test_bisect_splitters_match_the_reference_loops(hip, K, mdl):
    A = pattern(90, 70, 4)
    E = em.Env(A, mdl)
    lo, hi = em.bound_stripe(A, K, mdl)
    Pi = split(5, A.m, 3)
    for eps in (0.1, 0.01):
        got = cp.partition_stripe(A, K, cp.BisectCostBottleneckSplitter(mdl, eps), backend=hip).spl
        assert np.array_equal(got, em.bisect_cost(E.f, A.n, K, eps, lo, hi)), eps
    got = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(mdl), Pi, backend=hip)
    assert np.array_equal(got.spl, em.bisect_index(E.f, A.n, K, lo, hi))
    _, cst, _ = em.dp_literal(E, K, "max")
    assert cp.bottleneck_value(A, got, mdl, backend=hip) == cst[A.n, K - 1]


# ---------------------------------------------------------------- callers
def test_permuting_partitioner(hip):
    A = golden_matrices()["HB/can_292"]
    mdl = ENV(0, 10, 1, 100)
    rcm, inner = cp.CuthillMcKeePermuter(), cp.DynamicBottleneckSplitter(mdl)
    tau = cp.permute_stripe(A, rcm, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    for K in (1, 4):
        got = cp.partition_stripe(A, K, cp.PermutingPartitioner(rcm, inner), backend=hip)
        Phi = cp.partition_stripe(B, K, inner, backend=hip)
        assert isinstance(got, cp.DomainPartition) and got == tau[Phi]
        assert np.array_equal(Phi.spl, em.dp_literal(em.Env(B, mdl), K, "max")[0])
        assert cp.bottleneck_value(A, got, mdl, backend=hip) == cp.bottleneck_value(B, Phi, mdl, backend=hip)


def test_alternating_partitioner(hip):
    A = pattern(120, 90, 7, dens=0.05)
    mdl = ENV(2, 1, 3, 5)
    K = 4
    meth = cp.AlternatingPartitioner(cp.DynamicBottleneckSplitter(mdl), cp.DynamicBottleneckSplitter(mdl), cp.BisectIndexBottleneckSplitter(mdl))
    Pi, Phi = cp.partition_plaid(A, K, meth, backend=hip)
    T = cp.adjointpattern(A, backend=hip)
    pi = em.dp_literal(em.Env(T, mdl), K, "max")[0]            # (every sweep ignores the other side's partition)
    phi = em.bisect_index(em.Env(A, mdl).f, A.n, K, *em.bound_stripe(A, K, mdl))
    assert np.array_equal(Pi.spl, pi) and np.array_equal(Phi.spl, phi)


# ---------------------------------------------------------------- refusals of the library entries
def test_library_refusals_name_the_model(hip):
    from chainpartitioners_jl_amd import models as M
    A = pattern(40, 30, 20)
    K, n = 3, A.n
    env, work = ENV(1, 1, 2, 3), cp.AffineWorkModel(0, 1, 1)
    mm, wk, vc = env.marshal(), work.marshal(), cp.VertexCount().marshal()
    spl, big, Kout = np.zeros(K + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    rp, keep = cp.api._rowpart(split(21, A.m, K))

    def refused(rc):
        assert rc == M.CP_EUNSUPPORTED and "AffineEnvelopeModel" in hip.last_error(), (rc, hip.last_error())

    refused(hip.partition_dynamic(A, K, SUM, M.CP_ORDER_CHUNKER, mm, None, None, 0, 0.0, spl))
    refused(hip.partition_dynamic(A, K, MAX, M.CP_ORDER_CHUNKER, mm, None, None, 0, 0.0, spl))
    refused(hip.partition_dynamic(A, K, SUM, M.CP_ORDER_SPLITTER, mm, None, vc, 5, 5.0, spl))       # constrained, the model as the cost
    refused(hip.partition_dynamic(A, K, MAX, M.CP_ORDER_SPLITTER, wk, None, mm, 5, 5.0, spl))       # ... and as the weight
    for call in (hip.pack_dynamic, hip.pack_convex, hip.pack_concave):
        refused(call(A, mm, None, None, 0, 0.0, big, Kout))
        refused(call(A, mm, None, vc, 5, 5.0, big, Kout))
        refused(call(A, wk, None, mm, 5, 5.0, big, Kout))
    refused(hip.pack_dynamic_tables(A, mm, None, None, 0, 0.0)[0])
    for call in (hip.partition_convex, hip.partition_concave):
        refused(call(A, K, mm, None, None, 0, 0.0, spl))
    refused(hip.partition_lazy_bisect_cost(A, K, mm, 0.1, spl))
    refused(hip.partition_lazy_bisect_cost_probes(A, K, mm, 0.1)[0])
    refused(hip.partition_lazy_flip_bisect_cost(A, K, mm, 0.1, spl))
    refused(hip.partition_bisect_cost(A, K, mm, 0.1, 1, spl))                                       # the Flip bisections
    refused(hip.partition_bisect_index(A, K, mm, 1, spl))
    refused(hip.partition_bisect_cost_batch(A, [K], [mm], [0.1], [0])[0])
    refused(hip.pack_convex_batch(A, [mm], [3], n)[0])
    refused(hip.dynamic_tables_constrained(A, K, mm, 5)[0])
    refused(hip.dynamic_tables_constrained(A, K, wk, 5, 1, mm)[0])
    refused(hip.partition_greedy_bottleneck(A, K, mm, rp, 0, None, np.zeros(n, dtype=np.int64))[0])
    with pytest.raises(RuntimeError, match="AffineEnvelopeModel"):
        hip.dp_begin(A, K, SUM, M.CP_ORDER_SPLITTER, mm, 1, n + 2)
    # and through the public interface, where the library's text arrives
    with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
        cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(env), split(21, A.m, K), backend=hip)
    env_h = cp.rowenvelope(A, backend=hip)                     # an envelope handle is no counter
    out = np.zeros(1, dtype=np.int64)
    assert hip.count_query("net", env_h.handle, np.ones(1, dtype=np.int64), np.ones(1, dtype=np.int64), out) == M.CP_EINVAL
