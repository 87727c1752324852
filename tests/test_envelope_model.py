"""CPU checks of the envelope family's model (tests/envelope_model.py) and of its Python side: the literal tree against the
definition as test_EnvelopeMatrices.jl does it, the valley search against the literal DP tables, the two-column witness that the
span is not Monge in either direction, and the model's promotion, marshalling and dispatch."""
import numpy as np
import pytest

import envelope_model as em
from util import cp, sprand
from test_abi_and_host import StubBackend

ENV = cp.AffineEnvelopeModel


def from_cols(m, cols):
    """pattern from a list of row lists (1-based rows, ascending)"""
    colptr = np.concatenate([[1], 1 + np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rowval = np.array([r for c in cols for r in c], dtype=np.int64)
    return cp.SparseMatrixCSC(m, len(cols), colptr, rowval)


def random_pattern(rng, m, n, dens, p_empty):
    cols = []
    for _ in range(n):
        rows = np.nonzero(rng.random(m) < dens)[0] + 1
        cols.append([] if rng.random() < p_empty else rows.tolist())
    return from_cols(m, cols)


# ---------------------------------------------------------------- the structure
def test_tree_query_is_the_definition():
    rng = np.random.default_rng(7)
    for m in range(1, 101):
        n = m
        A = sprand(m, n, 0.5, rng)
        H, tree = em.build_tree(A)
        assert H == em.cllog2(n) and len(tree) == 1 << (H + 1)
        pairs = [(int(j), int(rng.integers(j, n + 2))) for j in rng.integers(1, n + 2, 100)]
        if n <= 20:
            pairs += [(j, jp) for j in range(1, n + 2) for jp in range(j, n + 2)]
        for j, jp in pairs:
            assert em.getindex(H, m, tree, j, jp) == em.definition(A, j, jp), (m, j, jp)


def test_span_table_is_the_definition():
    rng = np.random.default_rng(8)
    A = random_pattern(rng, 30, 25, 0.15, 0.3)
    D = em.span_table(A)
    E = em.Env(A, ENV(1, 2, 3, 4))
    for j in range(1, A.n + 2):
        for jp in range(j, A.n + 2):
            lo, hi = em.definition(A, j, jp)
            assert D[j - 1, jp - 1] == max(hi - lo, 0)
        assert np.array_equal(E.column(j, 2), E.table(2)[:j, j - 1]) and np.array_equal(E.row(j, 2), E.table(2)[j - 1, j - 1:])


# ---------------------------------------------------------------- the valley search is the literal bottleneck DP
def _models(rng, K):
    ak_i = [int(v) for v in rng.integers(-3, 6, K)]
    return [ENV(0, 0, 0, 1), ENV(0, 10, 1, 100), ENV(2, 0, 1, 1), ENV(0, 1, 0, 0), ENV(0.5, 0.25, 0.1, 1.7), ENV(0, 0, 0, 0),
            ENV(1, 1, 2, 3, alpha_k=ak_i), ENV(0.5, 0.25, 0.1, 1.7, alpha_k=[float(v) + 0.5 for v in ak_i])]


def test_valley_search_reproduces_the_literal_tables():
    cases = 0
    for seed in range(60):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(1, 20))
        m = int(rng.integers(1, 15))
        K = [1, 2, n + 2, int(rng.integers(3, 6))][seed % 4]
        A = from_cols(m, [[]] * n) if seed % 15 == 7 else random_pattern(rng, m, n, rng.choice([0.1, 0.3, 0.6]), rng.choice([0.0, 0.3, 0.6]))
        for mdl in _models(rng, K):
            E = em.Env(A, mdl)
            spl, cst, ptr = em.dp_literal(E, K, "max")
            spl2, cst2, ptr2 = em.dp_valley(E, K)
            assert np.array_equal(cst, cst2) and np.array_equal(ptr, ptr2) and np.array_equal(spl, spl2), (seed, mdl.__dict__)
            cases += 1
    assert cases >= 300


def test_all_zero_model_ties_everywhere():
    A = random_pattern(np.random.default_rng(3), 9, 12, 0.3, 0.3)
    _, cst, ptr = em.dp_valley(em.Env(A, ENV(0, 0, 0, 0)), 4)
    assert not cst[:, :3].any() and cst[A.n, 3] == 0
    for k in (2, 3):
        assert ptr[:, k - 1].tolist() == list(range(1, A.n + 2))      # every candidate ties: the largest j wins
    assert ptr[A.n, 3] == A.n + 1 and not ptr[:A.n, 3].any()


# ---------------------------------------------------------------- the total objective is not Monge
def test_two_column_witness_and_both_directions():
    A = from_cols(9, [[1], [9]])
    D = em.span_table(A)
    d = lambda j, jp: int(D[j - 1, jp - 1])
    assert (d(1, 2), d(2, 3), d(1, 3)) == (0, 0, 8)
    # union [1, 3) and intersection [2, 2) of [1, 2) and [2, 3): the union is dearer than the two together
    assert d(1, 3) + d(2, 2) > d(1, 2) + d(2, 3)
    gt = lt = 0
    rng = np.random.default_rng(11)
    for _ in range(40):
        B = random_pattern(rng, 12, 10, 0.2, 0.2)
        T = em.span_table(B)
        for a in range(1, 12):
            for b in range(a, 12):
                for c in range(b, 12):
                    for e in range(c, 12):      # A = [a, c), B = [b, e): union [a, e), intersection [b, c)
                        x, y = T[a - 1, e - 1] + T[b - 1, c - 1], T[a - 1, c - 1] + T[b - 1, e - 1]
                        gt += x > y; lt += x < y
    assert gt > 0 and lt > 0


# ---------------------------------------------------------------- the Python side
def test_model_promotion_and_marshalling():
    from chainpartitioners_jl_amd import models as M
    assert M.CP_MODEL_ENVELOPE == 15 and ENV.kind == 15 and ENV.hip_only
    i = ENV(1, 2, 3, 4)
    assert i.dtype == M.CP_I64 and i(5, 6, 7) == 1 + 10 + 18 + 28
    mm = i.marshal()
    assert mm.struct.kind == 15 and mm.struct.dtype == M.CP_I64 and list(mm.struct.p_i64[:4]) == [1, 2, 3, 4]
    assert mm.struct.p_i64[3] == 4 and mm.struct.p_i64[4] == 0 and not mm.struct.alpha_k          # beta_net in slot 3 (CP_P_NET)
    f = ENV(beta_net=0.5)                                      # the keyword form with zero defaults (EnvelopeCosts.jl:12-14)
    assert f.dtype == M.CP_F64 and (f.alpha, f.beta_vertex, f.beta_pin, f.beta_net) == (0, 0, 0, 0.5)
    assert list(f.marshal().struct.p_f64[:4]) == [0.0, 0.0, 0.0, 0.5]
    k = ENV(0, 1, 1, 1, alpha_k=[3, -1])
    assert k.dtype == M.CP_I64 and k(1, 1, 1, 2) == 2
    mk = k.marshal()
    assert mk.struct.n_alpha_k == 2 and mk.keep[0].tolist() == [3, -1]
    assert ENV(0, 1, 1, 1, alpha_k=[0.5]).dtype == M.CP_F64


def test_dispatch_reaches_the_splitter_dp_and_refuses_the_rest():
    from chainpartitioners_jl_amd import models as M
    A = cp.SparseMatrixCSC(4, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))
    mdl = ENV(0, 1, 1, 2)
    for cls, combine in ((M.DynamicTotalSplitter, 0), (M.DynamicBottleneckSplitter, 1), (M.ReferenceTotalSplitter, 0), (M.ReferenceBottleneckSplitter, 1)):
        b = StubBackend()
        cp.partition_stripe(A, 3, cls(mdl), cp.SplitPartition(2, [1, 3, 5]), backend=b)
        (meth, args), = b.calls
        assert meth == "partition_dynamic" and args[1:4] == (3, combine, M.CP_ORDER_SPLITTER) and args[4].struct.kind == 15 and args[6] is None
    for meth, call in ((M.BisectCostBottleneckSplitter(mdl, 0.1), "partition_bisect_cost"), (M.BisectIndexBottleneckSplitter(mdl), "partition_bisect_index")):
        b = StubBackend()
        cp.partition_stripe(A, 3, meth, backend=b)
        assert [c[0] for c in b.calls] == [call]
    refused = [M.DynamicTotalChunker(mdl), M.DynamicBottleneckChunker(mdl), M.ReferenceTotalChunker(mdl), M.ConvexTotalSplitter(mdl), M.ConcaveTotalSplitter(mdl),
               M.LazyBisectCostBottleneckSplitter(mdl, 0.1), M.LazyFlipBisectCostBottleneckSplitter(mdl, 0.1), M.FlipBisectCostBottleneckSplitter(mdl, 0.1),
               M.FlipBisectIndexBottleneckSplitter(mdl), M.DynamicTotalSplitter(M.ConstrainedCost(mdl, M.VertexCount(), 3)),
               M.DynamicBottleneckSplitter(M.ConstrainedCost(M.AffineWorkModel(0, 1, 1), mdl, 3))]
    for method in refused:
        b = StubBackend()
        with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
            cp.partition_stripe(A, 3, method, backend=b)
        assert b.calls == [], type(method).__name__
    for method in (M.DynamicTotalChunker(mdl), M.ConvexTotalChunker(mdl), M.ConcaveTotalChunker(mdl),
                   M.ConvexTotalChunker(M.ConstrainedCost(mdl, M.VertexCount(), 3))):
        b = StubBackend()
        with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
            cp.pack_stripe(A, method, backend=b)
        with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
            cp.pack_stripe_batch(A, [method], backend=b)
        assert b.calls == []
    b = StubBackend()
    with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
        cp.partition_stripe_batch(A, [(3, M.BisectCostBottleneckSplitter(mdl, 0.1))], backend=b)
    with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
        cp.pack_stripe_tables(A, M.DynamicTotalChunker(mdl), backend=b)
    with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
        cp.partition_stripe(A, 3, M.GreedyBottleneckPartitioner(mdl), cp.SplitPartition(3, [1, 2, 3, 5]), backend=b)
    assert b.calls == []
    class Cpu(StubBackend):
        name = "orc"
    with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
        cp.partition_stripe(A, 3, M.DynamicTotalSplitter(mdl), backend=Cpu())
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.rowenvelope(A, backend=Cpu())
