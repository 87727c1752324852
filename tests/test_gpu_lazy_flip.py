"""partition_stripe(A, K, LazyFlipBisectCostBottleneckSplitter(f, eps), [Pi]) on the device (csrc/lazy_flip.hip;
LazyBisectCostBottleneckSplitter.jl:72-138): the split vector and the number of probes are those of tests/lazy_flip_model.py, the
reference's loop in pure Python, for the secondary model under a row split, the connectivity models with per-part alpha and the
primary model under a row partition."""
import numpy as np
import pytest

import lazy_flip_model as lfm
from test_gpu_plaid_lazy import CHUNK_CASES, big, cyclic, dense_column, pattern, split
from util import cp, golden_matrices

pytestmark = pytest.mark.gpu

M = cp.models
CONN, PRIM, SEC = cp.AffineConnectivityModel, cp.AffinePrimaryConnectivityModel, cp.AffineSecondaryConnectivityModel
Lazy, LazyFlip = cp.LazyBisectCostBottleneckSplitter, cp.LazyFlipBisectCostBottleneckSplitter
LOC = SEC(0, 10, 1, 0, 100)                         # loc_model of bin/test_table_bottleneck.jl
NET, COMM = CONN(0, 10, 1, 100), PRIM(0, 10, 1, 0, 100)


def _r(A, K):
    return np.random.default_rng(7 * A.n + K).integers(1, 11, K)


def funky_conn(A, K, flt=False):
    """test_Partitioners.jl:124, and a Float64 model of the same shape"""
    base = 1 + A.nnz + 3 * A.n + 3 * A.m
    if flt:
        return CONN(0.0, -3.0, -1.0, -2.5, alpha_k=[float(base + v) + 0.25 for v in _r(A, K)])
    return CONN(0, -3, -1, -3, alpha_k=[int(base + v) for v in _r(A, K)])


def funky_prim(A, K):
    """test_Partitioners.jl:125"""
    return PRIM(0, -2, -1, -3, -6, alpha_k=[int(1 + A.nnz + 3 * A.n + 6 * A.m + v) for v in _r(A, K)])


def flip(hip, A, K, mdl, Pi, eps):
    """the entry with its probe count, and partition_stripe through the dispatch: the same split vector"""
    from chainpartitioners_jl_amd import api
    rp, keep = api._rowpart(Pi)
    rc, spl, probes = hip.partition_lazy_flip_bisect_cost_probes(A, K, mdl.marshal(), eps, rp)
    assert rc == 0, hip.last_error()
    assert np.array_equal(cp.partition_stripe(A, K, LazyFlip(mdl, eps), Pi, backend=hip).spl, spl)
    return spl, probes


def same_as_model(hip, A, K, mdl, Pi, eps, trace=None):
    want, wp = lfm.lazy_flip_bisect(A, K, mdl, Pi, eps, trace)
    spl, probes = flip(hip, A, K, mdl, Pi, eps)
    assert np.array_equal(spl, want) and probes == wp, (A, K, type(Pi).__name__, Pi and Pi.K, mdl._params(), mdl.alpha_k, eps, spl, want,
                                                        probes, wp)
    return spl, probes


# ---------------------------------------------------------------- the basic grid
@pytest.mark.parametrize("mf", [0, 1, 3], ids=["m=1", "m=n", "m=3n"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_equals_the_literal_loop(hip, n, mf):
    m = max(1, mf * n)
    A = pattern(m, n)
    for K in (1, 2, 7, 32):
        Pi = split(m, K)                                              # partition_stripe(A', K, EquiSplitter()); empty parts when m < K
        for eps in (0.01, 0.5):
            for mdl in (SEC(0, 2, 1, 3, 6), LOC, SEC(0.25, 0.1, 0.7, 1.9, 3.3)):
                same_as_model(hip, A, K, mdl, Pi, eps)
            spl, probes = same_as_model(hip, A, K, SEC(0, 2, 1, 6, 3), Pi, eps)     # increasing: every probe fails
            assert list(spl) == [1] + [n + 1] * K
            for flt in (False, True):
                same_as_model(hip, A, K, funky_conn(A, K, flt), None, eps)
            for PK in sorted({K, (K + 1) // 2}):
                for P in (split(m, PK), cyclic(m, PK)):
                    same_as_model(hip, A, K, funky_prim(A, K), P, eps)


# ---------------------------------------------------------------- control flow
def test_leading_empty_parts_and_runs_of_closed_parts(hip):
    lead = runs = 0
    for m, n, K in ((63, 63, 7), (64, 64, 32), (257, 40, 7)):
        trace = []
        same_as_model(hip, pattern(m, n), K, SEC(0, 2, 1, 3, 6), split(m, K), 0.01, trace)
        lead += sum(1 for t in trace if t[0] == "lead" and t[1] > 0)
        runs += sum(1 for t in trace if t[0] == "run" and t[2] > 1)
        assert ("exit", "split") in trace and ("exit", "fail") in trace
    assert lead > 0 and runs > 0


def test_success_inside_the_leading_loop(hip):
    """increasing models with a free empty part: f(1, 1, k) = 0 <= c for every k, and k == K ends the probe before a column is read"""
    A = pattern(64, 64)
    for mdl, Pi in ((CONN(0, 3, 1, 3), None), (PRIM(0, 2, 1, 3, 6), cyclic(64, 3)), (CONN(0.0, 0.5, 1.0, 3.0), None)):
        trace = []
        spl, probes = same_as_model(hip, A, 7, mdl, Pi, 0.1, trace)
        assert probes > 0 and {t for t in trace if t[0] == "exit"} == {("exit", "lead")} and list(spl) == [1] * 7 + [65]


def test_without_a_probe(hip):
    A = pattern(64, 64)
    spl, probes = same_as_model(hip, A, 3, SEC(10**9, 0, 1, 1, 1), split(64, 3), 0.5)
    assert probes == 0 and list(spl) == [1, 65, 65, 65]


# ---------------------------------------------------------------- chunk boundaries
@pytest.mark.parametrize("pat, K", CHUNK_CASES)
def test_across_chunk_boundaries(hip, pat, K):
    A = pat()                                                         # nnz > 2 * 16384: splits fall inside chunks
    for mdl, Pi in ((LOC, split(A.m, K)), (funky_conn(A, K), None), (funky_prim(A, K), cyclic(A.m, (K + 1) // 2))):
        spl, probes = same_as_model(hip, A, K, mdl, Pi, 0.01)
        assert probes > 0


@pytest.mark.parametrize("K", [3, 8])
def test_column_longer_than_a_chunk(hip, K):
    A = dense_column()
    assert A.colptr[40] - A.colptr[39] > 16384
    for mdl, Pi in ((LOC, split(A.m, K)), (SEC(0, 2, 1, 3, 6), split(A.m, K)), (funky_conn(A, K), None), (funky_prim(A, K), split(A.m, K))):
        spl, probes = same_as_model(hip, A, K, mdl, Pi, 0.01)
        assert probes > 0


# ---------------------------------------------------------------- the reference's matrices, its benchmark's model
@pytest.mark.parametrize("name", sorted(golden_matrices()))
def test_reference_matrices_loc_model(hip, name):
    A = golden_matrices()[name]
    T = cp.adjointpattern(A, backend=hip)
    for K in (2, 32):
        same_as_model(hip, T, K, LOC, split(T.m, K), 0.01)


# ---------------------------------------------------------------- quality
def test_bottleneck_within_eps_of_the_exact_flip_splitter(hip):
    A = big()
    for K, eps in ((8, 0.1), (32, 0.01)):
        Pi = split(A.m, K)
        got = cp.partition_stripe(A, K, LazyFlip(LOC, eps), Pi, backend=hip)
        best = cp.partition_stripe(A, K, cp.FlipBisectIndexBottleneckSplitter(LOC), Pi, backend=hip)
        v, opt = cp.bottleneck_value(A, got, LOC, Pi, backend=hip), cp.bottleneck_value(A, best, LOC, Pi, backend=hip)
        print(f"K={K} eps={eps}: LazyFlip {v}, FlipBisectIndex {opt}")
        assert v <= (1 + eps) * opt


# ---------------------------------------------------------------- entry errors
def test_entry_errors(hip):
    from chainpartitioners_jl_amd import api
    A = pattern(40, 30)
    K = 3
    rp, keep = api._rowpart(split(A.m, 3))
    rp4, keep4 = api._rowpart(split(A.m, 4))
    rp2, keep2 = api._rowpart(split(A.m, 2))
    rpm, keepm = api._rowpart(cyclic(A.m, 3))
    spl = np.zeros(K + 1, dtype=np.int64)
    entry = lambda mdl, rp: hip.lib.cp_partition_lazy_flip_bisect_cost(hip.csr(A), K, mdl.marshal(w_table=A.n + 1), rp, 0.1, spl, None)
    assert entry(LOC, rp) == M.CP_OK and entry(COMM, rp) == M.CP_OK and entry(COMM, rp2) == M.CP_OK and entry(NET, None) == M.CP_OK
    assert entry(NET, rp4) == M.CP_OK                                 # a connectivity model: Pi is not looked at
    # kinds without a device path, by name
    for mdl, name in ((cp.AffineWorkModel(0, 10, 1), "work"), (cp.AffineHyperedgeCutModel(0, 1, 1, 1, 2), "hyperedge cut"),
                      (cp.AffineMonotonizedSymmetricConnectivityModel(0, 3, 1, 3, 5), "monotonized symmetric connectivity"),
                      (cp.AffinePrimaryEdgeCutModel(0, 1, 1, 2), "primary edge cut"), (cp.AffineSecondaryEdgeCutModel(0, 1, 1, 2), "secondary edge cut")):
        assert entry(mdl, rp) == M.CP_EUNSUPPORTED and f"the {name} model" in hip.last_error(), (name, hip.last_error())
    blk = cp.BlockComponentCostModel(1, 0, (2,), (3,))
    assert hip.lib.cp_partition_lazy_flip_bisect_cost(hip.csr(A), K, blk.marshal(w_table=A.n + 1, u_table=A.m + 1), rp, 0.1, spl, None) == M.CP_EUNSUPPORTED
    assert "the block model" in hip.last_error()
    # the secondary model: a split of the rows with exactly K parts
    assert entry(LOC, None) == M.CP_EINVAL and "needs a row partition Pi" in hip.last_error()
    assert entry(LOC, rpm) == M.CP_EINVAL and "SplitPartition of the rows with exactly K parts" in hip.last_error()
    for bad in (rp2, rp4):
        assert entry(LOC, bad) == M.CP_EINVAL and "exactly K parts" in hip.last_error()
    # the primary model: a row partition with at most K parts
    assert entry(COMM, None) == M.CP_EINVAL and "needs a row partition Pi" in hip.last_error()
    assert entry(COMM, rp4) == M.CP_EINVAL and "more parts than K" in hip.last_error()
    # a plain model with a negative beta: the bound asserts
    for bad, r in ((SEC(0, 10, 1, 0, -100), rp), (SEC(0.0, 10.0, -1.0, 0.5, 100.0), rp), (PRIM(0, -1, 1, 0, 100), rp), (CONN(0, 3, 1, -3), None)):
        assert entry(bad, r) == M.CP_EINVAL and "beta >= 0" in hip.last_error()
    with pytest.raises(AssertionError, match="beta >= 0"):
        cp.partition_stripe(A, K, LazyFlip(CONN(0, -3, 1, 3), 0.1), backend=hip)
    with pytest.raises(NotImplementedError, match="the work model"):
        cp.partition_stripe(A, K, LazyFlip(cp.AffineWorkModel(0, 10, 1), 0.1), backend=hip)
    # nprobes_out is optional
    n1 = np.zeros(1, dtype=np.int64)
    s1 = np.zeros(K + 1, dtype=np.int64)
    assert hip.lib.cp_partition_lazy_flip_bisect_cost(hip.csr(A), K, LOC.marshal(), rp, 0.1, s1, n1) == M.CP_OK
    assert entry(LOC, rp) == M.CP_OK and np.array_equal(s1, spl) and int(n1[0]) > 0


# ---------------------------------------------------------------- the plaid caller
def test_plaid_alternating_partitioner(hip):
    """bin/test_table_bottleneck.jl:48 and its four-method form with Lazy(comm_model)"""
    eps, K = 0.1, 8
    for A in (golden_matrices()["HB/can_292"], golden_matrices()["LPnetlib/lp_blend"], pattern(120, 257)):
        T = cp.adjointpattern(A, backend=hip)
        Pi, Phi = cp.partition_plaid(A, K, cp.AlternatingPartitioner(Lazy(NET, eps), LazyFlip(LOC, eps)), adj_A=T, backend=hip)
        phi = cp.partition_stripe(A, K, Lazy(NET, eps), backend=hip)
        pi = cp.partition_stripe(T, K, LazyFlip(LOC, eps), phi, backend=hip)
        assert np.array_equal(pi.spl, lfm.lazy_flip_bisect(T, K, LOC, phi, eps)[0])
        assert np.array_equal(Pi.spl, pi.spl) and np.array_equal(Phi.spl, phi.spl)
        Pi4, Phi4 = cp.partition_plaid(A, K, cp.AlternatingPartitioner(Lazy(NET, eps), LazyFlip(LOC, eps), Lazy(COMM, eps), LazyFlip(LOC, eps)),
                                       adj_A=T, backend=hip)
        phi2 = cp.partition_stripe(A, K, Lazy(COMM, eps), pi, backend=hip)
        pi2 = cp.partition_stripe(T, K, LazyFlip(LOC, eps), phi2, backend=hip)
        assert np.array_equal(pi2.spl, lfm.lazy_flip_bisect(T, K, LOC, phi2, eps)[0])
        assert np.array_equal(Pi4.spl, pi2.spl) and np.array_equal(Phi4.spl, phi2.spl)
