"""partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AffinePrimaryConnectivityModel, eps), Pi) on the device
(csrc/lazy.hip, k_lazy_bisect in its primary mode; LazyBisectCostBottleneckSplitter.jl:390-483): the split vector and the number of probes are
those of tests/plaid_lazy_model.py, the reference's loop in pure Python."""
import ctypes as C
import functools

import numpy as np
import pytest

import plaid_lazy_model as plm
from util import cp, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu

M = cp.models
PRIM, SEC = cp.AffinePrimaryConnectivityModel, cp.AffineSecondaryConnectivityModel
Lazy = cp.LazyBisectCostBottleneckSplitter
COMM = PRIM(0, 10, 1, 0, 100)                       # runbenchmarks.jl:19, bin/test_table_bottleneck.jl:23


def from_dense(D):
    """D[row, col]"""
    m, n = D.shape
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


def pattern(m, n):
    """seeded, about four entries a column, with empty columns and empty rows"""
    rng = np.random.default_rng(1000 * n + m)
    D = rng.random((m, n)) < min(0.6, 4.0 / max(m, 1))
    if n > 2:
        D[:, rng.random(n) < 0.2] = False
    if m > 2:
        D[rng.random(m) < 0.2, :] = False
    return from_dense(D)


def split(m, K):
    """partition_stripe(A', K, EquiSplitter())"""
    k = np.arange(0, K + 1, dtype=np.int64)
    return cp.SplitPartition(K, k * (m // K) + np.minimum(m % K, k) + 1)


def cyclic(m, K):
    return cp.MapPartition(K, (np.arange(m, dtype=np.int64) % K) + 1)


def lazy(hip, A, K, mdl, Pi, eps):
    """the entry with its probe count, and partition_stripe through the dispatch: the same split vector"""
    from chainpartitioners_jl_amd import api
    rp, keep = api._rowpart(Pi)
    rc, spl, probes = hip.partition_lazy_bisect_cost_probes(A, K, mdl.marshal(), eps, rp)
    assert rc == 0, hip.last_error()
    assert np.array_equal(cp.partition_stripe(A, K, Lazy(mdl, eps), Pi, backend=hip).spl, spl)
    return spl, probes


def same_as_model(hip, A, K, mdl, Pi, eps, what=None):
    want, wp = plm.lazy_bisect(A, K, mdl, Pi, eps)
    spl, probes = lazy(hip, A, K, mdl, Pi, eps)
    assert np.array_equal(spl, want) and probes == wp, (what, A, K, type(Pi).__name__, Pi.K, mdl._params(), mdl.alpha_k, eps, spl, want, probes, wp)
    return spl, probes


def grid_models(K):
    return [PRIM(0, 2, 1, 3, 6), PRIM(0.25, 0.1, 0.7, 3.3, 1.9), PRIM(0, 2, 1, 3, 6, alpha_k=[1 + (7 * k) % 10 for k in range(K)])]


# ---------------------------------------------------------------- the basic grid
@pytest.mark.parametrize("mf", [0, 1, 3], ids=["m=1", "m=n", "m=3n"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_equals_the_literal_loop(hip, n, mf):
    m = max(1, mf * n)
    A = pattern(m, n)
    for K in (1, 2, 7, 32):
        for PK in sorted({K, (K + 1) // 2}):                          # Pi.K == K and Pi.K < K
            for Pi in (split(m, PK), cyclic(m, PK)):
                for mdl in grid_models(K):
                    for eps in (0.01, 0.5):
                        same_as_model(hip, A, K, mdl, Pi, eps)


# ---------------------------------------------------------------- the k-dependent restart
def restart_pattern():
    """12 rows in four parts of three; columns 1-3 hold one row of part 1 each, column 4 the three rows of part 3, columns 5-6 rows of
    part 3 again, columns 7-9 one row of part 4 each.  With b_local = 0 and b_remote = 100 column 4 costs 301 in parts 1, 2 and 4
    and 1 in part 3."""
    D = np.zeros((12, 9), dtype=bool)
    for c in range(3):
        D[c, c] = True
    D[6:9, 3] = True
    D[6, 4] = D[7, 5] = True
    for c in range(3):
        D[9 + c, 6 + c] = True
    return from_dense(D), split(12, 4)


def test_split_column_is_recounted_for_the_part_it_opens(hip):
    A, Pi = restart_pattern()
    mdl = PRIM(0, 1, 0, 0, 100)
    trace = []
    want, wp = plm.lazy_bisect(A, 4, mdl, Pi, 0.01, trace)
    # column 4 closes part 1, is too expensive as part 2 (its rows are remote there) and fits as part 3: parts 1-3 and an empty part 2
    assert want.tolist() == [1, 4, 4, 7, 10] and want[1] == want[2] and ("again", 4, 2) in trace
    spl, probes = lazy(hip, A, 4, mdl, Pi, 0.01)
    assert np.array_equal(spl, want) and probes == wp
    for m2 in (PRIM(0.0, 1.0, 0.0, 0.0, 100.0), PRIM(0, 1, 0, 0, 100, alpha_k=[0, 2, 0, 1])):
        same_as_model(hip, A, 4, m2, Pi, 0.01)
        same_as_model(hip, A, 4, m2, cp.MapPartition(4, plm._asg(Pi, 12)), 0.5)


def test_split_loop_runs_out_of_parts(hip):
    """K = 2, every row owned by part 1: columns 1-5 and 7-9 hold one row each, column 6 six rows.  At c = 565.2 (the fourth probe)
    column 6 closes part 1 (6 * 100 > c), costs 100 + 6 * 100 > c as part 2 as well, and k == K ends the probe inside the split
    loop, in its second pass (:441-443)."""
    D = np.zeros((14, 9), dtype=bool)
    for c in range(5):
        D[c, c] = True
    D[5:11, 5] = True
    for c in range(3):
        D[11 + c, 6 + c] = True
    A, Pi = from_dense(D), cp.MapPartition(2, [1] * 14)
    for mdl in (PRIM(0, 100, 0, 0, 100), PRIM(0.0, 100.0, 0.0, 0.0, 100.0)):
        trace = []
        want, wp = plm.lazy_bisect(A, 2, mdl, Pi, 0.01, trace)
        assert ("fail", 6, 2) in trace
        spl, probes = lazy(hip, A, 2, mdl, Pi, 0.01)
        assert np.array_equal(spl, want) and probes == wp


# ---------------------------------------------------------------- chunk boundaries
@functools.lru_cache(maxsize=None)
def big():
    A = suitesparse_shaped(3500, 12, 11)                      # nnz > 2 * 16384: splits fall inside chunks
    assert A.nnz > 2 * 16384
    return A


@functools.lru_cache(maxsize=None)
def regular(degs):
    """2100 x 2100 with 33600 entries: the column degrees are `degs`, repeated; the rows of a column are sorted distinct draws"""
    n = 2100
    rng = np.random.default_rng(2100 + sum(degs))
    deg = np.resize(np.array(degs, dtype=np.int64), n)
    colptr = np.concatenate([[1], 1 + np.cumsum(deg)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(n, size=d, replace=False)) + 1 for d in deg]).astype(np.int64)
    assert colptr[-1] - 1 == 33600
    return cp.SparseMatrixCSC(n, n, colptr, rows)


def deg16():
    """a chunk that starts at a column start holds exactly 1024 complete columns: the column batch fills every lane (and the loop
    goes round again with nothing left), and the last column ends at the end of the chunk"""
    return regular((16,))


def deg15_17():
    """column ends are odd: the restart behind a split begins inside an aligned 16-byte piece"""
    return regular((15, 17))


# (pattern, K); the ids of the cases on big() are their K
CHUNK_CASES = [pytest.param(big, 2, id="2"), pytest.param(big, 32, id="32"), pytest.param(deg16, 5, id="deg16"),
               pytest.param(deg15_17, 5, id="deg15_17")]


@pytest.mark.parametrize("pat, K", CHUNK_CASES)
def test_across_chunk_boundaries(hip, pat, K):
    A = pat()
    for Pi in (split(A.m, K), cyclic(A.m, (K + 1) // 2)):
        for mdl, eps in ((COMM, 0.01), (PRIM(0.5, 1.0, 0.25, 3.0, 7.5), 0.5)):
            spl, probes = same_as_model(hip, A, K, mdl, Pi, eps)
            assert probes > 0


@functools.lru_cache(maxsize=None)
def dense_column():
    """m = 20000; column 40 is dense (it spans two chunks, and its restart count runs over more entries than the block has lanes),
    the other 99 columns hold three rows each"""
    m, n = 20000, 100
    rng = np.random.default_rng(77)
    colptr, rows = [1], []
    for c in range(n):
        r = np.arange(m) if c == 39 else np.sort(rng.choice(m, 3, replace=False))
        rows.append(r); colptr.append(colptr[-1] + r.size)
    return cp.SparseMatrixCSC(m, n, np.array(colptr, dtype=np.int64), np.concatenate(rows).astype(np.int64) + 1)


@pytest.mark.parametrize("K", [3, 8])
def test_column_longer_than_a_chunk(hip, K):
    A = dense_column()
    assert A.colptr[40] - A.colptr[39] > 16384
    for Pi in (split(A.m, K), cyclic(A.m, K)):
        for mdl in (PRIM(0, 1000, 0, 1, 2), PRIM(0, 10, 1, 0, 100), PRIM(0, 1000, 0, 1, 2, alpha_k=list(range(1, K + 1)))):
            trace = []
            want, wp = plm.lazy_bisect(A, K, mdl, Pi, 0.01, trace)
            spl, probes = lazy(hip, A, K, mdl, Pi, 0.01)
            assert np.array_equal(spl, want) and probes == wp, (K, type(Pi).__name__, mdl._params(), spl, want, probes, wp)
            # the dense column closed a part in some probe, so its restart count ran; where pins are free it also ends up a boundary
            assert 40 in want[1:-1] or any(t[1] == 40 for t in trace)
            assert 40 in want[1:-1] or mdl.beta_pin != 0


# ---------------------------------------------------------------- no probe at all
def test_without_a_probe(hip):
    A = pattern(64, 64)
    mdl = PRIM(10**9, 0, 1, 1, 1)
    spl, probes = same_as_model(hip, A, 3, mdl, split(64, 3), 0.5)
    assert probes == 0 and list(spl) == [1, 65, 65, 65]


# ---------------------------------------------------------------- the reference's matrices, its benchmark's model
@pytest.mark.parametrize("name", sorted(golden_matrices()))
def test_reference_matrices_comm_model(hip, name):
    A = golden_matrices()[name]
    for K in (2, 32):
        for Pi in (split(A.m, K), cyclic(A.m, K)):
            same_as_model(hip, A, K, COMM, Pi, 0.01)


# ---------------------------------------------------------------- entry errors
def test_entry_errors(hip):
    from chainpartitioners_jl_amd import api
    A = pattern(40, 30)
    K = 3
    Pi = split(A.m, 3)
    rp, keep = api._rowpart(Pi)
    rp4, keep4 = api._rowpart(split(A.m, 4))
    mm = COMM.marshal()
    spl = np.zeros(K + 1, dtype=np.int64)
    pi_entry = lambda mm, rp: hip.lib.cp_partition_lazy_bisect_cost_pi(hip.csr(A), K, mm, rp, 0.1, spl, None)
    assert pi_entry(mm, rp) == M.CP_OK
    assert pi_entry(mm, None) == M.CP_EINVAL and "needs a row partition Pi" in hip.last_error()
    assert pi_entry(mm, rp4) == M.CP_EINVAL and "more parts than K" in hip.last_error()
    for bad in (PRIM(0, 10, 1, 0, -100), PRIM(0.0, 10.0, 1.0, -0.5, 100.0), PRIM(0, -1, 1, 0, 100)):
        assert pi_entry(bad.marshal(), rp) == M.CP_EINVAL and "beta >= 0" in hip.last_error()
    with pytest.raises(AssertionError, match="beta >= 0"):
        cp.partition_stripe(A, K, Lazy(PRIM(0, 10, -1, 0, 100), 0.1), Pi, backend=hip)
    # without Pi the call reaches the old export, which refuses the model as before
    with pytest.raises(AssertionError, match="the reference asserts on models that are not connectivity models"):
        cp.partition_stripe(A, K, Lazy(COMM, 0.1), backend=hip)
    # the secondary model stays refused exactly as before, with or without Pi
    for P in (Pi, None):
        with pytest.raises(AssertionError, match="the reference asserts on models that are not connectivity models"):
            cp.partition_stripe(A, K, Lazy(SEC(0, 10, 1, 0, 100), 0.1), P, backend=hip)
    assert pi_entry(SEC(0, 10, 1, 0, 100).marshal(), rp) == M.CP_EINVAL
    # the two old exports still answer CP_EINVAL for kind 8
    npr = C.c_int64()
    assert hip.lib.cp_partition_lazy_bisect_cost(hip.csr(A), K, mm, 0.1, spl) == M.CP_EINVAL
    assert hip.lib.cp_partition_lazy_bisect_cost_probes(hip.csr(A), K, mm, 0.1, spl, C.byref(npr)) == M.CP_EINVAL
    # every other kind: the _pi entry is cp_partition_lazy_bisect_cost_probes, Pi is not looked at
    conn = cp.AffineConnectivityModel(0, 10, 1, 100)
    n1 = np.zeros(1, dtype=np.int64)
    s1 = np.zeros(K + 1, dtype=np.int64)
    assert hip.lib.cp_partition_lazy_bisect_cost_pi(hip.csr(A), K, conn.marshal(), rp4, 0.1, s1, n1) == M.CP_OK
    rc, s2, n2 = hip.partition_lazy_bisect_cost_probes(A, K, conn.marshal(), 0.1)
    assert rc == 0 and np.array_equal(s1, s2) and int(n1[0]) == n2 > 0


# ---------------------------------------------------------------- the plaid caller
def test_plaid_alternating_partitioner(hip):
    """bin/test_table_bottleneck.jl:52"""
    net_model, loc_model = cp.AffineConnectivityModel(0, 10, 1, 100), SEC(0, 10, 1, 0, 100)
    eps, K = 0.1, 8
    Flip = cp.FlipBisectCostBottleneckSplitter
    for A in (golden_matrices()["HB/can_292"], golden_matrices()["LPnetlib/lp_blend"], pattern(120, 257)):
        Pi, Phi = cp.partition_plaid(A, K, cp.AlternatingPartitioner(Lazy(net_model, eps), Flip(loc_model, eps), Lazy(COMM, eps), Flip(loc_model, eps)),
                                     backend=hip)
        T = cp.adjointpattern(A, backend=hip)
        phi = cp.partition_stripe(A, K, Lazy(net_model, eps), backend=hip)
        pi = cp.partition_stripe(T, K, Flip(loc_model, eps), phi, backend=hip)
        phi2 = cp.partition_stripe(A, K, Lazy(COMM, eps), pi, backend=hip)
        want, _ = plm.lazy_bisect(A, K, COMM, pi, eps)
        assert np.array_equal(phi2.spl, want)
        pi2 = cp.partition_stripe(T, K, Flip(loc_model, eps), phi2, backend=hip)
        assert np.array_equal(Pi.spl, pi2.spl) and np.array_equal(Phi.spl, phi2.spl)
