"""LazyBisectCost for a primary connectivity model under a row partition (LazyBisectCostBottleneckSplitter.jl:390-483), without a GPU:

(i)  tests/plaid_lazy_model.py, the statement the GPU test compares the kernel with, has the reference's own property
     (test_Partitioners.jl:108-112): sorted, from 1 to n + 1, K parts, and a bottleneck value within (1 + eps) of the optimum --
     here the optimum of a brute-force bottleneck DP over cost tables built from tests/brute.py's definitions;
(ii) partition_stripe hands the row partition to the backend on the marshalled model (mm.rowpart) for a model that needs one,
     and refuses the pair by name on a backend that is not the HIP one.
"""
import ctypes as C

import numpy as np
import pytest

import plaid_lazy_model as plm
from util import cp, golden_matrices, sprand

PRIM = cp.AffinePrimaryConnectivityModel
EPS = (0.1, 0.01)
KS = (1, 2, 3, 4, 8)


def models(K, rng):
    return [PRIM(0, 2, 1, 3, 6), PRIM(0, 10, 1, 0, 100), PRIM(0, 2, 1, 3, 6, alpha_k=[int(v) for v in rng.integers(1, 11, K)])]


def partitions(A, K):
    """Pi = partition_stripe(A', K, EquiSplitter()) and the cyclic MapPartition of the rows (runbenchmarks.jl:67-79)"""
    m = A.m
    k = np.arange(0, K + 1, dtype=np.int64)
    return [cp.SplitPartition(K, k * (m // K) + np.minimum(m % K, k) + 1),
            cp.MapPartition(K, (np.arange(m, dtype=np.int64) % K) + 1)]


def check(A, K, rng):
    for Pi in partitions(A, K):
        for mdl in models(K, rng):
            Fs = plm.cost_tables(A, mdl, Pi, K)
            opt = plm.bottleneck_optimum(Fs, K)
            for eps in EPS:
                spl, probes = plm.lazy_bisect(A, K, mdl, Pi, eps)
                what = (A, K, type(Pi).__name__, mdl._params(), mdl.alpha_k, eps)
                assert len(spl) == K + 1 and spl[0] == 1 and spl[-1] == A.n + 1 and np.all(np.diff(spl) >= 0), what
                assert plm.bottleneck_value(Fs, spl) <= opt * (1 + eps), what


@pytest.mark.parametrize("name", sorted(golden_matrices()))
def test_reference_matrices(name):
    A = golden_matrices()[name]
    rng = np.random.default_rng(5)
    for K in KS:
        check(A, K, rng)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 8, 40])
def test_sprand_shapes(m):
    rng = np.random.default_rng(100 + m)
    for n in (1, 2, 3, 4, 8, 40):
        for p in (0.1, 0.5):
            A = sprand(m, n, p, rng)
            for K in KS:
                check(A, K, rng)


def test_cost_tables_are_the_objective_loop():
    """the tables against the literal loop of compute_objective (PrimaryConnectivityCosts.jl:94-125) on one split"""
    rng = np.random.default_rng(3)
    A = sprand(9, 12, 0.3, rng)
    K = 3
    colptr, rowval = A.colptr, A.rowval
    for Pi in partitions(A, K):
        asg = plm._asg(Pi, A.m)
        mdl = PRIM(1, 2, 1, 3, 7)
        Fs = plm.cost_tables(A, mdl, Pi, K)
        spl = [1, 4, 4, 13]
        hst = [0] * (A.m + 1)
        for k in range(1, K + 1):
            j, jp = spl[k - 1], spl[k]
            npins = nl = nr = 0
            for _j in range(j, jp):
                for q in range(int(colptr[_j - 1]), int(colptr[_j])):
                    i = int(rowval[q - 1])
                    npins += 1
                    if hst[i] < j:
                        if asg[i - 1] == k:
                            nl += 1
                        else:
                            nr += 1
                    hst[i] = j
            assert Fs[k - 1][j - 1, jp - 1] == mdl(jp - j, npins, nl, nr, k)


# ---------------------------------------------------------------- dispatch
class Recorder:
    """records every backend call and answers CP_OK"""

    def __init__(self, name):
        self.name, self.calls = name, []

    def last_error(self):
        return ""

    def __getattr__(self, meth):
        if meth.startswith("_"):
            raise AttributeError(meth)
        return lambda *args: self.calls.append((meth, args)) or 0


A6 = cp.SparseMatrixCSC(4, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))


@pytest.mark.parametrize("Pi", [cp.SplitPartition(2, [1, 3, 5]), cp.MapPartition(3, [3, 1, 2, 1])], ids=["split", "map"])
def test_row_partition_rides_on_the_marshalled_model(Pi):
    b = Recorder("hip")
    cp.partition_stripe(A6, 3, cp.LazyBisectCostBottleneckSplitter(PRIM(0, 1, 1, 2, 3), 0.25), Pi, backend=b)
    (meth, args), = b.calls
    assert meth == "partition_lazy_bisect_cost" and len(args) == 5                  # (A, K, mm, eps, spl): no sixth argument
    mm = args[2]
    assert isinstance(mm.rowpart, cp.models.cp_rowpart_t) and mm.rowpart.K == Pi.K
    asg = np.ctypeslib.as_array((C.c_int64 * A6.m).from_address(mm.rowpart.asg))
    assert asg.tolist() == cp.types.to_map(Pi).asg.tolist()
    assert bool(mm.rowpart.spl) == isinstance(Pi, cp.SplitPartition)
    assert any(a.ctypes.data == mm.rowpart.asg for a in mm.rowpart_keep)            # the buffers live as long as the model


def test_no_row_partition_on_the_model_without_need_or_without_pi():
    Pi = cp.SplitPartition(2, [1, 3, 5])
    for f, P in ((cp.AffineConnectivityModel(0, 1, 1, 2), Pi), (cp.AffineConnectivityModel(0, 1, 1, 2), None), (PRIM(0, 1, 1, 2, 3), None)):
        b = Recorder("hip")
        cp.partition_stripe(A6, 3, cp.LazyBisectCostBottleneckSplitter(f, 0.25), P, backend=b)
        (meth, args), = b.calls
        assert meth == "partition_lazy_bisect_cost" and len(args) == 5 and args[2].rowpart is None
    # the other methods keep passing Pi as an argument, never on the model
    b = Recorder("hip")
    cp.partition_stripe(A6, 3, cp.BisectCostBottleneckSplitter(PRIM(0, 1, 1, 2, 3), 0.25), Pi, backend=b)
    assert b.calls[0][1][2].rowpart is None and isinstance(b.calls[0][1][-1], cp.models.cp_rowpart_t)


def test_other_backends_refuse_the_pair_by_name():
    Pi = cp.SplitPartition(2, [1, 3, 5])
    b = Recorder("oracle")
    with pytest.raises(NotImplementedError) as e:
        cp.partition_stripe(A6, 3, cp.LazyBisectCostBottleneckSplitter(PRIM(0, 1, 1, 2, 3), 0.25), Pi, backend=b)
    assert str(e.value) == ("LazyBisectCostBottleneckSplitter(AffinePrimaryConnectivityModel) is implemented by the HIP backend only, "
                            "not by backend 'oracle'") and b.calls == []
    cp.partition_stripe(A6, 3, cp.LazyBisectCostBottleneckSplitter(cp.AffineConnectivityModel(0, 1, 1, 2), 0.25), Pi, backend=b)
    assert len(b.calls) == 1                                                        # (connectivity models still reach it)


def test_the_oracle_backend_is_refused(orc):
    with pytest.raises(NotImplementedError, match="is implemented by the HIP backend only, not by backend"):
        cp.partition_stripe(A6, 3, cp.LazyBisectCostBottleneckSplitter(PRIM(0, 1, 1, 2, 3), 0.25), cp.SplitPartition(2, [1, 3, 5]), backend=orc)


def test_hip_backend_picks_the_export_by_the_model():
    """HipBackend.partition_lazy_bisect_cost: the _pi export when mm.rowpart is set, the old one otherwise (no library needed)"""
    from chainpartitioners_jl_amd import _lib
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    hb = object.__new__(_lib.HipBackend)
    hb.lib = Lib()
    hb._h = lambda A: A
    spl = np.zeros(4, dtype=np.int64)
    mm = PRIM(0, 1, 1, 2, 3).marshal()
    hb.partition_lazy_bisect_cost("A", 3, mm, 0.5, spl)
    mm.rowpart = cp.models.cp_rowpart_t()
    hb.partition_lazy_bisect_cost("A", 3, mm, 0.5, spl)
    hb.partition_lazy_bisect_cost_probes("A", 3, mm, 0.5, mm.rowpart)
    assert [c[0] for c in calls] == ["cp_partition_lazy_bisect_cost", "cp_partition_lazy_bisect_cost_pi", "cp_partition_lazy_bisect_cost_pi"]
    assert calls[1][1][3] is mm.rowpart and calls[1][1][-1] is None
