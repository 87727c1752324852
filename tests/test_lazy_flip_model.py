"""LazyFlipBisectCostBottleneckSplitter (LazyBisectCostBottleneckSplitter.jl:72-138) without a GPU:

(i)  tests/lazy_flip_model.py, the statement the GPU test compares the kernels with, has the reference's own property
     (test_Partitioners.jl:145-150): from 1 to n + 1, sorted, and for decreasing costs a bottleneck value within (1 + eps) of the
     optimum -- here the optimum of a brute-force bottleneck DP over cost tables built from the definitions;
(ii) partition_stripe reaches the backend once, as partition_lazy_flip_bisect_cost(A, K, mm, eps, spl, rp), with Pi only for a model
     that needs one; a ConstrainedCost and a backend without the method are refused by name.
"""
import numpy as np
import pytest

import lazy_flip_model as lfm
from test_gpu_plaid_lazy import pattern, split
from util import cp

SEC, CONN, PRIM = cp.AffineSecondaryConnectivityModel, cp.AffineConnectivityModel, cp.AffinePrimaryConnectivityModel
LazyFlip = cp.LazyFlipBisectCostBottleneckSplitter
SHAPES = [(2, 2), (63, 63), (64, 64), (65, 65), (192, 64), (40, 65), (120, 40)]
KS = (1, 2, 3, 7)


def funky_conn(A, K):
    """test_Partitioners.jl:124"""
    r = np.random.default_rng(A.n + K).integers(1, 11, K)
    return CONN(0, -3, -1, -3, alpha_k=[int(1 + A.nnz + 3 * A.n + 3 * A.m + v) for v in r])


def check(A, K, mdl, Pi, eps):
    Fs = lfm.cost_tables(A, mdl, Pi, K)
    opt = lfm.bottleneck_optimum(Fs, K)
    spl, probes = lfm.lazy_flip_bisect(A, K, mdl, Pi, eps)
    what = (A, K, mdl._params(), mdl.alpha_k, eps, spl, probes)
    assert len(spl) == K + 1 and spl[0] == 1 and spl[-1] == A.n + 1 and np.all(np.diff(spl) >= 0), what
    assert lfm.bottleneck_value(Fs, spl) <= opt * (1 + eps), what


@pytest.mark.parametrize("m,n", SHAPES)
def test_secondary_models(m, n):
    A = pattern(m, n)
    for K in KS:
        Pi = split(m, K)
        for mdl in (SEC(0, 2, 1, 3, 6), SEC(0, 10, 1, 0, 100), SEC(0, 0, 0, 0, 1), SEC(5, 2, 1, 3, 3)):
            if K == 1 and lfm.bound_stripe(A, K, mdl, Pi)[0] == 0:
                continue                              # every probe succeeds and c_hi only halves: the reference loops (almost) forever
            for eps in (0.5, 0.1, 0.01):
                check(A, K, mdl, Pi, eps)


@pytest.mark.parametrize("m,n", SHAPES)
def test_funky_decreasing_connectivity(m, n):
    A = pattern(m, n)
    for K in KS:
        for eps in (0.1, 0.01, 0.0001):
            check(A, K, funky_conn(A, K), None, eps)


def test_secondary_tables_are_the_definition():
    """the secondary tables against the words of SecondaryConnectivityCosts.jl:82-89 on a few ranges"""
    A, K = pattern(40, 65), 3
    Pi = split(40, K)
    mdl = SEC(1, 2, 1, 3, 7)
    Fs = lfm.cost_tables(A, mdl, Pi, K)
    asg = lfm._asg(Pi, A.m)
    colrows = [[int(i) for i in A.rowval[A.colptr[c] - 1:A.colptr[c + 1] - 1]] for c in range(A.n)]
    for k in range(1, K + 1):
        rows = [i for i in range(1, A.m + 1) if asg[i - 1] == k]
        w = sum(1 for c in range(A.n) for i in colrows[c] if asg[i - 1] == k)
        d = sum(1 for c in range(A.n) if any(asg[i - 1] == k for i in colrows[c]))
        for p, r in ((0, 0), (0, A.n), (3, 17), (20, 21), (64, 65)):
            l = sum(1 for c in range(p, r) if any(asg[i - 1] == k for i in colrows[c]))
            assert Fs[k - 1][p, r] == mdl(len(rows), w, l, d - l, k)


def test_trace_names_the_control_flow():
    """the increasing model (0, 2, 1, 6, 3): c stays below c_hi = max_k f(1, 1, k), the least cost of the part that attains it, so that
    part never closes and every probe fails"""
    A = pattern(40, 65)
    trace = []
    spl, probes = lfm.lazy_flip_bisect(A, 3, SEC(0, 2, 1, 6, 3), split(40, 3), 0.5, trace)
    assert probes > 0 and ("exit", "fail") in trace and ("exit", "split") not in trace and list(spl) == [1, 66, 66, 66]


# ---------------------------------------------------------------- dispatch
class Stub:
    """a backend with exactly this method"""
    name = "hip"

    def __init__(self):
        self.calls = []

    def last_error(self):
        return ""

    def partition_lazy_flip_bisect_cost(self, *args):
        self.calls.append(args)
        return 0


class Bare:
    name = "bare"

    def last_error(self):
        return ""


A6 = cp.SparseMatrixCSC(4, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))
PI = cp.SplitPartition(3, [1, 2, 4, 5])


def test_dispatch_layout():
    b = Stub()
    cp.partition_stripe(A6, 3, LazyFlip(SEC(0, 1, 1, 2, 3), 0.25), PI, backend=b)
    (A, K, mm, eps, spl, rp), = b.calls
    assert A is A6 and K == 3 and eps == 0.25 and spl.dtype == np.int64 and spl.shape == (4,)
    assert mm.struct.kind == cp.models.CP_MODEL_SECONDARY and mm.rowpart is None          # no detour over the model
    assert isinstance(rp, cp.models.cp_rowpart_t) and rp.K == 3 and bool(rp.spl)


def test_row_partition_only_for_a_model_that_needs_it():
    for f, P, want in ((CONN(0, 1, 1, 2), PI, False), (CONN(0, 1, 1, 2), None, False), (PRIM(0, 1, 1, 2, 3), PI, True),
                       (PRIM(0, 1, 1, 2, 3), None, False)):
        b = Stub()
        cp.partition_stripe(A6, 3, LazyFlip(f, 0.5), P, backend=b)
        (args,) = b.calls
        assert len(args) == 6 and (args[5] is not None) == want and args[2].rowpart is None


def test_constrained_cost_is_refused():
    b = Stub()
    with pytest.raises(NotImplementedError, match="LazyFlipBisectCost on a ConstrainedCost has no method in the reference"):
        cp.partition_stripe(A6, 3, LazyFlip(cp.ConstrainedCost(CONN(0, 1, 1, 2), cp.VertexCount(), 4), 0.5), backend=b)
    assert b.calls == []


def test_backend_without_the_method_is_refused_by_name(orc):
    for b, name in ((Bare(), "bare"), (orc, orc.name)):
        with pytest.raises(NotImplementedError) as e:
            cp.partition_stripe(A6, 3, LazyFlip(CONN(0, 1, 1, 2), 0.5), backend=b)
        assert "partition_lazy_flip_bisect_cost" in str(e.value) and f"'{name}'" in str(e.value)


def test_exported():
    assert cp.LazyFlipBisectCostBottleneckSplitter is cp.models.LazyFlipBisectCostBottleneckSplitter
    assert not issubclass(LazyFlip, cp.LazyBisectCostBottleneckSplitter)
    from chainpartitioners_jl_amd import _lib
    assert "cp_partition_lazy_flip_bisect_cost" in _lib.SIGNATURES
