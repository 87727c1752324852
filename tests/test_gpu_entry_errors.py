"""The C entry points of the one-wave methods (csrc/seq.hip), the bisections (csrc/bisect.hip) and LazyBisectCost (csrc/lazy.hip):
what a wrong call gets -- the exception class the status maps to and the message text -- and one Int64 and one Float64 result per
entry against the CPU oracle; then cp_objective and cp_bound_stripe per element type.  One 8 x 8 pattern with 20 nonzeros (no
empty column, so a part budget of 0 is smaller than any column's weight).

Expected statuses and strings are those of the library before its entry points were rewritten over one skeleton.  Where a case
cannot reach the library it is left out: the bisections take no weight (ConstrainedCost is refused in Python), and a batch takes
width limits 1 .. 15 only, so its refusal of w_max = 0 is the entry's own."""
import numpy as np
import pytest

import sym_model as sm
from util import cp

pytestmark = pytest.mark.gpu

N = 8
ROWS = [[1, 2], [1, 3, 8], [2, 3], [4], [3, 4, 5], [5, 6, 7], [1, 6], [2, 7, 8, 5]]      # rows of column j (1-based), 20 nonzeros
A = cp.SparseMatrixCSC(N, N, np.cumsum([1] + [len(r) for r in ROWS]), np.array([i for r in ROWS for i in sorted(r)], dtype=np.int64))
K = 3
F_I = cp.AffineConnectivityModel(0, 3, 1, 3)
F_F = cp.AffineConnectivityModel(-0.5, 0.25, 0.0, 1.0)
SYM = cp.AffineSymmetricConnectivityModel(3, 2, 1, 5, 40)
NO_PATH = "the symmetric cost models have no device path in this method"


def chunks_of_table(spl):
    """unravel_chunks! (DynamicChunker.jl:58-75) of the table pack_stripe_tables returns (index j' - 1)"""
    out, jp = [N + 1], N + 1
    while jp != 1:
        jp = int(spl[jp - 1]); out.append(jp)
    return out[::-1]


# name -> (call(f, backend) -> split vector as a list, the oracle's call or None: the same call on the oracle backend)
def _pack(Meth):
    return lambda f, b: cp.pack_stripe(A, Meth(f), backend=b).spl.tolist()


def _part(Meth, *a):
    return lambda f, b: cp.partition_stripe(A, K, Meth(f, *a), backend=b).spl.tolist()


SEQ = {
    "pack_dynamic": (_pack(cp.DynamicTotalChunker), None),
    "pack_dynamic_tables": (lambda f, b: chunks_of_table(cp.pack_stripe_tables(A, cp.DynamicTotalChunker(f), backend=b)[1]), _pack(cp.DynamicTotalChunker)),
    "pack_convex": (_pack(cp.ConvexTotalChunker), None),
    "pack_convex_batch": (lambda f, b: cp.pack_stripe_batch(A, [cp.ConvexTotalChunker(f)], backend=b)[0].spl.tolist(), _pack(cp.ConvexTotalChunker)),
    "partition_convex": (_part(cp.ConvexTotalSplitter), None),
    "pack_concave": (_pack(cp.ConcaveTotalChunker), None),
    "partition_concave": (_part(cp.ConcaveTotalSplitter), None),
    "dyn_constrained": (_part(cp.DynamicTotalSplitter), None),
}
BISECT = {
    "bisect_cost": (_part(cp.BisectCostBottleneckSplitter, 0.01), None),
    "flip_bisect_cost": (_part(cp.FlipBisectCostBottleneckSplitter, 0.01), None),
    "bisect_index": (_part(cp.BisectIndexBottleneckSplitter), None),
    "flip_bisect_index": (_part(cp.FlipBisectIndexBottleneckSplitter), None),
    "lazy_bisect": (_part(cp.LazyBisectCostBottleneckSplitter, 0.01), None),
}
ENTRIES = {**SEQ, **BISECT}


def budget(f, w_max=4, w=None):
    return cp.ConstrainedCost(f, w if w is not None else cp.VertexCount(), w_max)


def arg_of(name, f):
    """the batch takes width-constrained requests only, and the one-wave constrained DP is reached through a budget of pins"""
    if name == "pack_convex_batch":
        return budget(f)
    if name == "dyn_constrained":
        return budget(f, 9, cp.AffineWorkModel(0, 0, 1))
    return f


def raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_symmetric_model_is_refused(hip, name):
    # the one-wave methods say so themselves; the bisections fail in bound_stripe, which has no method for this model
    # (test_gpu_symmetric.py); the lazy entry takes connectivity models only and, as the reference, asserts on the others
    exc, text = {"dyn_constrained": (NotImplementedError, "ConstrainedCost over a symmetric cost model has no device path"),
                 "lazy_bisect": (AssertionError, "the reference asserts on models that are not connectivity models")}.get(
        name, (NotImplementedError, NO_PATH if name in SEQ else "bound_stripe has no method for this model"))
    raises(exc, text, lambda: ENTRIES[name][0](arg_of(name, SYM), hip))


@pytest.mark.parametrize("name", [k for k in SEQ if k != "pack_convex_batch"])
def test_weight_that_is_no_width_or_work_model_is_refused(hip, name):
    text = "weight must be VertexCount or an AffineWorkModel" if name == "dyn_constrained" else "bad argument"
    raises(AssertionError, text, lambda: SEQ[name][0](budget(F_I, 4, cp.AffineConnectivityModel(0, 1, 0, 1)), hip))


@pytest.mark.parametrize("name,exc,text", [
    ("pack_dynamic", AssertionError, "pack_stripe: a single column exceeds w_max (@assert j0 < j')"),
    ("pack_dynamic_tables", AssertionError, "pack_stripe: a single column exceeds w_max (@assert j0 < j')"),
    ("pack_convex", AssertionError, "ConvexTotalChunker: a single column exceeds w_max"),
    ("pack_convex_batch", NotImplementedError, "a batch takes width limits 1 .. 15"),
])
def test_budget_below_one_column(hip, name, exc, text):
    raises(exc, text, lambda: SEQ[name][0](budget(F_I, 0), hip))
    if name != "pack_convex_batch":                     # ... and under a work budget of pins (every column has at least one)
        raises(exc, text, lambda: SEQ[name][0](budget(F_I, 0, cp.AffineWorkModel(0, 0, 1)), hip))


def test_budget_below_one_column_concave(hip, orc):
    """the concave chunker does not refuse this budget: with every pair infeasible the oracle returns chunks of one column"""
    for g in (budget(F_I, 0), budget(F_I, 0, cp.AffineWorkModel(0, 0, 1))):
        assert SEQ["pack_concave"][0](g, hip) == SEQ["pack_concave"][0](g, orc) == list(range(1, N + 2))


@pytest.mark.parametrize("f", [F_I, F_F], ids=["int64", "float64"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_result_is_the_oracles(hip, orc, name, f):
    call, ref = ENTRIES[name]
    for g in ([arg_of(name, f)] if name in BISECT or name in ("pack_convex_batch", "dyn_constrained") else [f, budget(f, 3)]):
        assert call(g, hip) == (ref or call)(g, orc), (name, g)


@pytest.mark.parametrize("flt", [False, True], ids=["int64", "float64"])
def test_objective_and_bound_stripe(hip, orc, flt):
    c = float if flt else int
    spl = cp.SplitPartition(K, [1, 3, 6, 9])
    Pi = cp.SplitPartition(K, [1, 4, 6, 9])
    work, conn = cp.AffineWorkModel(c(2), c(3), c(1)), cp.AffineConnectivityModel(c(1), c(3), c(1), c(2))
    funky = cp.AffineConnectivityModel(c(0), c(3), c(1), c(2), alpha_k=[c(5), c(-2), c(40)])
    prim = cp.AffinePrimaryConnectivityModel(c(1), c(2), c(1), c(3), c(7))
    for mdl in (work, conn, funky):
        assert cp.total_value(A, spl, mdl, backend=hip) == cp.total_value(A, spl, mdl, backend=orc)
        assert cp.bottleneck_value(A, spl, mdl, backend=hip) == cp.bottleneck_value(A, spl, mdl, backend=orc)
        assert cp.bound_stripe(A, K, mdl, backend=hip) == cp.bound_stripe(A, K, mdl, backend=orc)
    assert cp.total_value(A, spl, prim, Pi, backend=hip) == cp.total_value(A, spl, prim, Pi, backend=orc)
    assert cp.bottleneck_value(A, spl, prim, Pi, backend=hip) == cp.bottleneck_value(A, spl, prim, Pi, backend=orc)
    assert cp.bound_stripe(A, K, prim, Pi, backend=hip) == cp.bound_stripe(A, K, prim, Pi, backend=orc)
    mono = cp.AffineMonotonizedSymmetricConnectivityModel(c(1), c(2), c(1), c(5), c(1))
    T = sm.Tables(A)
    assert cp.bound_stripe(A, K, mono, backend=hip) == sm.bound_stripe_model(A, K, mono)
    for combine, value in (("sum", cp.total_value), ("max", cp.bottleneck_value)):
        assert value(A, spl, mono, backend=hip) == sm.objective(T, mono, spl.spl, combine)
    with pytest.raises(AssertionError):                  # beta >= 0 (a NaN fails the Float64 test too)
        cp.bound_stripe(A, K, cp.AffineMonotonizedSymmetricConnectivityModel(c(1), c(2), c(-1), c(5), c(1)), backend=hip)
    if flt:
        with pytest.raises(AssertionError):
            cp.bound_stripe(A, K, cp.AffineMonotonizedSymmetricConnectivityModel(1.0, float("nan"), 1.0, 5.0, 1.0), backend=hip)
