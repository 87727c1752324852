"""Self-checks of tests/plaid_cut_model.py (the pure-Python statement of the plaid edge-cut costs) on the properties the reference
tests (test/test_Costs.jl:50-103), and of the host mirror: the two model classes and their dispatch.  No GPU."""
import numpy as np
import pytest

import plaid_cut_model as pc
import sym_model as sm
from util import cp, sprand

TRIPLES = [(0, 0, 0, 1), (0, 0, 1, 1), (1, 1, 1, 1)]          # test_Costs.jl:58-63


def _adjoint(A):
    D = sm._dense(A)
    rows, cols = np.nonzero(D)                                # entries of the adjoint: column = row of A, sorted by (row of A, column of A)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(rows, minlength=A.m))]).astype(np.int64)
    return cp.SparseMatrixCSC(A.n, A.m, colptr, cols.astype(np.int64) + 1)


def _rand_split(rng, n, K):
    return cp.SplitPartition(K, np.concatenate([[1], np.sort(rng.integers(1, n + 2, K - 1)), [n + 1]]).astype(np.int64))


def _cases():
    rng = np.random.default_rng(20)
    for n in (1, 2, 7, 23, 40):
        for K in (1, 2, 4):
            yield sprand(n, n, 0.125, rng), _rand_split(rng, n, K), _rand_split(rng, n, K), K


def test_model_classes_exist_and_marshal():
    p = cp.AffinePrimaryEdgeCutModel(1, 2, 3, 4)
    s = cp.AffineSecondaryEdgeCutModel(alpha=1, beta_vertex=2, beta_self_pin=3, beta_cut_pin=4)
    assert (p.kind, s.kind) == (13, 14) and p.needs_rowpart and s.needs_rowpart
    assert p(2, 3, 4) == s(2, 3, 4) == 1 + 4 + 9 + 16
    assert p.dtype == cp.models.CP_I64 and cp.AffinePrimaryEdgeCutModel(0, 0.5, 1, 1).dtype == cp.models.CP_F64
    f = cp.AffineSecondaryEdgeCutModel(0, 1, 1, 1, alpha_k=[3, 1, 2])
    assert f(0, 0, 0, 2) == 1 and f.marshal().struct.n_alpha_k == 3
    st = p.marshal().struct
    assert st.kind == 13 and list(st.p_i64)[:4] == [1, 2, 3, 4]


def test_duality_of_the_pair():
    """bottleneck_value(adj_A, Phi, Pi, secondary) == bottleneck_value(A, Pi, Phi, primary)   (test_Costs.jl:77)"""
    for A, Pi, Phi, K in _cases():
        T = _adjoint(A)
        for a, bv, bs, bc in TRIPLES + [(3, 2, 5, 1)]:
            prim = pc.Cut(A, Pi, cp.AffinePrimaryEdgeCutModel(a, bv, bs, bc))
            sec = pc.Cut(T, Phi, cp.AffineSecondaryEdgeCutModel(a, bv, bs, bc))
            for g in ("max", "sum"):
                assert pc.objective(sec, Pi.spl, g) == pc.objective(prim, Phi.spl, g)


def test_bounds_bracket_the_bottleneck():
    """0 <= c_lo <= value <= c_hi, both models, both secondary forms   (test_Costs.jl:73-76)"""
    for A, Pi, Phi, K in _cases():
        T = _adjoint(A)
        for a, bv, bs, bc in TRIPLES:
            pm, smd = cp.AffinePrimaryEdgeCutModel(a, bv, bs, bc), cp.AffineSecondaryEdgeCutModel(a, bv, bs, bc)
            lo, hi = pc.bound_primary(A, K, pm)
            assert 0 <= lo <= pc.objective(pc.Cut(A, Pi, pm), Phi.spl, "max") <= hi
            v = pc.objective(pc.Cut(T, Phi, smd), Pi.spl, "max")
            for lo, hi in (pc.bound_secondary_model(T, K, Phi, smd), pc.bound_secondary_oracle(T, K, Phi, smd)):
                assert 0 <= lo <= v <= hi
    # the two forms differ when b_self_pin > b_cut_pin: the model form's "lower" bound is then the larger one
    A, Pi, Phi, K = list(_cases())[-1]
    m = cp.AffineSecondaryEdgeCutModel(1, 1, 5, 2)
    assert pc.bound_secondary_model(_adjoint(A), K, Phi, m) != pc.bound_secondary_oracle(_adjoint(A), K, Phi, m)


def test_primary_with_one_partition_is_the_symmetric_edge_cut():
    """Pi == Phi: the self pins are the nonzeros of the diagonal blocks   (test_Costs.jl:88-102)"""
    for A, Pi, _, K in _cases():
        T = sm.Tables(A)
        for a, bv, bs, bc in TRIPLES + [(2, 1, 7, 3)]:
            C = pc.Cut(A, Pi, cp.AffinePrimaryEdgeCutModel(a, bv, bs, bc))
            for g in ("max", "sum"):
                assert pc.objective(C, Pi.spl, g) == sm.objective(T, cp.AffineSymmetricEdgeCutModel(a, bv, bs, bc), Pi.spl, g)


def _holes(n, rng):
    A = sprand(n, n, 0.15, rng)
    D = sm._dense(A)
    D[:, rng.random(n) < 0.4] = False                         # empty columns
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, rows.astype(np.int64) + 1)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_scan_formulation_equals_the_literal_dp(K):
    rng = np.random.default_rng(30 + K)
    for n in (1, 5, 40):
        A = _holes(n, rng)
        Pi = _rand_split(rng, n, 4)
        Pm = cp.MapPartition(4, rng.integers(1, 4, n).astype(np.int64))       # in no order, part 4 empty
        models = [cp.AffinePrimaryEdgeCutModel(1, 0, 0, 0), cp.AffineSecondaryEdgeCutModel(1, 0, 0, 0),      # all ties
                  cp.AffinePrimaryEdgeCutModel(3, 2, 1, 7), cp.AffineSecondaryEdgeCutModel(3, 2, 9, 4),
                  cp.AffinePrimaryEdgeCutModel(2, -1, 5, -3), cp.AffinePrimaryEdgeCutModel(0.0, 1.0, 2.0, 6.0),
                  cp.AffineSecondaryEdgeCutModel(0, 1, 2, 5, alpha_k=[4, 0, 9, 1])]
        for mdl in models:
            for P in ([Pi] if type(mdl).__name__.startswith("AffineSecondary") else [Pi, Pm]):
                spl, csts, ptrs = pc.dp(pc.Cut(A, P, mdl), K, "sum")
                spl2, csts2, ptrs2 = pc.dp_scan(A, P, mdl, K)
                assert np.array_equal(spl, spl2)
                for k in range(K):
                    assert np.array_equal(csts[k], csts2[k]) and np.array_equal(ptrs[k], ptrs2[k]), (n, k, type(mdl).__name__)


def test_bisect_index_reaches_the_dp_bottleneck_for_a_monotone_cost():
    rng = np.random.default_rng(40)
    A = sprand(30, 30, 0.2, rng)
    Pi = _rand_split(rng, 30, 3)
    for K in (1, 2, 3):
        C = pc.Cut(A, Pi, cp.AffinePrimaryEdgeCutModel(1, 1, 2, 3))
        lo, hi = pc.bisect_bounds(C, K)
        spl = pc.bisect_index(C.f, A.n, K, lo, hi)
        assert pc.objective(C, spl, "max") == pc.dp(C, K, "max")[1][-1][A.n]
        # the secondary cost with b_self_pin < b_cut_pin does not grow with the range: the Flip variant is the one that applies
        S = pc.Cut(A, Pi, cp.AffineSecondaryEdgeCutModel(1, 1, 1, 4))
        lo, hi = pc.bisect_bounds(S, K)
        spl = pc.bisect_index(S.f, A.n, K, lo, hi, flip=1)
        assert spl[0] == 1 and spl[-1] == A.n + 1 and np.all(np.diff(spl) >= 0)
        assert pc.objective(S, spl, "max") == pc.dp(S, K, "max")[1][-1][A.n]


# ---------------------------------------------------------------- host dispatch
class _Stub:
    """a backend that records what reaches it"""
    name = "hip"

    def __init__(self):
        self.calls = []

    def partition_dynamic(self, A, K, combine, order, mm, rp, wm, wi, wf, spl):
        self.calls.append(("dynamic", mm.struct.kind, rp))
        spl[:] = 1
        return 0

    def partition_bisect_cost(self, A, K, mm, eps, flip, spl, rp=None):
        self.calls.append(("bisect_cost", mm.struct.kind, rp))
        return 0

    def partition_bisect_index(self, A, K, mm, flip, spl, rp=None):
        self.calls.append(("bisect_index", mm.struct.kind, rp))
        return 0

    def bound_stripe(self, A, K, mm):
        self.calls.append(("bound", mm.struct.kind, None))
        return 0, 0, 0

    def bound_stripe_pi(self, A, K, rp, mm):
        self.calls.append(("bound_pi", mm.struct.kind, rp))
        return 0, 0, 0


def test_host_dispatch_passes_the_row_partition():
    A = sprand(6, 6, 0.4, np.random.default_rng(1))
    Pi = cp.SplitPartition(2, [1, 4, 7])
    for mdl in (cp.AffinePrimaryEdgeCutModel(1, 1, 1, 1), cp.AffineSecondaryEdgeCutModel(1, 1, 1, 1)):
        b = _Stub()
        cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(mdl), Pi, backend=b)
        cp.partition_stripe(A, 2, cp.BisectCostBottleneckSplitter(mdl, 0.1), Pi, backend=b)
        cp.partition_stripe(A, 2, cp.FlipBisectIndexBottleneckSplitter(mdl), Pi, backend=b)
        assert [c[0] for c in b.calls] == ["dynamic", "bisect_cost", "bisect_index"]
        for _, kind, rp in b.calls:
            assert kind == mdl.kind and rp is not None and rp.K == 2
        cp.bound_stripe(A, 2, mdl, Pi, backend=b)
        assert b.calls[-1][0] == ("bound_pi" if mdl.kind == 14 else "bound")


def test_new_kinds_need_the_hip_backend(orc):
    A = sprand(6, 6, 0.4, np.random.default_rng(1))
    Pi = cp.SplitPartition(2, [1, 4, 7])
    for mdl in (cp.AffinePrimaryEdgeCutModel(1, 1, 1, 1), cp.AffineSecondaryEdgeCutModel(1, 1, 1, 1)):
        name = type(mdl).__name__
        with pytest.raises(NotImplementedError, match=f"{name} is implemented by the HIP backend only, not by backend 'oracle'"):
            cp.partition_stripe(A, 2, cp.DynamicTotalSplitter(mdl), Pi, backend=orc)
        with pytest.raises(NotImplementedError, match="HIP backend only"):
            cp.bound_stripe(A, 2, mdl, Pi, backend=orc)
        with pytest.raises(NotImplementedError, match="HIP backend only"):
            cp.bottleneck_value(A, Pi, mdl, Pi, backend=orc)
        with pytest.raises(NotImplementedError, match="HIP backend only"):
            cp.oracle_stripe(cp.NoHint(), mdl, A, Pi, backend=orc)
    # the message of the symmetric models is what it was
    with pytest.raises(NotImplementedError, match="AffineSymmetricEdgeCutModel is implemented by the HIP backend only, not by backend 'oracle'"):
        cp.bound_stripe(A, 2, cp.AffineSymmetricEdgeCutModel(1, 1, 1, 1), backend=orc)
