"""Self-checks of tests/sym_model.py (the pure-Python statement of the symmetric cost family) and of the host mirror's three
model classes.  No GPU."""
import numpy as np
import pytest

import sym_model as sm
from util import cp, sprand, golden_matrices


def _with_diag(A, keep):
    """A with the diagonal entries of the columns in `keep` added"""
    D = sm._dense(A)
    for j in keep:
        D[j, j] = True
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=A.n))]).astype(np.int64)
    return cp.SparseMatrixCSC(A.n, A.n, colptr, rows.astype(np.int64) + 1)


def test_model_classes_exist_and_evaluate():
    s = cp.AffineSymmetricConnectivityModel(1, 2, 3, 4, 5)
    m = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)
    k = cp.AffineMonotonizedSymmetricConnectivityModel(alpha=0, beta_vertex=0, beta_over_pin=1, beta_dia_net=100, delta_pins=90)
    e = cp.AffineSymmetricEdgeCutModel(1, 2, 3, 4)
    assert (s.kind, m.kind, e.kind) == (10, 11, 12)
    assert s(2, 3, 4, 5) == 1 + 4 + 9 + 16 + 25 and m(2, 3, 4) == 403 and e(2, 3, 4) == 1 + 4 + 9 + 16
    assert m._params() == k._params() == [0, 0, 1, 100, 90]
    assert m.dtype == cp.models.CP_I64 and cp.AffineSymmetricEdgeCutModel(0, 0.5, 1, 1).dtype == cp.models.CP_F64
    f = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90, alpha_k=[3, 1, 2])
    assert f(0, 0, 0, 2) == 1 and f.marshal().struct.n_alpha_k == 3
    st = m.marshal().struct
    assert st.kind == 11 and list(st.p_i64) == [0, 0, 1, 100, 90]


def test_converting_constructor_both_branches():
    # beta_vertex < beta_remote_net (:21-23): Delta_pins = cld(b_remote - b_vertex, b_pin), beta_vertex = 0
    m = cp.AffineMonotonizedSymmetricConnectivityModel(cp.AffineSymmetricConnectivityModel(7, 10, 3, 0, 100))
    assert m._params() == [7, 0, 3, 100, 30] and m.dtype == cp.models.CP_I64          # cld(90, 3) = 30
    m = cp.AffineMonotonizedSymmetricConnectivityModel(cp.AffineSymmetricConnectivityModel(7, 10, 4, 0, 100))
    assert m._params() == [7, 0, 4, 100, 23]                                          # cld(90, 4) = 23
    # otherwise (:24-26): Delta_pins = 0, beta_vertex reduced
    m = cp.AffineMonotonizedSymmetricConnectivityModel(cp.AffineSymmetricConnectivityModel(7, 100, 3, 0, 40))
    assert m._params() == [7, 60, 3, 40, 0]
    m = cp.AffineMonotonizedSymmetricConnectivityModel(cp.AffineSymmetricConnectivityModel(0.0, 1.0, 0.5, 0.0, 2.25))
    assert m._params() == [0.0, 0.0, 0.5, 2.25, 3.0] and m.dtype == cp.models.CP_F64  # cld(1.25, 0.5) = 3.0


def test_new_kinds_need_the_hip_backend(orc):
    A = sprand(6, 6, 0.4, np.random.default_rng(1))
    m = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2)
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.partition_stripe(A, 2, cp.DynamicBottleneckSplitter(m), backend=orc)
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.bound_stripe(A, 2, m, backend=orc)
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.dianetcount(A, backend=orc)
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.pack_stripe(A, cp.DynamicTotalChunker(m), backend=orc)
    with pytest.raises(NotImplementedError, match="HIP backend only"):
        cp.pack_stripe_batch(A, [cp.ConvexTotalChunker(cp.ConstrainedCost(m, cp.VertexCount(), 3))], backend=orc)


def test_bisect_index_chain_reaches_the_dp_optimum():
    rng = np.random.default_rng(9)
    for A in (sprand(40, 40, 0.1, rng), golden_matrices()["Pajek/GD99_c"]):
        T = sm.Tables(A)
        for mdl in (cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2), cp.AffineMonotonizedSymmetricConnectivityModel(5, 1, 2, 3, 0)):
            for K in (1, 2, 5):
                spl, _ = sm.bisect_index(T, K, mdl)
                _check_spl(spl, A.n, K)
                assert sm.objective(T, mdl, spl, "max") == sm.dp_partition(T, mdl, K, "max")[1]


def test_count_tables_against_set_definitions():
    rng = np.random.default_rng(5)
    for A in (sprand(9, 9, 0.3, rng), sprand(1, 1, 0.5, rng), sprand(12, 12, 0.0, rng)):
        D = sm._dense(A); n = A.n
        dn, sp = sm.dianet_table(A), sm.selfpin_table(A)
        for p in range(n + 1):
            for r in range(p, n + 1):
                rows = set(np.nonzero(D[:, p:r].any(axis=1))[0].tolist()) | set(range(p, r))
                assert dn[p, r] == len(rows)
                assert sp[p, r] == int(D[p:r, p:r].sum())


def test_bound_forms_agree_on_full_diagonal_and_zero_delta():
    """ocl(1, n+1) equals the model-form c_hi only where dianet(1, n+1) == m and overpos == pos: full diagonal, Delta_pins = 0"""
    rng = np.random.default_rng(6)
    for A0 in (sprand(17, 17, 0.2, rng), golden_matrices()["Pajek/GD99_c"]):
        A = _with_diag(A0, range(A0.n))
        T = sm.Tables(A)
        for mdl in (cp.AffineMonotonizedSymmetricConnectivityModel(3, 2, 1, 100, 0), cp.AffineMonotonizedSymmetricConnectivityModel(0.5, 0.25, 1.5, 10.0, 0.0)):
            for K in (1, 3, 7):
                assert sm.bound_stripe_model(A, K, mdl) == sm.bound_stripe_oracle(T, K, mdl)


def _check_spl(spl, n, K):
    assert len(spl) == K + 1 and spl[0] == 1 and spl[K] == n + 1 and all(spl[k] <= spl[k + 1] for k in range(K))


@pytest.mark.parametrize("eps", [0.01, 0.5])
def test_lazy_and_bisect_within_eps_of_the_dp_optimum(eps):
    rng = np.random.default_rng(7)
    mats = [sprand(40, 40, 0.1, rng), _with_diag(sprand(33, 33, 0.15, rng), range(0, 33, 2)), golden_matrices()["Pajek/GD99_c"]]
    for A in mats:
        T = sm.Tables(A)
        for mdl in (cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2), cp.AffineMonotonizedSymmetricConnectivityModel(5, 1, 2, 3, 0)):
            for K in (1, 2, 5):
                _, opt = sm.dp_partition(T, mdl, K, "max")
                for spl, probes in (sm.lazy_bisect(A, K, mdl, eps), sm.bisect_cost(T, K, mdl, eps)):
                    _check_spl(spl, A.n, K)
                    got = sm.objective(T, mdl, spl, "max")
                    assert opt <= got <= (1 + eps) * opt, (K, got, opt)
