"""Self-checks of tests/sym_model.py (the pure-Python statement of the symmetric cost family) and of the host mirror's three
model classes, and of Sym, its rows and columns of the count and cost tables that need no dense table (the referee of the GPU
tests past the literal tables' reach): every row, every column and windows of both against the dense tables.  No GPU."""
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


# ---------------------------------------------------------------- Sym: rows and columns against the dense tables
def _sym_models():
    import test_gpu_sym_total as g
    return [(m, None) for m in g.MODELS_IN] + [(g.MODELS_IN_F[0], None)] + [(m, k) for m in g.MODELS_AK for k in (1, 3)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_sym_rows_and_columns_equal_the_dense_tables(n):
    from test_gpu_symmetric import pattern, tables, VARIANTS
    rng = np.random.default_rng(n)
    for v in VARIANTS:
        A, T = pattern(n, v), tables(n, v)
        S = sm.Sym(A)
        windows = [(int(a), int(b)) for a, b in np.sort(rng.integers(1, n + 2, (6, 2)), axis=1)] + [(1, 1), (n + 1, n + 1), (2, n + 1), (1, n)]
        for name in ("dianet", "selfpin", "net"):
            D = T.get(name)
            for j in range(1, n + 2):
                assert np.array_equal(S.count_row(name, j), D[j - 1, j - 1:]), (v, name, j)
                assert np.array_equal(S.count_column(name, j), D[:j, j - 1]), (v, name, j)
            for a, b in windows:                                                # frm > 1 / upto < n + 1
                assert np.array_equal(S.count_row(name, a, upto=b), D[a - 1, a - 1:b]), (v, name, a, b)
                assert np.array_equal(S.count_column(name, b, frm=a), D[a - 1:b, b - 1]), (v, name, a, b)
        for mdl, k in _sym_models():
            F, S = sm.cost_table(T, mdl, k), sm.Sym(A, mdl)
            for j in range(1, n + 2):
                row, col = S.row(j, k), S.column(j, k)
                assert row.dtype == F.dtype and np.array_equal(row, F[j - 1, j - 1:]), (v, mdl._params(), k, j)
                assert col.dtype == F.dtype and np.array_equal(col, F[:j, j - 1]), (v, mdl._params(), k, j)
            for a, b in windows:
                assert np.array_equal(S.row(a, k, upto=b), F[a - 1, a - 1:b]) and np.array_equal(S.column(b, k, frm=a), F[a - 1:b, b - 1]), (v, a, b)


def test_sym_wraps_like_the_dense_table():
    from test_gpu_symmetric import pattern, tables
    A, T = pattern(65, "partial"), tables(65, "partial")
    mdl = cp.AffineSymmetricConnectivityModel(2**62, 2**61, 3, -2**60, 2**59)
    assert np.array_equal(sm.Sym(A, mdl).column(66), sm.cost_table(T, mdl)[:66, 65])
