"""pack_stripe(A, DynamicTotalChunker(...)) for any width or monotone work budget: the on-line divide and conquer of
csrc/chunk_lws.hip against the CPU oracle and the one-wave kernel (cp_set_option("lws", 0) / "force_brute"), its tables
(pack_stripe_tables), its routing (profile slot chunk_lws) and one run at the bench shape."""
import time

import numpy as np
import pytest

from util import cp, sprand, golden_matrices, suitesparse_shaped, banded

pytestmark = pytest.mark.gpu

L = 512             # rows per leaf wave (cp_set_option("lws_leaf") default)

MODELS = [cp.AffineConnectivityModel(0, 0, 0, 1), cp.AffineConnectivityModel(0, 3, 1, 3), cp.AffineConnectivityModel(-7, 0, 0, 1),
          cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0), cp.AffineWorkModel(0, 0, 0), cp.AffineWorkModel(-3, 1, 0),
          cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3)]


def mats(seed):
    rng = np.random.default_rng(seed)
    out = [sprand(m, n, p, rng) for (m, n, p) in [(1, 1, 0.5), (2, 3, 0.5), (8, 16, 0.3), (12, 31, 0.15), (20, 40, 0.1), (30, 65, 0.08)]]
    g = golden_matrices()
    out += [g["LPnetlib/lpi_itest6"], g["Pajek/GD99_c"], g["LPnetlib/lp_blend"]]
    out += [suitesparse_shaped(200, 4, 7), banded(150, 3, 0.5, 3), suitesparse_shaped(1500, 6, 11), banded(2100, 4, 0.4, 5)]
    return out


def weights(A):
    n = A.n
    deg = np.diff(A.colptr)
    budget = int(max(deg.max(initial=0), A.nnz // 8, 1))
    out = [None]
    ws = [(cp.VertexCount(), w) for w in sorted({1, 2, 17, 63, 64, 65, max(n // 4, 1), max(n, 1)})]
    ws += [(cp.AffineWorkModel(0, 0, 1), budget), (cp.AffineWorkModel(0, 1, 1), budget + max(n // 8, 1)), (cp.AffineWorkModel(0, 1, 0), max(n // 3, 1))]
    return out + ws


def chunker(f, wt):
    return cp.DynamicTotalChunker(f if wt is None else cp.ConstrainedCost(f, wt[0], wt[1]))


def lws_launches(hip):
    return hip.prof_get()["chunk_lws"]["launches"]


def test_split_vectors_equal_the_oracle(hip, orc):
    for A in mats(21):
        for f in MODELS:
            for wt in weights(A):
                meth = chunker(f, wt)
                got = cp.pack_stripe(A, meth, backend=hip)
                want = cp.pack_stripe(A, meth, backend=orc)
                assert got == want, (A, f, wt)
                if wt is not None and isinstance(wt[0], cp.VertexCount):
                    assert np.all(np.diff(got.spl) <= wt[1])


def test_tables_equal_the_one_wave_kernel(hip):
    for n in (1, 2, 63, 64, 65, L - 1, L, L + 1, 4097, 20000):
        A = suitesparse_shaped(n, 5, n) if n % 2 else banded(n, 4, 0.5, n)
        fs = [cp.AffineConnectivityModel(0, 0, 0, 1), cp.AffineWorkModel(-3, 1, 0), cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3),
              cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0)]
        wts = [(cp.VertexCount(), max(n // 4, 17)), (cp.AffineWorkModel(0, 1, 1), int(A.nnz // 6 + 40))]
        if n <= 4097:
            wts.append(None)
        for f in fs:
            for wt in wts:
                meth = chunker(f, wt)
                cst, spl = cp.pack_stripe_tables(A, meth, backend=hip)
                hip.set_option("force_brute", 1)
                try:
                    cst0, spl0 = cp.pack_stripe_tables(A, meth, backend=hip)
                finally:
                    hip.set_option("force_brute", 0)
                assert spl[0] == 0 and spl0[0] == 0
                assert np.array_equal(spl, spl0), (n, f, wt)
                assert np.array_equal(cst, cst0), (n, f, wt)
                P = cp.pack_stripe(A, meth, backend=hip)
                assert cst[n] == cp.total_value(A, P, f, backend=hip), (n, f, wt)


def test_routing(hip, orc):
    rng = np.random.default_rng(5)
    A = sprand(40, 300, 0.03, rng)
    f = cp.AffineConnectivityModel(0, 3, 1, 3)
    hip.prof_enable(True)
    try:
        for wt in [(cp.VertexCount(), 17), (cp.VertexCount(), 100), (cp.AffineWorkModel(0, 0, 1), 30), (cp.AffineWorkModel(0, 1, 0), 40), None]:
            hip.prof_reset()
            got = cp.pack_stripe(A, chunker(f, wt), backend=hip)
            assert lws_launches(hip) > 0, wt
            assert got == cp.pack_stripe(A, chunker(f, wt), backend=orc)
        wide = (cp.VertexCount(), 100)
        cb = cp.ColumnBlockComponentCostModel(3, lambda w: 1 + w)
        per_part = cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[5, 1, 9, 2, 7])
        wrapped = cp.AffineConnectivityModel(0, 1 << 58, 1, 3)
        cases = [("lws", f, wide), ("force_brute", f, wide), (None, cb, wide), (None, per_part, wide), (None, wrapped, wide),
                 (None, f, (cp.VertexCount(), 16))]
        for opt, g, wt in cases:
            if opt == "lws":
                hip.set_option("lws", 0)
            elif opt == "force_brute":
                hip.set_option("force_brute", 1)
            try:
                hip.prof_reset()
                got = cp.pack_stripe(A, chunker(g, wt), backend=hip)
                assert lws_launches(hip) == 0, (opt, g, wt)
            finally:
                hip.set_option("lws", 1)
                hip.set_option("force_brute", 0)
            assert got == cp.pack_stripe(A, chunker(g, wt), backend=orc), (opt, g, wt)
    finally:
        hip.prof_enable(False)


def test_infeasible_budget_same_error(hip):
    _marshal = cp.api._marshal
    rng = np.random.default_rng(9)
    A = sprand(30, 200, 0.05, rng)
    deg = int(np.diff(A.colptr).max())
    f = cp.AffineConnectivityModel(0, 3, 1, 3)
    for wt in [(cp.AffineWorkModel(0, 0, 1), deg - 1), (cp.AffineWorkModel(0, 1, 1), deg), (cp.AffineWorkModel(5, 1, 0), 4),
               (cp.VertexCount(), 0), (cp.VertexCount(), -3)]:
        codes = []
        for lws in (1, 0):
            hip.set_option("lws", lws)
            try:
                mdl, mm, wm, wi, wf, rp, keep = _marshal(A, cp.ConstrainedCost(f, wt[0], wt[1]), None)
                spl = np.zeros(A.n + 1, dtype=np.int64)
                Kout = np.zeros(1, dtype=np.int64)
                codes.append(hip.pack_dynamic(A, mm, rp, wm, wi, wf, spl, Kout))
            finally:
                hip.set_option("lws", 1)
        assert codes[0] == codes[1] != 0, (wt, codes)
        with pytest.raises(AssertionError):
            cp.pack_stripe(A, chunker(f, wt), backend=hip)


def test_bench_shape_quarter_width(hip):
    import torch
    import synth
    n, N = 10_000_000, 100_000_000
    _, _, colptr, rowval = synth.suitesparse_shaped_t(n, N / n, 1, torch.device("cuda", 0), nnz=N)
    A = cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())
    del colptr, rowval
    f = cp.AffineConnectivityModel(0, 0, 0, 1)
    meth = cp.DynamicTotalChunker(cp.ConstrainedCost(f, cp.VertexCount(), n // 4))
    t0 = time.perf_counter()
    cst, spl = cp.pack_stripe_tables(A, meth, backend=hip)
    P = cp.pack_stripe(A, meth, backend=hip)
    dt = time.perf_counter() - t0
    assert dt < 240, dt
    assert P.spl[0] == 1 and P.spl[-1] == n + 1
    assert np.all(np.diff(P.spl) >= 1) and np.all(np.diff(P.spl) <= n // 4)
    assert cst[n] == cp.total_value(A, P, f, backend=hip)
