"""The executable specification of csrc/dp_total_budget.hip (tests/budget_model.py): the two-staircase decomposition covers every
feasible cell exactly once, the rightmost-argmin divide and conquer equals the brute-force row minimum (ties to the largest p) in
every full rectangle, and a whole K-layer run equals the oracle's constrained tables cell for cell."""
import numpy as np
import pytest

from util import cp, sprand, golden_matrices, suitesparse_shaped, banded
import brute
import budget_model as bm
import lws_model as lm

MODELS = [cp.AffineConnectivityModel(0, 0, 0, 1), cp.AffineConnectivityModel(0, 3, 1, 3), cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0),
          cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[5, 1, 9, 2, 7, 3, 8, 4]), cp.AffineWorkModel(-3, 1, 0),
          cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3)]


def patterns():
    rng = np.random.default_rng(2024)
    out = [sprand(m, n, p, rng) for (m, n, p) in [(1, 1, 0.5), (3, 5, 0.5), (8, 16, 0.3), (12, 31, 0.15), (20, 40, 0.1), (4, 8, 0.0)]]
    out += [suitesparse_shaped(65, 4, 7), banded(50, 3, 0.5, 3), golden_matrices()["LPnetlib/lpi_itest6"]]
    return out


def staircases(rng, n):
    """random non-decreasing a <= b <= r over the rows 0 .. n, with flat runs (a == b, jumps over several blocks) now and then"""
    b = np.minimum(np.sort(rng.integers(0, n + 1, size=n + 1)), np.arange(n + 1))
    b = np.maximum.accumulate(b)
    mode = int(rng.integers(0, 4))
    if mode == 0:
        a = b.copy()                                                    # a == b: one cell per row
    elif mode == 1:
        a = np.maximum.accumulate(np.minimum(np.sort(rng.integers(0, n + 1, size=n + 1)), b))
    elif mode == 2:
        a = np.maximum.accumulate(np.minimum((np.sort(rng.integers(0, 4, size=n + 1)) * (n // 3 + 1)), b))      # a few long jumps
    else:
        a = np.maximum(b - int(rng.integers(0, 6)), 0)
        a = np.maximum.accumulate(a)
    return [int(v) for v in a], [int(v) for v in b]


def cells_of(blocks, a, b):
    seen = {}
    for blk in blocks:
        if blk[0] == "rect":
            _, ja, jb, ra, rb = blk
            for r in range(ra, rb + 1):
                assert a[r] <= ja and jb <= b[r] and jb <= ra, "a rectangle must be full"
                for p in range(ja, jb + 1):
                    seen[(r, p)] = seen.get((r, p), 0) + 1
        else:
            _, ja, jb, rows = blk
            for r in rows:
                for p in range(max(a[r], ja), min(b[r], jb) + 1):
                    seen[(r, p)] = seen.get((r, p), 0) + 1
    return seen


def test_decomposition_covers_each_feasible_cell_once():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(0, 70))
        a, b = staircases(rng, n)
        rlo = int(rng.integers(0, n + 1)); rhi = int(rng.integers(rlo, n + 1))
        p_lo0 = int(rng.integers(0, n + 1)); p_hi0 = int(rng.integers(p_lo0, n + 1))
        if trial % 5 == 0:
            p_lo0, p_hi0 = 0, n
        if trial % 7 == 0 and n > 3:                                    # an empty range: rows that see nothing of the block
            rlo, rhi, p_lo0, p_hi0 = 0, n // 3, 2 * n // 3 + 1, n
        aa = {r: max(a[r], p_lo0) for r in range(rlo, rhi + 1)}
        bb = {r: min(b[r], p_hi0) for r in range(rlo, rhi + 1)}
        for stair in (1, 4, 1000):
            blocks = []
            bm.push_blocks(p_lo0, p_hi0, rlo, rhi, aa, bb, blocks, stair)
            seen = cells_of(blocks, aa, bb)
            want = {(r, p) for r in range(rlo, rhi + 1) for p in range(aa[r], bb[r] + 1)}
            assert set(seen) == want, (trial, stair)
            assert all(v == 1 for v in seen.values()), (trial, stair)
            if stair == 1:
                assert all(blk[0] == "rect" for blk in blocks)         # one-column blocks have no partial rows


def layer_costs(A, mdl, rng):
    """(W, F) of a layer k >= 2: W a real previous layer (the unconstrained layer 1 .. 2), F the cost table"""
    NT, ST = brute.net_table(A), brute.selfnet_table(A)
    F1 = brute.cost_table(A, mdl, 1, NT, ST)
    F2 = brute.cost_table(A, mdl, 2, NT, ST)
    W = F1[0, :].copy()
    if rng.integers(0, 2):
        W, _ = brute.layer(W, F2)
    return W, brute.cost_table(A, mdl, 3, NT, ST)


@pytest.mark.parametrize("mi", range(len(MODELS)))
def test_rightmost_argmin_divide_and_conquer_in_every_rectangle(mi):
    mdl = MODELS[mi]
    rng = np.random.default_rng(5 + mi)
    nrect = 0
    for A in patterns():
        n = A.n
        W, F = layer_costs(A, mdl, rng)
        val = lambda p, r: W[p] + F[p, r]
        for trial in range(6):
            a, b = staircases(rng, n)
            blocks = []
            bm.push_blocks(0, n, 0, n, dict(enumerate(a)), dict(enumerate(b)), blocks, stair=int(rng.choice([1, 4])))
            for blk in blocks:
                if blk[0] != "rect":
                    continue
                _, ja, jb, ra, rb = blk
                nrect += 1
                got = bm.rect_minima(ja, jb, ra, rb, val)
                prev = None
                for r in range(ra, rb + 1):
                    v = W[ja:jb + 1] + F[ja:jb + 1, r]
                    i = brute._rightmost_argmin(v)
                    assert got[r] == (v[i], ja + i), (A, mi, blk, r)
                    assert prev is None or ja + i <= prev, "the rightmost argmin must not increase with r"
                    prev = ja + i
    assert nrect > 50


WEIGHTS = [(0, 0, 1), (2, 3, 1), (0, 1, 2)]


@pytest.mark.parametrize("mi", range(len(MODELS)))
def test_k_layer_run_equals_the_oracle_tables(orc, mi):
    """thresholds shrunk (whole scans up to 8 cells / 4 columns, stair scans below 4 columns) so that n <= 65 meets rectangles,
    levels and stair scans"""
    mdl = MODELS[mi]
    feasible = infeasible = 0
    kinds = set()
    for A in patterns():
        n = A.n
        NT, ST = brute.net_table(A), brute.selfnet_table(A)
        tabs = {}
        F_of_k = lambda k: tabs.setdefault(k if mdl.alpha_k is not None else 0, brute.cost_table(A, mdl, k, NT, ST))
        typemax = np.iinfo(np.int64).max if mdl.dtype == cp.models.CP_I64 else np.inf
        for (a0, bv, bp) in WEIGHTS:
            wgt = cp.AffineWorkModel(a0, bv, bp)
            full = a0 + bv * n + bp * A.nnz
            for K in (1, 2, 5, 8):
                for frac in (1.0 / K, 1.5 / K, 0.5, 1.0, 0.0):
                    wmax = int(a0 + (full - a0) * frac + (1 if frac else 0))
                    rc2, lo2, hi2, p2, c2 = orc.dynamic_tables_constrained(A, K, 0, mdl.marshal(), None, wgt.marshal(), wmax, float(wmax))
                    j0 = lm.lo_budget(A, a0, bv, bp, wmax)
                    blocks = []
                    ok, lo1, hi1, p1, c1 = bm.run(n, K, F_of_k, j0, typemax, scan_cells=8, scan_cols=4, stair=4, blocks=blocks)
                    assert ok == (rc2 == 0), (A, K, wmax)
                    assert list(lo1) == lo2.tolist() and list(hi1) == hi2.tolist(), (A, K, wmax)
                    infeasible += not ok
                    if ok:
                        feasible += 1
                        kinds |= {blk[0] for blk in blocks}
                        assert np.array_equal(p1, p2), (A, K, wmax, mi)
                        assert np.array_equal(c1, c2), (A, K, wmax, mi)
    assert feasible > 100 and infeasible > 10 and kinds == {"rect", "stair"}
