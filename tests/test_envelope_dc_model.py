"""CPU checks of the divide-and-conquer total DP of the envelope model (tests/envelope_dc_model.py) against the literal DP of
tests/envelope_model.py: every cst / ptr cell and the split vector, with leaf blocks of 2, 4 and 8 rows so that sizes up to 40
have up to five upper levels, truncated last nodes and right halves of a single row; the range-minimum structure against a
scan; the host-side gate."""
import numpy as np

import envelope_dc_model as dc
import envelope_model as em
from util import cp

ENV = cp.AffineEnvelopeModel


def from_cols(m, cols):
    colptr = np.concatenate([[1], 1 + np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rowval = np.array([r for c in cols for r in c], dtype=np.int64)
    return cp.SparseMatrixCSC(m, len(cols), colptr, rowval)


def random_pattern(rng, m, n, dens, p_empty):
    cols = []
    for _ in range(n):
        rows = np.nonzero(rng.random(m) < dens)[0] + 1
        cols.append([] if rng.random() < p_empty else rows.tolist())
    return from_cols(m, cols)


def models(rng, K):
    ak = [int(v) for v in rng.integers(-3, 6, K)]
    return [ENV(0, 10, 1, 100), ENV(0, 0, 0, 0), ENV(0, 1, -1, 2), ENV(3, -2, 1, -1), ENV(1, 1, 2, 3, alpha_k=ak), ENV(0, 0, 0, 1),
            ENV(0.0, 10.0, 1.0, 100.0), ENV(2.0, -1.0, 3.0, -2.0, alpha_k=[float(v) for v in ak])]


def check(A, mdl, K, leaf, counts=None):
    E = em.Env(A, mdl)
    assert dc.dc_ok(mdl, A.m, A.n, A.nnz, K)
    spl, cst, ptr = em.dp_literal(E, K, "sum")
    gs, gc, gp = dc.dp_dc(E, K, leaf, counts)
    assert np.array_equal(gp, ptr) and np.array_equal(gc, cst) and np.array_equal(gs, spl), (A.n, K, leaf, mdl._params())


def test_range_minimum_returns_the_rightmost_argument():
    rng = np.random.default_rng(1)
    for B in (2, 4, 8, 64):
        for nb in (1, 2, 3, 5, 8):
            key = rng.integers(0, 4, nb * B).astype(np.int64)  # (few values: many ties)
            R = dc.Rmq(key, B)
            for x in range(key.size):
                for y in range(x, key.size):
                    w = key[x:y + 1]
                    assert R.query(x, y) == x + w.size - 1 - int(np.argmin(w[::-1])), (B, nb, x, y)


def test_every_cell_matches_the_literal_dp():
    rng = np.random.default_rng(2)
    cases, counts = 0, {}
    sizes = [1, 2, 3, 4, 7, 8] + [int(v) for v in rng.integers(5, 41, 32)]      # n + 1 in 2, 3, 4, 5, 8, 9 and n up to 40
    for t, n in enumerate(sizes):
        m = 1 if t % 7 == 3 else int(rng.integers(2, 30))
        A = random_pattern(rng, m, n, float(rng.choice([0.1, 0.3, 0.6])), float(rng.choice([0.0, 0.3, 0.7])))
        if t % 9 == 5:
            A = from_cols(m, [[] for _ in range(n)])           # no entry at all
        for K in (1, 2, n + 2, 3 + t % 3):
            for mdl in models(rng, K)[::1 if n <= 9 else 2] if K > 2 else models(rng, K)[:2]:
                check(A, mdl, K, (2, 4, 8)[(t + K) % 3], counts)
                cases += 1
    assert cases >= 400, cases
    tot = np.sum([c for c in counts.values()], axis=0)
    assert len(counts) >= 4 and all(tot > 1000), counts       # every regime, at several levels


def test_device_leaf_size():
    """leaf = 64 as the device runs it: one upper level with a right half of a single row, and a truncated last node"""
    rng = np.random.default_rng(3)
    for n in (128, 200):
        A = random_pattern(rng, 40, n, 0.1, 0.3)
        for mdl in (ENV(0, 10, 1, 100), ENV(0, 1, -1, 2)):
            check(A, mdl, 3, 64)


def test_gate():
    ok = lambda mdl, K: dc.dc_ok(mdl, 50, 64, 300, K)
    assert not ok(ENV(0.5, 0.25, 0.1, 1.7), 4)                 # non-integral Float64: the regrouped sums round differently
    assert not ok(ENV(0.0, 1.0, 1.0, 1.0, alpha_k=[0.0, 0.5]), 4)
    assert not ok(ENV(0.0, float("inf"), 1.0, 1.0), 4)
    assert not ok(ENV(2 ** 58, 1, 1, 1), 4) and ok(ENV(2 ** 58, 1, 1, 1), 3)
    assert ok(ENV(0, 1, -1, 2), 4) and ok(ENV(0, -1, -1, -1), 4) and ok(ENV(0.0, 10.0, -1.0, 100.0), 4)
    assert ok(ENV(2.0 ** 48, 1.0, 1.0, 1.0), 4) and not ok(ENV(2.0 ** 49, 1.0, 1.0, 1.0), 4)      # 2^51 for Float64
    assert not ok(ENV(0, 0, 0, 2 ** 53), 4) and ok(ENV(0, 0, 0, 2 ** 53), 1)                     # the net term enters once per part: 50 * 2^53 * K


def test_non_integral_float_differs_somewhere():
    """why the gate refuses them: with a non-integral Float64 model the regrouped arithmetic misses cells of the literal tables"""
    rng = np.random.default_rng(4)
    bad = 0
    for _ in range(20):
        A = random_pattern(rng, 20, 30, 0.3, 0.2)
        E = em.Env(A, ENV(0.5, 0.25, 0.1, 1.7))
        _, cst, ptr = em.dp_literal(E, 4, "sum")
        _, gc, gp = dc.dp_dc(E, 4, 4)
        bad += not (np.array_equal(gc, cst) and np.array_equal(gp, ptr))
    assert bad > 0
