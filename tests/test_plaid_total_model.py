"""The gates of csrc/plaid_total.hip (plaid_total_ok / plaid_scan_exact, csrc/model.hpp) on the CPU, with cost tables built from the
definition of the two plaid connectivity costs (tests/plaid_total_model.py):

  primary    inside the gate (b_local_net >= 0 and b_remote_net >= 0) the two-staircase layer of tests/budget_model.py with j0 = 0 and
             the limits shrunk to 8 cells / 4 columns / 4 stair columns equals the literal layer in every (cst, ptr) cell; outside the
             gate it does not -- the gate is not vacuous;
  secondary  the prefix-min scan with the rightmost argmin equals the literal layer for b_local_net <, =, > b_remote_net."""
import numpy as np
import pytest

import brute
import plaid_total_model as ptm
from util import cp

PRIM, SEC = ptm.PRIM, ptm.SEC
IN_GATE = [(0, 10, 1, 0, 100), (3, -2, 1, 5, 40), (0, 0, 0, 1, 1), (0, 0, 0, 7, 0), (1, -3, -1, 2, 2), (0, 0, 0, 100, 1), (0, 0, 0, 0, 1)]
OUT_OF_GATE = [(0, 0, 0, -1, 1), (0, 0, 0, 1, -1), (0, 10, 1, -3, 100)]
SHRUNK = dict(scan_cells=8, scan_cols=4, stair=4)


def _pattern(m, n, density, rng):
    D = rng.random((m, n)) < density
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


def _map_with_an_empty_part(rng, m, K):
    asg = rng.integers(1, K + 1, m)
    asg[asg == 2] = 1                                 # part 2 owns nothing
    return cp.MapPartition(K, asg.astype(np.int64))


@pytest.fixture(scope="module")
def primaries():
    """seeded patterns, n in [2, 40), m != n, three densities, random MapPartitions of 4 parts with an empty one; counted once"""
    rng = np.random.default_rng(808)
    out = []
    for i in range(36):
        n = int(rng.integers(2, 40))
        m = n + int(rng.integers(1, 9)) * (1 if i % 2 else -1)
        m = max(m, 1) if m != n else n + 1
        A = _pattern(m, n, (0.05, 0.15, 0.4)[i % 3], rng)
        out.append(ptm.Primary(A, _map_with_an_empty_part(rng, m, 4)))
    return out


def layers_that_differ(T, mdl):
    """layers 2 .. 4: how many differ from the literal layer in some (cst, ptr) cell; the block kinds met"""
    W = T.table(mdl, 1)[0, :].copy()
    differ, kinds = 0, set()
    for k in (2, 3, 4):
        F = T.table(mdl, k)
        blocks = []
        got = ptm.stm.layer(W, F, blocks=blocks, **SHRUNK)
        cst, ptr = brute.layer(W, F)
        kinds |= {blk[0] for blk in blocks}
        differ += any(got[r] != (cst[r], ptr[r]) for r in range(F.shape[0]))
        W = cst
    return differ, kinds


@pytest.mark.parametrize("prm", IN_GATE)
def test_primary_inside_the_gate_every_cell_equals_the_literal_layer(primaries, prm):
    kinds = set()
    for T in primaries:
        differ, k = layers_that_differ(T, PRIM(*prm))
        assert differ == 0, (T.A, prm)
        kinds |= k
    assert kinds == {"rect", "stair"}


@pytest.mark.parametrize("prm", OUT_OF_GATE)
def test_primary_gate_is_not_vacuous(primaries, prm):
    assert sum(layers_that_differ(T, PRIM(*prm))[0] for T in primaries) >= 1


def test_primary_tables_come_from_the_definition():
    """one hand-checked cell per count: 3 rows, 3 columns, owners (1, 2, 1)"""
    A = cp.SparseMatrixCSC(3, 3, [1, 3, 4, 6], [1, 2, 2, 1, 3])
    T = ptm.Primary(A, cp.MapPartition(2, [1, 2, 1]))
    assert T.pins[0, 3] == 5 and T.nets[0, 3] == 3 and T.local[1][0, 3] == 2 and T.local[2][0, 3] == 1
    assert T.nets[1, 2] == 1 and T.local[2][1, 2] == 1 and T.local[1][1, 2] == 0
    assert T.table(PRIM(1, 10, 100, 1000, 10000), 2)[0, 3] == 1 + 30 + 500 + 1000 + 20000


@pytest.mark.parametrize("prm", [(3, 2, 1, 1, 7), (3, 2, 1, 4, 4), (0, -1, 2, 9, 2), (0, 0, 0, 0, 1), (0, 0, 0, -2, 3), (1.0, 2.0, 0.0, 5.0, 40.0)],
                         ids=["local_lt_remote", "equal", "local_gt_remote", "remote_only", "negative_local", "float64"])
def test_secondary_scan_equals_the_literal_layer(prm):
    rng = np.random.default_rng(909)
    mdl = SEC(*prm)
    for i in range(30):
        n = int(rng.integers(2, 40))
        m = n + 1 + int(rng.integers(0, 9))
        A = _pattern(m, n, (0.05, 0.15, 0.4)[i % 3], rng)
        Pi = cp.SplitPartition(4, np.concatenate([[1], np.sort(rng.integers(1, m + 2, 3)), [m + 1]]).astype(np.int64))
        S = ptm.Secondary(A, Pi)
        W = S.table(mdl, 1)[0, :].copy()
        for k in (2, 3, 4):
            cst, ptr = brute.layer(W, S.table(mdl, k))
            c2, p2 = ptm.scan_layer(W, S, mdl, k)
            assert np.array_equal(c2, cst) and np.array_equal(p2, ptr), (A, Pi.spl, k)
            W = cst


def test_secondary_tables_come_from_the_definition():
    A = cp.SparseMatrixCSC(3, 3, [1, 3, 4, 6], [1, 2, 2, 1, 3])
    S = ptm.Secondary(A, cp.SplitPartition(2, [1, 3, 4]))            # rows 1, 2 | row 3
    assert S.nv == {1: 2, 2: 1} and S.w == {1: 4, 2: 1} and S.d == {1: 3, 2: 1}
    assert S.prefix(2).tolist() == [0, 0, 0, 1]
    # part 2 and the first two columns: neither holds row 3 -> 0 local, 1 remote; the last two: column 3 does -> 1 local, 0 remote
    assert S.table(SEC(1, 10, 100, 1000, 10000), 2)[0, 2] == 1 + 10 + 100 + 0 + 10000
    assert S.table(SEC(1, 10, 100, 1000, 10000), 2)[1, 3] == 1 + 10 + 100 + 1000 + 0


# ---------------------------------------------------------------- PrimaryCols: rows and columns against the dense tables
@pytest.mark.parametrize("part", ["split", "map"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_primary_rows_and_columns_equal_the_dense_tables(n, part):
    """every row, every column and windows with frm > 1 / upto < n + 1, for all in-gate models of the GPU file, the alpha_k model, a
    Float64 twin and a part number past Pi.K"""
    import test_gpu_plaid_total as g
    T = g.counts(n, part)
    A, Pi = T.A, T.Pi
    rng = np.random.default_rng(n)
    windows = [(int(a), int(b)) for a, b in np.sort(rng.integers(1, n + 2, (6, 2)), axis=1)] + [(1, 1), (n + 1, n + 1), (2, n + 1), (1, n)]
    cases = [(m, k) for m in g.MODELS["i"] for k in (1, 5)] + [(g.MODELS["i"][1], Pi.K + 1), (g.MODELS["f"][1], 2)]
    cases += [(g.MODELS["ak"][0], k) for k in (1, 3, 7)]
    C = ptm.PrimaryCols(A, Pi)
    for k in (1, 4, 5, Pi.K + 1):                                               # the counts themselves (5 / 4: the empty part of split / none)
        loc = T.local[k] if k in T.local else np.zeros_like(T.nets)
        for j in range(1, n + 2):
            nets, l = C.counts_row(j - 1, k)
            assert np.array_equal(nets, T.nets[j - 1, j - 1:]) and np.array_equal(l, loc[j - 1, j - 1:]), (k, j)
            nets, l = C.counts_col(j - 1, k)
            assert np.array_equal(nets, T.nets[:j, j - 1]) and np.array_equal(l, loc[:j, j - 1]), (k, j)
    for mdl, k in cases:
        F, C = T.table(mdl, k), ptm.PrimaryCols(A, Pi, mdl)
        for j in range(1, n + 2):
            row, col = C.row(j, k), C.column(j, k)
            assert row.dtype == F.dtype and np.array_equal(row, F[j - 1, j - 1:]), (mdl._params(), k, j)
            assert col.dtype == F.dtype and np.array_equal(col, F[:j, j - 1]), (mdl._params(), k, j)
        for a, b in windows:
            assert np.array_equal(C.row(a, k, upto=b), F[a - 1, a - 1:b]) and np.array_equal(C.column(b, k, frm=a), F[a - 1:b, b - 1]), (a, b)


def test_secondary_columns_equal_the_table():
    rng = np.random.default_rng(910)
    A = _pattern(45, 37, 0.15, rng)
    S = ptm.Secondary(A, cp.SplitPartition(4, np.array([1, 9, 9, 30, 46], dtype=np.int64)))
    for mdl in (SEC(3, 2, 1, 1, 7), SEC(0.0, 1.0, 1.0, 5.0, 2.0, alpha_k=[5.0, 1.0, 9.0, 2.0])):
        for k in (1, 2, 4):
            F = S.table(mdl, k)
            for jp in range(1, A.n + 2):
                col = S.column(mdl, jp, k)
                assert col.dtype == F.dtype and np.array_equal(col, F[:jp, jp - 1]), (k, jp)
