"""The gate of csrc/sym_total.hip (sym_total_ok, csrc/model.hpp) and its depth batching, on the CPU: inside the gate the two-staircase
layer of tests/budget_model.py with a(r) = 0, b(r) = r equals the literal layer on the cost tables of tests/sym_model.py in every
(cst, ptr) cell; outside the gate it does not; and the rectangles that one depth of the column tree contributes are pairwise
disjoint in rows and in columns, which is what lets the device run them in one launch sequence."""
import numpy as np
import pytest

import brute
import sym_model as sm
import sym_total_model as stm
from test_budget_model import cells_of
from util import cp

SC, MSC, SEC = cp.AffineSymmetricConnectivityModel, cp.AffineMonotonizedSymmetricConnectivityModel, cp.AffineSymmetricEdgeCutModel
# inside the gate: b_local_net >= 0 and b_remote_net >= b_local_net; b_dia_net >= 0; b_self_pin <= b_cut_pin
IN_GATE = [SC(3, -2, 1, 5, 40), SC(0, 0, 0, 0, 1), SC(0, 1, 0, 2, 2), MSC(0, 0, 1, 100, 2), MSC(1, -3, -1, 1, 0),
           SEC(1, 2, 3, 7), SEC(0, 0, 0, 1), SEC(0, -1, -2, -2)]
OUT_OF_GATE = [SC(0, 0, 0, 3, 1), MSC(0, 0, 1, -1, 2), SEC(0, 0, 1, 0)]
SHRUNK = dict(scan_cells=8, scan_cols=4, stair=4)


def _square(n, density, symmetric, rng):
    D = rng.random((n, n)) < density
    if symmetric:
        D |= D.T
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, rows.astype(np.int64) + 1)


@pytest.fixture(scope="module")
def count_tables():
    """seeded square patterns, n in [2, 40), three densities, every other one symmetrised; their count tables are built once"""
    rng = np.random.default_rng(424)
    out = []
    for i in range(60):
        n = int(rng.integers(2, 40))
        out.append(sm.Tables(_square(n, (0.05, 0.15, 0.4)[i % 3], i % 2 == 0, rng)))
    return out


def layers_that_differ(T, mdl):
    """layers 2 .. 4: (how many differ from the literal layer in some (cst, ptr) cell, how many ran, the block kinds met)"""
    F = sm.cost_table(T, mdl)
    W = F[0, :].copy()
    differ, kinds = 0, set()
    for k in (2, 3, 4):
        blocks = []
        got = stm.layer(W, F, blocks=blocks, **SHRUNK)
        cst, ptr = brute.layer(W, F)
        kinds |= {blk[0] for blk in blocks}
        differ += any(got[r] != (cst[r], ptr[r]) for r in range(F.shape[0]))
        W = cst
    return differ, 3, kinds


@pytest.mark.parametrize("mi", range(len(IN_GATE)))
def test_inside_the_gate_every_cell_equals_the_literal_layer(count_tables, mi):
    kinds = set()
    for T in count_tables:
        differ, ran, k = layers_that_differ(T, IN_GATE[mi])
        assert differ == 0, (T.A, IN_GATE[mi])
        kinds |= k
    assert kinds == {"rect", "stair"}


@pytest.mark.parametrize("mi", range(len(OUT_OF_GATE)))
def test_the_gate_is_not_vacuous(count_tables, mi):
    assert sum(layers_that_differ(T, OUT_OF_GATE[mi])[0] for T in count_tables) >= 1


@pytest.mark.parametrize("stair", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 300])
def test_rectangles_of_one_depth_are_disjoint_and_cover_the_triangle(n, stair):
    blocks, a, b = stm.triangle_blocks(n, stair)
    seen = cells_of(blocks, a, b)
    assert set(seen) == {(r, p) for r in range(n + 1) for p in range(r + 1)} and all(v == 1 for v in seen.values())
    groups = stm.by_depth(n, blocks)
    assert sorted(groups) == list(range(len(groups)))                    # every depth down to the leaves contributes
    for d, (rects, stairs) in groups.items():
        rows = [r for (_, ja, jb, ra, rb) in rects for r in range(ra, rb + 1)]
        cols = [p for (_, ja, jb, ra, rb) in rects for p in range(ja, jb + 1)]
        assert len(rows) == len(set(rows)) and len(cols) == len(set(cols)), (n, stair, d)
        srows = [r for (_, ja, jb, rr) in stairs for r in rr]            # the partial rows share their launch too
        assert len(srows) == len(set(srows)), (n, stair, d)
    assert len(groups) * (4 * int(np.ceil(np.log2(n + 1))) + 2) + 1 == stm.launch_cap(n, stair)


def test_last_layer_geometry():
    """layer K computes row n alone: the same tree, one cell column per block"""
    for n in (5, 65):
        blocks, a, b = stm.triangle_blocks(n, 4, rlo=n)
        seen = cells_of(blocks, a, b)
        assert set(seen) == {(n, p) for p in range(n + 1)} and all(v == 1 for v in seen.values())
