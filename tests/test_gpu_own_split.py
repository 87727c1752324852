"""Own tiles that stream only their plane's variable link entries (cp_set_option("own_split", 1), the default; csrc/dp_total_own.hip,
SplitLinks) against the tiles that stream whole columns (own_split 0) and against brute force.

  * cp_test_own_split: the three device arrays equal the numpy specification (tests/own_split_model.py) exactly -- sizes around the
    first stored plane (n = 511, 512, 513), odd sizes, empty columns, a column of several 256-entry blocks, a one-row matrix;
  * layer parity (check_layer of tests/test_gpu_blocks.py: the combined row, every per-block winner and the counts stored with it
    against brute force) under own_split 1 and 0, for the connectivity, work (pin counts from the original column pointers), Float64
    and hyperedge models, under the driver options that change which tiles exist, and for row tiles;
  * cp_get_stat("own_split_tiles"): positive where the path must be taken, zero with the option off, for hyperedge costs and for
    windowed layers.

Off-diagonal guard: the winners off the diagonal (counted by brute force alone) must exceed 10 000 over the three mid-size matrices
(6 525 columns in all); every mid-size case asserts its share of that in proportion to its n, for every model."""
import numpy as np
import pytest

import own_split_model as osm
from test_gpu_blocks import check_layer, Tables, w_rows
from util import cp, sprand, suitesparse_shaped, banded

pytestmark = pytest.mark.gpu

CONN0 = cp.AffineConnectivityModel(0, 0, 0, 1)
NET = cp.AffineConnectivityModel(1, 10, 1, 100)
WORK = cp.AffineWorkModel(0, 10, 1)
CONNF = cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0)
HYP = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
MODELS = [("conn0", CONN0), ("net", NET), ("work", WORK), ("conn_f64", CONNF), ("hyp", HYP)]
DEFAULTS = {"own_split": 1, "own_blk": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0, "own_min": 64, "poison": 0, "block_tables": 0}


def dense_one(n, m, seed, col=777, deg=700):
    """sparse columns (1-6 rows) and one column of `deg` rows: its tile streams several 256-entry blocks"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 7, n)
    cols = np.repeat(np.arange(n), d)
    rows = np.clip(cols * m // n + rng.integers(-m // 8, m // 8 + 1, cols.size), 0, m - 1)
    cols = np.concatenate([cols, np.full(deg, col)])
    rows = np.concatenate([rows, rng.choice(m, deg, replace=False)])
    key = np.unique(cols.astype(np.int64) * m + rows)
    cols, rows = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows + 1)


def one_row(n, seed):
    rng = np.random.default_rng(seed)
    has = rng.random(n) < 0.4
    colptr = np.concatenate([[1], 1 + np.cumsum(has)]).astype(np.int64)
    return cp.SparseMatrixCSC(1, n, colptr, np.ones(int(has.sum()), dtype=np.int64))


MID = [("shaped3000", lambda: suitesparse_shaped(3000, 8, 1)), ("banded2500", lambda: banded(2500, 6, 0.5, 3)),
       ("shaped1025", lambda: suitesparse_shaped(1025, 5, 7))]
MID_COLUMNS = 3000 + 2500 + 1025
MATS = MID + [("shaped513", lambda: suitesparse_shaped(513, 6, 11)), ("dense_one", lambda: dense_one(1300, 1500, 4))]

DOWNLOAD = [("n511", lambda: suitesparse_shaped(511, 6, 31)), ("n512", lambda: suitesparse_shaped(512, 6, 32)),
            ("n513", lambda: suitesparse_shaped(513, 6, 11)), ("n1025", lambda: suitesparse_shaped(1025, 5, 7)),
            ("n3000", lambda: suitesparse_shaped(3000, 8, 1)), ("empty_columns", lambda: sprand(50, 700, 0.01, np.random.default_rng(3))),
            ("dense_one", lambda: dense_one(1300, 1500, 4)), ("one_row", lambda: one_row(600, 8))]


@pytest.mark.parametrize("name,make", DOWNLOAD)
def test_device_arrays_equal_the_specification(hip, name, make):
    A = make()
    if name == "empty_columns":
        assert np.any(np.diff(A.colptr) == 0)
    if name == "dense_one":
        assert np.diff(A.colptr).max() > 600
    nb, vpos, vsa, vnext = osm.split(A)
    assert nb >= 1
    gnb, gpos, gsa, gnext = hip.test_own_split(A)
    assert gnb == nb
    assert np.array_equal(gpos, vpos), name
    assert np.array_equal(gsa, vsa), name
    assert gnext.size == vnext.size and np.array_equal(gnext, vnext), name


def both(hip, A, T, mdl, rows_on, rows_off, opts=None, tile=None):
    """check_layer under own_split 1, then 0: (winners off the diagonal, split tiles with the option on, ... off)"""
    try:
        for k, v in (opts or {}).items():
            assert hip.set_option(k, v) == 0
        out = []
        for on, rows in ((1, rows_on), (0, rows_off)):
            assert hip.set_option("own_split", on) == 0
            assert hip.set_option("stat_reset", 1) == 0
            moved = check_layer(hip, A, T, mdl, rows, tile=tile)
            out.append((moved, hip.get_stat("own_split_tiles")))
        return out[0][0], out[0][1], out[1][1]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)


_tables = {}


def tables(mi):
    if mi not in _tables:
        _tables[mi] = Tables(MATS[mi][1]())
    return _tables[mi]


@pytest.mark.parametrize("mi", range(len(MATS)))
@pytest.mark.parametrize("ki", range(len(MODELS)))
def test_layer_parity_on_and_off(hip, mi, ki):
    T = tables(mi)
    A, mdl = T.A, MODELS[ki][1]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    rng = np.random.default_rng(800 + 10 * mi + ki)
    scale = int(abs(T.F(mdl, 2)).max()) + 1
    rows = w_rows(rng, A.n, scale, dt)
    moved, tiles_on, tiles_off = both(hip, A, T, mdl, rows, [rows[0], rows[5]])
    assert tiles_off == 0
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    if hyper:
        assert tiles_on == 0                                # the second entry list is not split: the tiles stream whole columns
    if mi < len(MID):
        assert moved * MID_COLUMNS > 10000 * A.n, (MATS[mi][0], MODELS[ki][0], moved)
        if not hyper:
            assert tiles_on > 0, (MATS[mi][0], MODELS[ki][0])


OPTION_SETS = [{"own_blk": 0}, {"gap_tau": -1}, {"gap_tau": 8, "gap_min": 8}, {"nospec": 1}, {"own_min": 1000}, {"poison": 1}]


@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_layer_parity_under_driver_options(hip, oi):
    """(gap_tau -1: tiles of plane 7, which stream whole columns, and split tiles in one launch)"""
    for mi, models in ((0, [NET]), (2, [NET, WORK])):
        T = tables(mi)
        A = T.A
        for k, mdl in enumerate(models):
            rng = np.random.default_rng(900 + 10 * oi + 3 * mi + k)
            scale = int(abs(T.F(mdl, 2)).max()) + 1
            rows = w_rows(rng, A.n, scale, np.int64)
            moved, tiles_on, tiles_off = both(hip, A, T, mdl, [rows[0], rows[2], rows[5]], [rows[5]], opts=OPTION_SETS[oi])
            assert tiles_off == 0 and 2 * moved * MID_COLUMNS > 10000 * A.n       # (half the rows of a mid-size case: half its share)
            if OPTION_SETS[oi] in ({"own_blk": 0}, {"gap_tau": -1}, {"nospec": 1}, {"poison": 1}):
                assert tiles_on > 0, (OPTION_SETS[oi], MATS[mi][0])


def test_row_tiles_with_injected_rows(hip):
    A = suitesparse_shaped(2000, 6, 5)
    T = Tables(A)
    n = A.n
    rng = np.random.default_rng(12)
    for mdl in (NET, WORK):
        scale = int(abs(T.F(mdl, 2)).max()) + 1
        for (lo, hi) in [(1, n // 3), (n // 3, n // 2 + 7), (n // 2 + 7, n + 2)]:
            rows = w_rows(rng, n, scale, np.int64)
            both(hip, A, T, mdl, [rows[0], rows[5]], [rows[5]], tile=(max(1, lo), hi))


def test_windowed_layers_take_no_split_tiles(hip):
    """a constrained partition runs windowed layers: their blocks are not the Fenwick blocks -- no split tiles, and the arrays are
    never built; both it and the unconstrained partition of the same matrix equal the partitions with the option off"""
    A = suitesparse_shaped(6000, 8, 21)
    n, K = A.n, 4
    try:
        res = {}
        for name, f in (("win", cp.ConstrainedCost(NET, cp.VertexCount(), -(-3 * n // (2 * K)))), ("free", NET)):
            for on in (1, 0):
                assert hip.set_option("own_split", on) == 0 and hip.set_option("stat_reset", 1) == 0
                res[name, on] = (cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip), hip.get_stat("own_split_tiles"))
        assert res["win", 1][1] == 0 and res["win", 0][1] == 0 and res["free", 0][1] == 0
        assert res["win", 1][0] == res["win", 0][0] and res["free", 1][0] == res["free", 0][0]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
