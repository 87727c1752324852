"""The tiles of the long DP tasks at absolute 256-column blocks, run in column-block order (cp_set_option("own_blk", 1), the
default) against the tiles counted from each task's head, run in task order (own_blk 0): every per-block winner and count
(cp_dp_block_tables), the combined row, windowed layers and whole partitions must be bit-identical.  The shapes cover tasks
that start and end inside a block, tasks shorter than a block with tiles of their own (own_min 64), blocks of dense columns
(several times the mean number of link entries), the hyperedge model (a second entry list), the gap passes of round 6 (their
entry-by-entry walk of a tile needs the tile's first column), mispredicted layer sizes (the second layer on a handle is sized
from the first one's counts, under the other geometry) and poison mode."""
import numpy as np
import pytest
import torch

from util import cp, suitesparse_shaped, banded

pytestmark = pytest.mark.gpu

NET = cp.AffineConnectivityModel(1, 10, 1, 100)
HYP = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
MODELS = [cp.AffineConnectivityModel(0, 0, 0, 1), NET, cp.AffineWorkModel(0, 10, 1), HYP, cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0)]
DEFAULTS = {"own_blk": 1, "own_min": 64, "gap_tau": 6, "gap_min": 64, "block_tables": 0, "poison": 0, "nospec": 0, "dbg": 0}


def dense_columns(n, m, seed):
    """sparse columns (1-7 rows), plus two runs of dense ones: 400 columns of 24 rows, the last 300 columns of 20"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 8, n)
    deg[700:1100] = 24
    deg[n - 300:] = 20
    cols = np.repeat(np.arange(n), deg)
    rows = np.clip(cols * m // n + rng.integers(-m // 10, m // 10 + 1, cols.size), 0, m - 1)
    key = np.unique(cols.astype(np.int64) * m + rows)
    cols, rows = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows + 1)


def block_entries(A):
    cp_ = np.asarray(A.colptr) - 1
    n = len(cp_) - 1
    tops = np.minimum(np.arange(0, n + 1, 256) + 256, n)
    return cp_[tops] - cp_[np.arange(0, n + 1, 256)]


def w_rows(rng, n, scale, dt):
    # flat stretches with deep wells: arg-min staircases with wide gaps (long tasks, own tiles, gap passes, tiles with many
    # specials); a monotone row; a random one
    rows = [np.where(rng.random(n + 1) < 0.01, 0, scale * 8), np.where(rng.random(n + 1) < 0.002, 0, scale * 8),
            np.sort(rng.integers(0, scale + 1, n + 1)), rng.integers(0, scale + 1, n + 1)]
    return [np.ascontiguousarray(r).astype(dt) for r in rows]


def layer(hip, A, mdl, W, blocks):
    n = A.n
    dev = torch.device("cuda", 0)
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    dt = torch.int64 if mdl.dtype == cp.models.CP_I64 else torch.float64
    assert hip.set_option("block_tables", 1 if blocks else 0) == 0
    dp = hip.dp_begin(A, 3, 0, 0, mdl.marshal(), 1, n + 2)
    try:
        prev = torch.from_numpy(W).to(dev)
        cur = torch.zeros(n + 1, dtype=dt, device=dev)
        hip.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
        out = [cur.cpu().numpy(), hip.dp_ptr_row(dp, 2, n)]
        if blocks:
            out += [x for x in hip.dp_block_tables(dp, n, hyper)[1:] if x is not None]
        return out
    finally:
        hip.dp_destroy(dp)


def both(hip, fn):
    try:
        res = []
        for ob in (0, 1):
            assert hip.set_option("own_blk", ob) == 0
            res.append(fn())
        return res
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)


def assert_same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


MATS = [("shaped", lambda: suitesparse_shaped(3000, 8, 1)), ("banded", lambda: banded(2500, 6, 0.5, 3)),
        ("shaped_odd", lambda: suitesparse_shaped(1025, 5, 7)), ("dense", lambda: dense_columns(2600, 2000, 4))]


@pytest.mark.parametrize("mi", range(len(MATS)))
# (dbg 512: every gap tile is walked entry by entry by the SLOW gap kernels)
@pytest.mark.parametrize("opts", [{}, {"own_min": 1000}, {"gap_tau": -1}, {"gap_tau": 8, "gap_min": 8}, {"nospec": 1},
                                  {"dbg": 512, "gap_tau": 8, "gap_min": 8}])
def test_block_tables_equal_between_tile_geometries(hip, mi, opts):
    A = MATS[mi][1]()
    if MATS[mi][0] == "dense":
        assert block_entries(A).max() > 5000              # blocks of 256 columns with ~20 entries per column
    rng = np.random.default_rng(40 + mi)
    for mdl in MODELS:
        dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
        for W in w_rows(rng, A.n, 1000, dt):
            def run():
                for k, v in opts.items():
                    assert hip.set_option(k, v) == 0
                # a second layer on the same handle is sized from the first one's counts (speculative layers)
                return layer(hip, A, mdl, W, True) + layer(hip, A, mdl, W[::-1].copy(), False)
            r0, r1 = both(hip, run)
            assert_same(r0, r1, (MATS[mi][0], opts, mdl.kind))


def test_windowed_layers_equal_between_tile_geometries(hip):
    rng = np.random.default_rng(9)
    for A in [suitesparse_shaped(2000, 6, 5), dense_columns(2600, 2000, 6)]:
        n = A.n
        for mdl in (NET, HYP):
            for w in (63, 300, 777, n // 2, n):
                W = np.where(rng.random(n + 1) < 0.01, 0, 8000).astype(np.int64)
                r0, r1 = both(hip, lambda: list(hip.windowed_layer(A, mdl.marshal(), W, w)))
                assert_same(r0, r1, (n, w, mdl.kind))


def test_partitions_equal_between_tile_geometries_in_poison_mode(hip):
    mats = [suitesparse_shaped(6000, 8, 21), dense_columns(4000, 3000, 2)]
    for A in mats:
        n = A.n
        for K in (4, 9):
            for f in (NET, HYP, cp.ConstrainedCost(NET, cp.VertexCount(), -(-3 * n // (2 * K)))):
                def run():
                    assert hip.set_option("poison", 1) == 0
                    return cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
                r0, r1 = both(hip, run)
                assert r0 == r1, (n, K, type(f).__name__)
