"""Split own tiles that read a column's start and prefix sum as one packed word (cp_set_option("own_pack", 1), the default;
csrc/dp_total_own.hip, SplitLinks::vpk / vbase, interior_stream<PK> of csrc/dp_total_stream.hpp) against the tiles that read the
two wide arrays (own_pack 0) and against brute force.

  * cp_test_own_pack: the device arrays equal the numpy specification (tests/own_pack_model.py) exactly -- sizes around a block edge,
    around n + 1 = 0 (mod 256) and around the first stored plane, empty columns, a column of several 256-entry blocks, one row;
  * the 16-bit boundary: a pattern whose largest in-block offset is exactly 65 535 in both fields runs packed, one with 65 790 falls
    back to the wide arrays, and a layer is right in both cases;
  * layer parity (check_layer of tests/test_gpu_blocks.py) under own_pack 1 and 0 for the connectivity, work, Float64 and hyperedge
    models, under the driver options that change which tiles exist or which kernel runs them, for row tiles, and with the winners
    (and so the heads of the tasks between them) on the first and the last column of 256-column blocks;
  * cp_get_stat("own_pack_tiles"): positive where the packed path must be taken; zero with the option off, with own_blk 0 (tiles
    straddle blocks), for hyperedge costs and for windowed layers.

Off-diagonal guard as in tests/test_gpu_own_split.py: the winners off the diagonal must exceed 10 000 over the three mid-size
matrices (6 525 columns in all), each case its share in proportion to its n."""
import numpy as np
import pytest

import own_pack_model as opm
from test_gpu_blocks import check_layer, Tables, w_rows
from test_gpu_own_split import dense_one, one_row, tables, MATS, MID, MID_COLUMNS, MODELS, NET, WORK
from util import cp, sprand, suitesparse_shaped

pytestmark = pytest.mark.gpu

DEFAULTS = {"own_pack": 1, "own_split": 1, "own_blk": 1, "own_pair": 1, "gap_split": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0, "own_min": 64,
            "poison": 0, "block_tables": 0}

DOWNLOAD = [("n%d" % n, (lambda n=n: suitesparse_shaped(n, 6, 100 + n))) for n in (511, 512, 513, 767, 1023, 1024, 1025)] + \
           [("n3000", lambda: suitesparse_shaped(3000, 8, 1)), ("empty_columns", lambda: sprand(50, 700, 0.01, np.random.default_rng(3))),
            ("dense_one", lambda: dense_one(1300, 1500, 4)), ("one_row", lambda: one_row(600, 8))]


def arrays_equal_spec(hip, A, name):
    nb, vpk, vbase, info = opm.pack(A)
    gnb, gpk, gbase, ginfo = hip.test_own_pack(A)
    assert gnb == nb and ginfo == info, (name, ginfo, info)
    assert np.array_equal(gpk, vpk), name
    assert np.array_equal(gbase, vbase), name
    return info


@pytest.mark.parametrize("name,make", DOWNLOAD)
def test_device_arrays_equal_the_specification(hip, name, make):
    A = make()
    if name == "empty_columns":
        assert np.any(np.diff(A.colptr) == 0)
    if name == "dense_one":
        assert np.diff(A.colptr).max() > 600
    info = arrays_equal_spec(hip, A, name)
    assert info["packed"] == 1 and info["blocks"] == -(-(A.n + 1) // 256)


def both(hip, A, T, mdl, rows_on, rows_off, opts=None, tile=None):
    """check_layer under own_pack 1, then 0: (winners off the diagonal, packed tiles with the option on, ... off, split tiles on, off, own_pack_wide)"""
    try:
        for k, v in (opts or {}).items():
            assert hip.set_option(k, v) == 0
        out = []
        for on, rows in ((1, rows_on), (0, rows_off)):
            assert hip.set_option("own_pack", on) == 0
            assert hip.set_option("stat_reset", 1) == 0
            moved = check_layer(hip, A, T, mdl, rows, tile=tile)
            out.append((moved, hip.get_stat("own_pack_tiles"), hip.get_stat("own_split_tiles"), hip.get_stat("own_pack_wide"), hip.get_stat("gap_split_tiles")))
        assert out[0][1] <= out[0][2] + out[0][4]           # (packed tiles are split tiles, those of the gap rounds included)
        return out[0][0], out[0][1], out[1][1], out[0][2], out[1][2], out[0][3]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)


@pytest.mark.parametrize("c,fits,largest", [(257, 1, 65535), (258, 0, 65790)])
def test_sixteen_bit_boundary(hip, c, fits, largest):
    A = opm.boundary(c)
    info = arrays_equal_spec(hip, A, "boundary%d" % c)
    assert info == {"blocks": 3, "packed": fits, "max_start": largest, "max_prefix": largest}
    T = Tables(A)
    rng = np.random.default_rng(70 + c)
    for mdl in (NET, WORK):
        scale = int(abs(T.F(mdl, 2)).max()) + 1
        rows = w_rows(rng, A.n, scale, np.int64)
        moved, pk_on, pk_off, sp_on, sp_off, wide = both(hip, A, T, mdl, rows, [rows[0], rows[5]])
        assert wide == 1 - fits and pk_off == 0
        assert sp_on > 0                                    # (split tiles in both cases: the fallback streams them from the wide arrays)
        assert (pk_on > 0) if fits else (pk_on == 0)


@pytest.mark.parametrize("mi", range(len(MATS)))
@pytest.mark.parametrize("ki", range(len(MODELS)))
def test_layer_parity_on_and_off(hip, mi, ki):
    T = tables(mi)
    A, mdl = T.A, MODELS[ki][1]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    rng = np.random.default_rng(1800 + 10 * mi + ki)
    scale = int(abs(T.F(mdl, 2)).max()) + 1
    rows = w_rows(rng, A.n, scale, dt)
    moved, pk_on, pk_off, sp_on, sp_off, wide = both(hip, A, T, mdl, rows, [rows[0], rows[5]])
    assert pk_off == 0 and wide == 0
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    if hyper:
        assert pk_on == 0                                   # the second entry list is not split: the tiles stream whole columns
    if mi < len(MID):
        assert moved * MID_COLUMNS > 10000 * A.n, (MATS[mi][0], MODELS[ki][0], moved)
        if not hyper:
            assert pk_on > 0 and sp_on > 0, (MATS[mi][0], MODELS[ki][0])


OPTION_SETS = [{"own_blk": 0}, {"own_pair": 0}, {"gap_tau": -1}, {"gap_tau": 8, "gap_min": 8}, {"gap_split": 0}, {"nospec": 1}, {"own_min": 1000},
               {"poison": 1}]


@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_layer_parity_under_driver_options(hip, oi):
    """(gap_tau -1: a paired launch that holds tiles of plane 7 next to split ones keeps the wide arrays; own_pair 0 with it: the
    one-tile kernel chooses per tile)"""
    for mi, models in ((0, [NET]), (2, [NET, WORK])):
        T = tables(mi)
        A = T.A
        for k, mdl in enumerate(models):
            rng = np.random.default_rng(1900 + 10 * oi + 3 * mi + k)
            scale = int(abs(T.F(mdl, 2)).max()) + 1
            rows = w_rows(rng, A.n, scale, np.int64)
            moved, pk_on, pk_off, sp_on, sp_off, wide = both(hip, A, T, mdl, [rows[0], rows[2], rows[5]], [rows[5]], opts=OPTION_SETS[oi])
            assert pk_off == 0 and wide == 0 and 2 * moved * MID_COLUMNS > 10000 * A.n       # (half the rows of a mid-size case: half its share)
            if OPTION_SETS[oi] == {"own_blk": 0}:
                assert pk_on == 0 and sp_on > 0
            if OPTION_SETS[oi] in ({"own_pair": 0}, {"nospec": 1}, {"poison": 1}):
                assert pk_on > 0, (OPTION_SETS[oi], MATS[mi][0])


def test_one_tile_kernel_chooses_per_tile(hip):
    """own_pair 0 and no gap rounds: the rounds below plane 8 hold plane-7 tiles (whole columns) and split tiles in one launch"""
    T = tables(0)
    A = T.A
    rng = np.random.default_rng(77)
    scale = int(abs(T.F(NET, 2)).max()) + 1
    rows = w_rows(rng, A.n, scale, np.int64)
    moved, pk_on, pk_off, sp_on, sp_off, wide = both(hip, A, T, NET, [rows[0], rows[5]], [rows[5]], opts={"own_pair": 0, "gap_tau": -1})
    assert pk_on > 0 and pk_on == sp_on and pk_off == 0     # (no gap rounds: every split tile is counted by own_split_tiles)


def test_row_tiles_with_injected_rows(hip):
    A = suitesparse_shaped(2000, 6, 5)
    T = Tables(A)
    n = A.n
    rng = np.random.default_rng(112)
    for mdl in (NET, WORK):
        scale = int(abs(T.F(mdl, 2)).max()) + 1
        for (lo, hi) in [(1, n // 3), (n // 3, n // 2 + 7), (n // 2 + 7, n + 2)]:
            rows = w_rows(rng, n, scale, np.int64)
            both(hip, A, T, mdl, [rows[0], rows[5]], [rows[5]], tile=(max(1, lo), hi))


@pytest.mark.parametrize("edge", [0, 255])
def test_winners_on_block_edges(hip, edge):
    """W is flat with wells on the first (0) / the last (255) column of some 256-column blocks: the winners of most rows, and with
    them the heads B of the tasks the next rounds bound by them, sit on those columns -- a head tile of one step at the start of a
    block, or one that covers its whole block"""
    T = tables(0)
    A = T.A
    n = A.n
    for mdl in (NET, WORK):
        scale = int(abs(T.F(mdl, 2)).max()) + 1
        W = np.full(n + 1, 8 * scale, dtype=np.int64)
        wells = np.arange(256, n, 512) + edge
        W[wells[wells < n]] = 0
        W2 = W.copy()
        more = np.arange(512, n, 256) + edge
        W2[more[more < n]] = scale // 2
        moved, pk_on, pk_off, sp_on, sp_off, wide = both(hip, A, T, mdl, [W, W2], [W2])
        assert pk_on > 0 and pk_off == 0 and moved > n // 2


def test_windowed_layers_take_no_packed_tiles(hip):
    A = suitesparse_shaped(6000, 8, 21)
    n, K = A.n, 4
    try:
        res = {}
        for name, f in (("win", cp.ConstrainedCost(NET, cp.VertexCount(), -(-3 * n // (2 * K)))), ("free", NET)):
            for on in (1, 0):
                assert hip.set_option("own_pack", on) == 0 and hip.set_option("stat_reset", 1) == 0
                res[name, on] = (cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip), hip.get_stat("own_pack_tiles"))
        assert res["win", 1][1] == 0 and res["win", 0][1] == 0 and res["free", 0][1] == 0
        assert res["win", 1][0] == res["win", 0][0] and res["free", 1][0] == res["free", 0][0]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
