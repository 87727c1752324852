"""Two own tiles per wave (cp_set_option("own_pair", 1), the default; k_lpass_own<PAIR> of csrc/dp_total_own.hip) against one tile per
wave (own_pair 0) and against brute force.  Wave w takes the slots 2 w and 2 w + 1 of a round's run order (tests/own_pair_model.py;
the pairing itself is checked without a device in tests/test_own_pair_model.py); the two tiles may belong to different tasks, planes
and blocks, one may be split (own_split) and the other not, and the wave that ends an odd order runs one tile and stores once.

Every case is check_layer of tests/test_gpu_blocks.py -- the combined row, every per-block winner and its counts against brute
force -- under own_pair 1, then 0: both settings equal brute force, hence each other.  The shapes are those of
tests/test_gpu_own_tile_loads.py (its brute-force tables are shared when both files run in one session):

  * n just above 512 (513, 600, 767, 768, 769): planes 8 and 9 exist and a round holds a few own tiles -- round A alone 3, 4, 5, 3, 5
    of them (own_pair_model.round_a_tiles): a pair and a lone wave, two pairs, two pairs and a lone wave;
  * n = 1200 with the wide-gap rows: tasks of three and more tiles; under own_blk 0 a pair is the head and an interior tile of one
    task, under own_blk 1 tiles of different tasks, planes and blocks;
  * gap_tau 5: round tau = 6 is then an ordinary round whose launch holds plane-7 tiles (never split) next to the split tiles of
    the planes 8 and 9, under own_split 1 and 0;
  * the dense-column and empty-block shapes at run lengths around 256 / 512 / 768 / 1024: the partner's clamped loads meet empty and
    full runs and the end of the arrays;
  * connectivity, work (pin positions), integral Float64, pin-free Int64 and hyperedge costs (which do not pair); poison, own_blk 0,
    and gap_tau 8.

No case passes vacuously.  With own_pair 1 every case that is not a hyperedge case has own_pair_waves > 0, with own_pair 0 and for
hyperedge costs both counters are zero, and the sizes with an odd round A assert own_pair_lone > 0.  Under gap_tau 8 every round
but round A is a gap round at n < 1024 -- round A never is one, and its own tiles go through the paired kernel -- so there the
counters must be exactly round A's: layers * (round_a_tiles // 2) and layers * (round_a_tiles % 2).  The winners off the diagonal,
counted by brute force alone, are at least n / 2 per shape and setting."""
import numpy as np
import pytest

import brute
import own_pair_model as opm
from test_gpu_blocks import check_layer
from test_gpu_own_tile_loads import D_RANGES, DENSE_AT, dense_at, empty_block, end_shape, long_task_rows, tables
from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

NET = cp.AffineConnectivityModel(1, 10, 1, 100)
WORK = cp.AffineWorkModel(0, 10, 1)                     # (pin counts: the reloaded column pointers)
CONNF = cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0)
CONN1 = cp.AffineConnectivityModel(0, 0, 0, 1)          # (pin coefficient zero, as CONNF: the paired waves narrow the pin-position loads)
HYP = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
DEFAULTS = {"own_pair": 1, "own_split": 1, "gap_split": 1, "own_blk": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0, "own_min": 64, "poison": 0,
            "block_tables": 0}
KINDS = (1, 5)          # w_rows: increasing (nearly every winner leaves the diagonal), flat with deep wells (wide gaps: long tasks)


def plane7_rows(T, mdl, seed, dt):
    """long_task_rows, and a long plane-7 task in round tau = 6 as well: row 192 (bits 7 and 6) takes the candidates [0, winner of
    row 128 in plane 7], so a winner at column 64 or beyond makes it a task of more than own_min steps -- by brute force alone"""
    F = T.F(mdl, 2)
    nb = int(T.A.n).bit_length()
    for s in range(seed, seed + 64):
        rows = long_task_rows(T, mdl, s, dt, KINDS)
        if any(brute.block_argmins(rows[k], F, nb)[7, 128] >= 64 for k in KINDS):
            return rows
    raise AssertionError("no seed gives row 192 a long plane-7 task")


def pair_and_single(hip, T, mdl, seed, opts=None, lone=False, rows_of=None):
    """check_layer under own_pair 1, then 0, with the guards of this file; returns the counters of the paired run"""
    A = T.A
    opts = opts or {}
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    all_gap = opts.get("gap_tau", DEFAULTS["gap_tau"]) >= int(A.n).bit_length() - 2
    rows = rows_of(T, mdl, seed, dt) if rows_of else long_task_rows(T, mdl, seed, dt, KINDS)
    nta = opm.round_a_tiles(A.n, opts.get("own_min", DEFAULTS["own_min"]), opts.get("own_blk", DEFAULTS["own_blk"]))
    out = None
    try:
        for k, v in opts.items():
            assert hip.set_option(k, v) == 0
        for on in (1, 0):
            assert hip.set_option("own_pair", on) == 0
            assert hip.set_option("stat_reset", 1) == 0
            moved = check_layer(hip, A, T, mdl, [rows[k] for k in KINDS])
            waves, lones = hip.get_stat("own_pair_waves"), hip.get_stat("own_pair_lone")
            print(A, mdl.kind, opts, "own_pair", on, "off-diagonal winners", moved, "own_pair_waves", waves, "own_pair_lone", lones, "round A tiles", nta)
            assert 2 * moved >= A.n, (A, on, moved)
            if not on or hyper:
                assert waves == 0 and lones == 0, (A, on, waves, lones)
            elif all_gap:
                assert (waves, lones) == (len(KINDS) * (nta // 2), len(KINDS) * (nta % 2)), (A, waves, lones, nta)
            else:
                assert waves > 0, (A, opts, waves, lones)
                if lone:
                    assert lones > 0, (A, opts, waves, lones)
                out = (waves, lones, hip.get_stat("own_split_tiles"))
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
    return out


def size_shape(n):
    return tables(("dense", 300, 256), lambda: dense_at(600, 300, 256)) if n == 600 else tables(("end", n, 0), lambda: end_shape(n, 0))


@pytest.mark.parametrize("n", [513, 600, 767, 768, 769])
def test_sizes_just_above_512(hip, n):
    """a lone wave, exact pairs, pairs and a lone wave; an odd round A (513, 767, 768, 769) leaves a lone wave whatever the other rounds hold"""
    T = size_shape(n)
    assert T.A.n == n and opm.round_a_tiles(n) >= 2
    for mdl in (NET, WORK):
        pair_and_single(hip, T, mdl, 100 + n, lone=opm.round_a_tiles(n) % 2 == 1)


@pytest.mark.parametrize("blk", [1, 0])
def test_tasks_of_three_and_more_tiles(hip, blk):
    T = tables("shaped1200", lambda: suitesparse_shaped(1200, 5, 7))
    assert opm.own_ntiles(blk, 1024, 1025) >= 4            # (round A's plane-10 task; the wide gaps give the tau rounds theirs)
    for mdl in (NET, WORK):
        pair_and_single(hip, T, mdl, 200 + blk, {"own_blk": blk})


@pytest.mark.parametrize("split", [1, 0])
def test_split_and_unsplit_tiles_in_one_launch(hip, split):
    """gap_tau 5: the launch of round tau = 6 holds plane-7 tiles, which stream whole columns, and tiles of the planes 8 and 9, and
    its waves run them in pairs.  (Which two tiles share a wave is not fixed: a tile's rank inside its column block, and a task's
    place in the list, come from atomics.  So the case shows both kinds in one paired launch, not a given mixed pair.)"""
    T = size_shape(600)
    for mdl in (NET, WORK):
        waves, lones, split_tiles = pair_and_single(hip, T, mdl, 300, {"gap_tau": 5, "own_split": split}, rows_of=plane7_rows)
        assert (split_tiles > 0) == (split == 1)
        assert split_tiles < 2 * waves + lones           # (the paired waves also ran tiles that are not split: round A's, plane 7's)


BOUNDARY_D = [(255, 256, 257), (511, 512, 513), (767, 768, 769), (1023, 1024, 1025)]


@pytest.mark.parametrize("col", DENSE_AT)
@pytest.mark.parametrize("ri", range(len(BOUNDARY_D)))
def test_run_lengths_around_the_loop_boundaries(hip, ri, col):
    for d in BOUNDARY_D[ri]:
        assert d in D_RANGES[ri]
        T = tables(("dense", col, d), lambda: dense_at(600, col, d))
        for mdl in (NET, WORK):
            pair_and_single(hip, T, mdl, 1000 * ri + col + d)


def test_empty_runs(hip):
    """the partner of a tile may be a zero-trip tile: Q_lo == Q_hi"""
    B = empty_block()
    assert np.all(np.diff(B.colptr)[256:512] == 0) and np.all(np.diff(B.colptr)[:256] > 0)
    T = tables("empty_block", lambda: B)
    for mdl in (NET, WORK):
        pair_and_single(hip, T, mdl, 4000)


@pytest.mark.parametrize("name,mdl", [("f64", CONNF), ("hyp", HYP), ("pin0", CONN1)])
def test_float64_hyperedge_and_pin_free_models(hip, name, mdl):
    """(the hyperedge tiles stream two entry lists and keep one tile per wave; the Float64 tiles pair; a model without a pin term
    reads one pin position per tile, NET and WORK everywhere else in this file read them all)"""
    for n in (513, 600, 769):
        pair_and_single(hip, size_shape(n), mdl, 3000 + n, lone=opm.round_a_tiles(n) % 2 == 1)
    pair_and_single(hip, tables(("dense", 3, 1024), lambda: dense_at(600, 3, 1024)), mdl, 3100)


OPTION_SETS = [{"poison": 1}, {"own_blk": 0}, {"gap_tau": 8, "gap_min": 8}]


@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_driver_options(hip, oi):
    """with poison 1 a stale or wrongly clamped record shows as a poisoned winner; own_blk 0 reads the records unsorted; under
    gap_tau 8 only round A's tiles are paired"""
    for n in (513, 600, 767):
        pair_and_single(hip, size_shape(n), NET, 5000 + n + 7 * oi, OPTION_SETS[oi])
    pair_and_single(hip, tables(("dense", 300, 768), lambda: dense_at(600, 300, 768)), WORK, 5100 + oi, OPTION_SETS[oi])


def test_one_partition(hip):
    A = suitesparse_shaped(6000, 8, 21)
    try:
        res = []
        for on in (1, 0):
            assert hip.set_option("own_pair", on) == 0 and hip.set_option("stat_reset", 1) == 0
            res.append(cp.partition_stripe(A, 4, cp.DynamicTotalSplitter(NET), backend=hip))
            assert (hip.get_stat("own_pair_waves") > 0) == (on == 1)
            assert on == 1 or hip.get_stat("own_pair_lone") == 0
        assert res[0] == res[1]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
