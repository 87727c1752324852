"""The loads of an own tile (k_lpass_own, csrc/dp_total_own.hip / interior_stream, csrc/dp_total_stream.hpp) are unconditional,
at indices clamped into the tile:
the column pointers of steps beyond the tile's length, the entry quads at and above the end of the run, the end-of-wave reloads of
the pin positions and of W, and the tile's record read from its sorted slot.  The shapes here are the smallest at which such a load
can go wrong; every case is compared with brute force (check_layer of tests/test_gpu_blocks.py: the combined row, every per-block
winner and its counts) under own_split 1 and 0.  n is just above 512, so that the planes 8 and 9 exist and take the split path.

  * run lengths around the loop's boundaries: one row per column and one dense column of degree d, d over 250..260, 506..518,
    762..772, 1020..1030 (inner / last block / one trip / two trips, at every alignment of the run's start), the dense column at
    column 3 (p_first - e negative without the clamp) and at column 300;
  * the end of the arrays: n = 513, 767, 768, 769, the last column dense, nnz of every residue mod 4;
  * empty runs; one-step and full tiles; the gap round, the unsorted tile list, poison and exact counts; one whole partition.

No case passes vacuously: with own_split 1 the split path is taken (cp_get_stat("own_split_tiles") > 0; hyperedge costs never split
and neither does a gap round: under gap_tau 8 at n < 1024 every round is one, and there the stat is zero by design), and the
winners off the diagonal, counted by brute force alone, are at least n / 2 per shape and setting."""
import numpy as np
import pytest

import brute
import own_split_model as osm
from test_gpu_blocks import check_layer, Tables, w_rows
from util import cp, sprand, suitesparse_shaped

pytestmark = pytest.mark.gpu

NET = cp.AffineConnectivityModel(1, 10, 1, 100)
WORK = cp.AffineWorkModel(0, 10, 1)                     # (pin counts: the reloaded column pointers)
CONNF = cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0)
HYP = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
DEFAULTS = {"own_split": 1, "own_blk": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0, "own_min": 64, "poison": 0, "block_tables": 0}
# w_rows kinds whose winners leave the diagonal: random, increasing (nearly every row, for every seed), flat with deep wells (wide
# gaps: long tasks; how many rows it moves depends on where the seed puts the wells)
KINDS_ON, KINDS_OFF = (0, 1, 5), (1, 5)

D_RANGES = [range(250, 261), range(506, 519), range(762, 773), range(1020, 1031)]
DENSE_AT = [3, 300]


def dense_at(n, col, d, drop=0):
    """column j holds row d + j; column `col` holds the rows 0 .. d - 1 as well; the last `drop` entries (of the last column) dropped"""
    m = n + d
    key = np.unique(np.concatenate([np.arange(n, dtype=np.int64) * m + d + np.arange(n), col * m + np.arange(d, dtype=np.int64)]))
    key = key[:key.size - drop]
    cols, rows = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows + 1)


def empty_block(n=700, m=400, seed=5):
    """three rows per column, the columns 256 .. 511 empty"""
    rng = np.random.default_rng(seed)
    cols = np.repeat(np.concatenate([np.arange(256), np.arange(512, n)]), 3)
    key = np.unique(cols.astype(np.int64) * m + rng.integers(0, m, cols.size))
    cols, rows = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows + 1)


_tables = {}


def tables(key, make):
    """brute-force tables of a shape: computed once, shared by the cases"""
    if key not in _tables:
        _tables[key] = Tables(make())
    return _tables[key]


def long_task_rows(T, mdl, seed, dt, kinds):
    """w_rows of the first seed from `seed` on that gives the split path a task, by brute force alone.  At n < 640 the only row
    outside round A and the gap rounds (tau <= 6) that has a plane >= 8 is r = 384 (tau 7, plane 8, block [0, 256)); its candidates
    end at the plane-8 winner of row 256, so one of the rows used must put that winner at column 128 or beyond: a task of more
    than twice own_min steps, whatever the other bound.  (Every n of this file has that row.)"""
    F = T.F(mdl, 2)
    nb = int(T.A.n).bit_length()
    for s in range(seed, seed + 64):
        rows = w_rows(np.random.default_rng(s), T.A.n, int(abs(F).max()) + 1, dt)
        if any(brute.block_argmins(rows[k], F, nb)[8, 256] >= 128 for k in kinds):
            return rows
    raise AssertionError("no seed gives row 384 a long plane-8 task")


def on_and_off(hip, T, mdl, seed, opts=None, kinds_on=KINDS_ON, kinds_off=KINDS_OFF):
    """check_layer under own_split 1, then 0, with the guards of this file.  Split tiles exist outside round A and the gap rounds
    only: with gap_tau >= nbits - 2 every other round is a gap round (a row with ctz = nbits - 1 has one set bit: round A), and the
    stat must then be zero"""
    A = T.A
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    all_gap = (opts or {}).get("gap_tau", DEFAULTS["gap_tau"]) >= int(A.n).bit_length() - 2
    rows = long_task_rows(T, mdl, seed, dt, kinds_on)
    try:
        for k, v in (opts or {}).items():
            assert hip.set_option(k, v) == 0
        for on, kinds in ((1, kinds_on), (0, kinds_off)):
            assert hip.set_option("own_split", on) == 0
            assert hip.set_option("stat_reset", 1) == 0
            moved = check_layer(hip, A, T, mdl, [rows[k] for k in kinds])
            assert 2 * moved >= A.n, (A, on, moved)
            tiles = hip.get_stat("own_split_tiles")
            assert (tiles > 0) if (on and not hyper and not all_gap) else (tiles == 0), (A, on, tiles)
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)


def run_family(hip, ri, col, mdl, seed, opts=None, **kw):
    for d in D_RANGES[ri]:
        on_and_off(hip, tables(("dense", col, d), lambda: dense_at(600, col, d)), mdl, seed + d, opts, **kw)


@pytest.mark.parametrize("col", DENSE_AT)
@pytest.mark.parametrize("ri", range(len(D_RANGES)))
def test_run_lengths_around_the_loop_boundaries(hip, ri, col):
    for mdl in (NET, WORK):
        run_family(hip, ri, col, mdl, 1000 * ri + col)


OPTION_SETS = [{"gap_tau": 8, "gap_min": 8}, {"own_blk": 0}, {"poison": 1}, {"nospec": 1}]


@pytest.mark.parametrize("col", DENSE_AT)
@pytest.mark.parametrize("ri", range(len(D_RANGES)))
@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_run_lengths_under_driver_options(hip, oi, ri, col):
    """the gap round streams the same runs with the DET flags; own_blk 0 reads the records unsorted; with poison 1 a stale or
    wrongly clamped record shows as a poisoned winner"""
    run_family(hip, ri, col, NET, 5000 + 1000 * ri + col + 7 * oi, OPTION_SETS[oi], kinds_on=(1, 5))


END_N = [513, 767, 768, 769]


def end_shape(n, drop):
    return dense_at(n, n - 1, 300, drop)


@pytest.mark.parametrize("n", END_N)
def test_end_of_the_arrays(hip, n):
    residues = set()
    for drop in range(4):
        T = tables(("end", n, drop), lambda: end_shape(n, drop))
        A = T.A
        nnz = int(A.colptr[-1] - 1)
        assert nnz == n + 300 - drop
        residues.add(nnz % 4)
        # the last column's entries end the link array, and the last stored plane's entries of the column block in front of its
        # sibling block, [256, 512), are the last entries of vnext: a tile's run ends where the array does
        assert int(A.colptr[n] - A.colptr[n - 1]) >= 298
        nb, vpos, vsa, vnext = osm.split(A)
        assert nb == 2 and int(vpos[nb - 1, 512]) == vnext.size and int(vpos[nb - 1, 512]) > int(vpos[nb - 1, 256])
        for mdl in (NET, WORK):
            on_and_off(hip, T, mdl, 2000 + 4 * n + drop)
    assert residues == {0, 1, 2, 3}


@pytest.mark.parametrize("name,mdl", [("f64", CONNF), ("hyp", HYP)])
def test_float64_and_hyperedge_models(hip, name, mdl):
    """(the hyperedge tiles stream two entry lists and never split; the Float64 tiles do)"""
    for ri in range(len(D_RANGES)):
        for col in DENSE_AT:
            for d in (D_RANGES[ri][0], D_RANGES[ri][5], D_RANGES[ri][-1]):
                on_and_off(hip, tables(("dense", col, d), lambda: dense_at(600, col, d)), mdl, 3000 + d + col, kinds_on=(1, 5))
    for n in END_N:
        for drop in (0, 3):
            on_and_off(hip, tables(("end", n, drop), lambda: end_shape(n, drop)), mdl, 3500 + n + drop, kinds_on=(1, 5))


def test_empty_runs(hip):
    """zero-trip tiles: Q_lo == Q_hi"""
    A = sprand(50, 700, 0.01, np.random.default_rng(3))
    assert np.any(np.diff(A.colptr) == 0)
    B = empty_block()
    assert np.all(np.diff(B.colptr)[256:512] == 0) and np.all(np.diff(B.colptr)[:256] > 0)
    for key, M in (("sprand", A), ("empty_block", B)):
        T = tables(key, lambda: M)
        for mdl in (NET, WORK):
            on_and_off(hip, T, mdl, 4000)


def test_one_step_and_full_tiles(hip):
    """own_min 1: every task has tiles of its own, with head and tail tiles of tl = 0 .. 255"""
    T = tables("shaped1025", lambda: suitesparse_shaped(1025, 5, 7))
    for mdl in (NET, WORK):
        on_and_off(hip, T, mdl, 4100, {"own_min": 1, "own_blk": 1})


def test_one_partition(hip):
    A = suitesparse_shaped(6000, 8, 21)
    try:
        res = []
        for on in (1, 0):
            assert hip.set_option("own_split", on) == 0 and hip.set_option("stat_reset", 1) == 0
            res.append(cp.partition_stripe(A, 4, cp.DynamicTotalSplitter(NET), backend=hip))
            assert (hip.get_stat("own_split_tiles") > 0) == (on == 1)
        assert res[0] == res[1]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
