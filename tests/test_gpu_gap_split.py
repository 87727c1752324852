"""Gap tiles of the planes >= 8 that stream only their plane's variable link entries (cp_set_option("gap_split", 1), the default;
k_lpass_own<GAP> of csrc/dp_total_own.hip) against the gap tiles that stream whole columns (gap_split 0) and against brute force
(check_layer of tests/test_gpu_blocks.py: the combined row, every per-block winner and the counts stored with it).

Which gap tasks a layer has is modelled here in numpy from brute force's per-block winners (gap_tasks: the rule of k_setup_short),
their tiles and the specials each tile holds from the split arrays of tests/own_split_model.py (tile_specials), so that no case is
vacuous: cp_get_stat("gap_split_tiles") must be positive wherever the model finds a gap task of a plane >= 8, and the engineered
patterns assert the number of specials they were built for.

Engineered patterns (scenario): one private row per column; a previous-layer row that is huge except for two wells pa < pB of one
Fenwick block; "switch" rows that sit in a column of [pa, pB) and again in a column x.  A row r' of the rectangle prefers pB until
the columns [pB, r') hold x for enough of the switch rows, then pa: with every x inside [rL, rR - 1] of a gap row r (rL = r - 2^tau,
rR = r + 2^tau) the task of r has the candidates [pa, pB], and a switch entry is special exactly when rL < x < rR - 1.

  * sizes just above 512 (513, 767 - 769: the planes 8 and 9 exist) and n = 3000, random patterns and previous rows, under the
    driver options that change which tiles exist (plane-7 and split tiles in one launch; every round a gap round; unsorted tiles;
    poison; exact counts; every tile flagged: the SLOW walks);
  * run lengths of the VARIABLE stream: a column of d variable entries, d around 256, 512, 768, 1024, at every alignment of the
    run's start, near column 3 and at column 300; truly empty columns inside the tile;
  * 1, 31 and 32 specials in one tile (32: the tile is handed to the SLOW walk), in the tile's first and last column, two in one
    column, in a tile of plane 8 and in the two tiles of a plane-9 task;
  * the stat is zero with gap_split 0, with own_split 0, for hyperedge costs and for a constrained partition, and own_split_tiles
    does not count gap tiles;
  * one whole partition.

Off-diagonal guard: the winners off the diagonal, counted by brute force alone, number at least n / 2 per shape and setting."""
import numpy as np
import pytest

import brute
import own_split_model as osm
from test_gpu_blocks import check_layer, Tables, w_rows
from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

CONN0 = cp.AffineConnectivityModel(0, 0, 0, 1)
NET = cp.AffineConnectivityModel(1, 10, 1, 100)
WORK = cp.AffineWorkModel(0, 10, 1)
HYP = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
DEFAULTS = {"gap_split": 1, "own_split": 1, "own_blk": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0, "poison": 0, "dbg": 0, "block_tables": 0}
LEAF_T, LT, SHORT_T = 6, 256, 8
BIG = 10 ** 12


# ---------------------------------------------------------------- the numpy model
def gap_tasks(ob, n, gap_tau=6, gap_min=64):
    """the gap tasks of an unconstrained layer whose per-block winners are ob[b, r] (brute.block_argmins): rows r with
    ctz(r) = tau <= gap_tau (the rounds below LEAF_T are the leaf pass), every plane b > tau with bit b of r set, candidates
    [a, B] from the two tree neighbours, at least gap_min of them; a gap task finishes the rows (rL, hi) of its plane"""
    nb = ob.shape[0]
    fin, out = set(), []
    for tau in range(min(gap_tau, nb - 1), LEAF_T - 1, -1):
        for r in range(1 << tau, n + 1, 2 << tau):
            for b in range(tau + 1, nb):
                if not (r >> b) & 1 or (b, r) in fin:
                    continue
                rb = (r >> b) << b
                rL, rR = r - (1 << tau), r + (1 << tau)
                B = int(ob[b, rL])
                a = int(ob[b, min(rR, n)]) if rR - rb < (1 << b) else rb - (1 << b)
                a = min(a, B)
                if 1 + B - a >= gap_min and 1 + B - a > SHORT_T:
                    hi = min(rR, rb + (1 << b), n + 1)
                    out.append(dict(tau=tau, r=r, b=b, a=a, B=B, rL=rL, hi=hi))
                    fin.update((b, x) for x in range(rL + 1, hi))
    return out


def tile_specials(S, t):
    """{256-column block: variable entries of the task's plane, in the columns the block's candidates step over, with
    rL < next < hi - 1} for a gap task of a plane >= 8 (own_blk 1: one tile per block)"""
    nb, vpos, vsa, vnext = S
    i = t["b"] - osm.BMIN
    out = {}
    for c in range(t["a"] // LT, t["B"] // LT + 1):
        lo, hi = max(t["a"], LT * c), min(t["B"] - 1, LT * c + LT - 1)       # (the head candidate B steps over no column)
        v = vnext[int(vpos[i, lo]):int(vpos[i, hi + 1])] if hi >= lo else vnext[:0]
        out[c] = int(np.sum((v > t["rL"]) & (v < t["hi"] - 1)))
    return out


def split_gap_tasks(T, mdl, rows, opts):
    F = T.F(mdl, 2)
    n = T.A.n
    o = dict(DEFAULTS, **(opts or {}))
    return [[t for t in gap_tasks(brute.block_argmins(W, F, int(n).bit_length()), n, o["gap_tau"], o["gap_min"]) if t["b"] >= osm.BMIN] for W in rows]


# ---------------------------------------------------------------- patterns
def build(n, pairs, empty=()):
    """one private row per column (none for the columns of `empty`) and the (row id >= n, column) pairs"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    m = n + (int(pairs[:, 0].max()) - n + 1 if pairs.size else 0)
    diag = np.setdiff1d(np.arange(n, dtype=np.int64), np.asarray(empty, dtype=np.int64))
    key = np.unique(np.concatenate([diag * m + diag, pairs[:, 1] * m + pairs[:, 0]]))
    cols, rws = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rws + 1)


def scenario(n, switches, dense=None, empty=()):
    """switches: (column, x) per switch row; dense: (column, d, x): d more rows in `column` and again in column x"""
    pairs, rid = [], n
    for c, x in switches:
        pairs += [(rid, c), (rid, x)]
        rid += 1
    if dense:
        c, d, x = dense
        for _ in range(d):
            pairs += [(rid, c), (rid, x)]
            rid += 1
    return build(n, pairs, empty)


def wells(T, mdl, n, pa, pB, rL, rR):
    """a previous row whose only affordable candidates are pa and pB, priced so that the rows <= rL take pB and the rows >= rR pa"""
    F = T.F(mdl, 2)
    W = np.full(n + 1, BIG, dtype=np.int64)
    W[pa] = 0
    W[pB] = int(F[pa, rR] - F[pB, rR]) + 1
    assert int(F[pa, rL] - F[pB, rL]) >= W[pB] > 0, "the switch rows do not move the winner"
    return W


_tables = {}


def tables(key, make):
    if key not in _tables:
        _tables[key] = Tables(make())
    return _tables[key]


def both(hip, T, mdl, rows, opts=None, expect_tasks=None):
    """check_layer under gap_split 1, then 0, with the guards of this file -> the modelled gap tasks of the planes >= 8 per row"""
    A = T.A
    tasks = split_gap_tasks(T, mdl, rows, opts)
    have = any(len(t) > 0 for t in tasks)
    if expect_tasks is not None:
        assert have == expect_tasks, (A, tasks)
    hyper = mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT
    o = dict(DEFAULTS, **(opts or {}))
    all_gap = o["gap_tau"] >= int(A.n).bit_length() - 2
    try:
        for k, v in (opts or {}).items():
            assert hip.set_option(k, v) == 0
        for on in (1, 0):
            assert hip.set_option("gap_split", on) == 0 and hip.set_option("stat_reset", 1) == 0
            moved = check_layer(hip, A, T, mdl, rows)
            gt, ot = hip.get_stat("gap_split_tiles"), hip.get_stat("own_split_tiles")
            print(A, "gap_split", on, "off-diagonal winners", moved, "gap_split_tiles", gt, "own_split_tiles", ot, "modelled tasks", [len(t) for t in tasks])
            assert 2 * moved >= A.n, (A, on, moved)
            if not on or hyper or not o["own_split"]:
                assert gt == 0, (A, on, gt)
            elif have:
                assert gt > 0, (A, tasks)
            if all_gap:
                assert ot == 0, (A, ot)
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
    return tasks


# ---------------------------------------------------------------- random patterns: sizes and driver options
SIZES = [("n513", lambda: suitesparse_shaped(513, 6, 11)), ("n767", lambda: suitesparse_shaped(767, 6, 12)),
         ("n768", lambda: suitesparse_shaped(768, 6, 13)), ("n769", lambda: suitesparse_shaped(769, 6, 14)),
         ("n3000", lambda: suitesparse_shaped(3000, 8, 1))]
OPTION_SETS = [{}, {"gap_tau": 8, "gap_min": 8}, {"own_blk": 0}, {"poison": 1}, {"nospec": 1}, {"dbg": 512}]


def rows_with_tasks(T, mdl, seed, opts, kinds=(0, 1, 5)):
    """w_rows of the first seed from `seed` on that gives the layer a gap task of a plane >= 8, by brute force alone"""
    F = T.F(mdl, 2)
    for s in range(seed, seed + 32):
        allrows = w_rows(np.random.default_rng(s), T.A.n, int(abs(F).max()) + 1, np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64)
        rows = [allrows[k] for k in kinds]
        if any(split_gap_tasks(T, mdl, rows, opts)):
            return rows
    raise AssertionError("no seed gives the layer a gap task of a plane >= 8")


@pytest.mark.parametrize("si", range(len(SIZES)), ids=[s[0] for s in SIZES])
def test_sizes_around_the_first_split_planes(hip, si):
    T = tables(SIZES[si][0], SIZES[si][1])
    for k, mdl in enumerate((NET, WORK)):
        both(hip, T, mdl, rows_with_tasks(T, mdl, 2000 + 10 * si + k, {}), expect_tasks=True)


@pytest.mark.parametrize("oi", range(1, len(OPTION_SETS)), ids=[str(o) for o in OPTION_SETS[1:]])
def test_driver_options(hip, oi):
    """(defaults: plane-7 tiles, which stream whole columns, and split gap tiles in one launch -- the sizes above; gap_tau 8 with
    gap_min 8: every round of these sizes is a gap round, own_split_tiles stays zero; dbg 512: every tile goes to the SLOW walks of
    k_gap_finish / k_gap_seg, which read the original arrays)"""
    for si in (0, 3, 4):
        T = tables(SIZES[si][0], SIZES[si][1])
        rows = rows_with_tasks(T, NET, 2100 + 10 * si + oi, OPTION_SETS[oi], kinds=(1, 5))
        tasks = both(hip, T, NET, rows, OPTION_SETS[oi], expect_tasks=True)
        if OPTION_SETS[oi].get("gap_tau") == 8:
            assert any(t["tau"] > 6 for ts in tasks for t in ts) or T.A.n < 600


# ---------------------------------------------------------------- engineered patterns
# (n, plane, gap row r of round 6, wells): plane 8: block [0, 256), rows (256, 512); plane 9: block [0, 512), rows (512, 1024)
GEO = {8: dict(n=600, r=320, pa=2, pB=250), 9: dict(n=769, r=576, pa=100, pB=400)}


def engineered(hip, key, b, switches, dense=None, empty=(), models=(CONN0, NET), want=None, opts=None):
    g = GEO[b]
    n, r, pa, pB = g["n"], g["r"], g["pa"], g["pB"]
    rL, rR = r - 64, r + 64
    T = tables(key, lambda: scenario(n, switches, dense, empty))
    S = osm.split(T.A)
    for mdl in models:
        W = wells(T, mdl, n, pa, pB, rL, rR)
        tasks = both(hip, T, mdl, [W], opts, expect_tasks=True)[0]
        mine = [t for t in tasks if t["r"] == r and t["b"] == b]
        assert len(mine) == 1 and (mine[0]["a"], mine[0]["B"]) == (pa, pB), tasks
        sp = tile_specials(S, mine[0])
        if want is not None:
            assert sorted(sp.values()) == sorted(want), (key, sp)
    return T


def spread(cols, xs):
    return [(int(cols[i % len(cols)]), int(xs[i % len(xs)])) for i in range(max(len(cols), len(xs)))]


@pytest.mark.parametrize("k", [1, 31, 32])
@pytest.mark.parametrize("b", [8, 9])
def test_specials_in_one_tile(hip, b, k):
    """k specials in one tile of the task (plane 9: the task's other tile holds none); 32: spec 255, the SLOW walk"""
    g = GEO[b]
    rL, rR = g["r"] - 64, g["r"] + 64
    lo = max(g["pa"], g["pB"] // LT * LT)                   # the columns of the tile that holds pB
    cols = np.linspace(lo + 1, g["pB"] - 2, k).astype(int)
    xs = np.linspace(rL + 1, rR - 2, k).astype(int)         # every x inside (rL, rR - 1): all special
    want = [k] if b == 8 else [0, k]
    engineered(hip, ("spec", b, k), b, list(zip(cols.tolist(), xs.tolist())), want=want)


PLACES = ["first_column", "last_column", "two_in_one_column", "both_tiles_and_plain_switches"]


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("b", [8, 9])
def test_special_placement(hip, b, place):
    g = GEO[b]
    r, pa, pB = g["r"], g["pa"], g["pB"]
    rL, rR = r - 64, r + 64
    if place == "first_column":                             # the first column the tile steps over: pB - 1 (step 1)
        sw, want = [(pB - 1, rL + 5)], [1]
    elif place == "last_column":                            # the task's last candidate: the last step of its last tile
        sw, want = [(pa, rR - 2)], [1]
    elif place == "two_in_one_column":
        sw, want = [(pa + 9, rL + 1), (pa + 9, rL + 30), (pB - 7, rL + 30)], [3]
    else:                                                   # specials in every tile, and switch rows that are no specials (x = rL, x = rR - 1)
        sw = [(pa + 3, rL + 7), (pa + 3, rL), (pB - 3, rR - 1), (pB - 30, rR - 3), (pa + 40, rL + 60)]
        want = [3]
    if b == 9:
        per_tile = {0: 0, 1: 0}
        for c, x in sw:
            per_tile[c // LT] += rL < x < rR - 1
        want = list(per_tile.values())
    engineered(hip, ("place", b, place), b, sw, want=want)


def test_empty_columns_inside_a_tile(hip):
    """truly empty columns (equal starts in the column pointers too: the whole-column stream of gap_split 0 and of plane 7) around the
    specials' columns: a special's column is the LARGEST column that starts at or below its position"""
    for b in (8, 9):
        g = GEO[b]
        r, pa, pB = g["r"], g["pa"], g["pB"]
        rL, rR = r - 64, r + 64
        hole = list(range(pa + 20, pa + 60)) + [pB - 2, pB - 3]
        sw = [(pa + 19, rL + 3), (pa + 60, rL + 9), (pB - 4, rR - 2), (pB - 1, rL + 1)]
        T = engineered(hip, ("holes", b), b, sw, empty=hole, want=[4] if b == 8 else [2, 2])
        assert np.all(np.diff(T.A.colptr)[hole] == 0)


D_RANGES = [range(250, 261), range(506, 519), range(762, 773), range(1020, 1031)]


@pytest.mark.parametrize("where", ["near_column_3", "column_300"])
@pytest.mark.parametrize("ri", range(len(D_RANGES)))
def test_run_lengths_of_the_variable_stream(hip, ri, where):
    """a column of d entries that are variable in the task's plane and no specials (their next column is rL), behind 0 .. 3 variable
    entries of the columns in front: the run starts at every alignment and spans one block, a trip, two trips"""
    b = 8 if where == "near_column_3" else 9
    g = GEO[b]
    r, pa, pB = g["r"], g["pa"], g["pB"]
    rL, rR = r - 64, r + 64
    col = pa + 1 if b == 8 else 300
    for d in D_RANGES[ri]:
        lead = [(pa, rL)] * (d % 4)                          # variable entries in front of the run: its start moves through a quad
        sw = lead + [(pB - 5, rL + 2)]
        T = engineered(hip, ("run", b, d), b, sw, dense=(col, d, rL), models=(NET,), want=[1] if b == 8 else [0, 1])
        nb, vpos, vsa, vnext = osm.split(T.A)
        i = b - osm.BMIN
        assert int(vpos[i, col + 1] - vpos[i, col]) >= d and int(vpos[i, col] - vpos[i, 0]) % 4 == d % 4


# ---------------------------------------------------------------- where the path must not be taken
def test_stat_is_zero_without_the_options_and_for_hyperedge_costs(hip):
    T = tables(SIZES[3][0], SIZES[3][1])
    rows = rows_with_tasks(T, NET, 2300, {}, kinds=(1, 5))
    both(hip, T, NET, rows, {"own_split": 0}, expect_tasks=True)
    hrows = w_rows(np.random.default_rng(2301), T.A.n, int(abs(T.F(HYP, 2)).max()) + 1, np.int64)
    both(hip, T, HYP, [hrows[1], hrows[5]])


def test_one_partition_and_a_constrained_one(hip):
    """K = 4 at n = 6000: identical under gap_split 1 and 0; the windowed layers of a constrained partition take no split tile"""
    A = suitesparse_shaped(6000, 8, 21)
    n, K = A.n, 4
    try:
        res = {}
        for name, f in (("win", cp.ConstrainedCost(NET, cp.VertexCount(), -(-3 * n // (2 * K)))), ("free", NET)):
            for on in (1, 0):
                assert hip.set_option("gap_split", on) == 0 and hip.set_option("stat_reset", 1) == 0
                res[name, on] = (cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip), hip.get_stat("gap_split_tiles"))
        assert res["win", 1][1] == 0 and res["win", 0][1] == 0 and res["free", 0][1] == 0 and res["free", 1][1] > 0
        assert res["win", 1][0] == res["win", 0][0] and res["free", 1][0] == res["free", 0][0]
    finally:
        for k, v in DEFAULTS.items():
            hip.set_option(k, v)
