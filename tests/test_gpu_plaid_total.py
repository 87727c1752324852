"""GPU tests of the total objective of the plaid connectivity pair (kinds 8 / 9) on the exact paths of csrc/plaid_total.hip: the
primary model on the rectangle engine, the secondary model on the prefix-min scan.

What referees what, by size:

  n <= 1000              tables bit for bit against the literal DP over cost tables built from the definition
                         (tests/plaid_total_model.py) with the engine's limits shrunk; more than one 256-column chunk per level row;
  n = 10 500 / 17 000    the defaults as shipped against the device sweep with the launch cap (the sweep counts by link scans of its
                         own, so it would notice a miscount of the engine's wavelet counters, not an error both share); the scan at
                         the tile edges and past one strip of its second level against its numpy restatement;
  n = 20 011             the public oracle entry (a link scan again; 15 wavelet levels and more than ten 2048-key blocks on the
                         pattern) against ptm.PrimaryCols on whole rows and columns of the cost table;
  n = 17 001             the defaults against the DEFINITION: tests/bellman_audit.py audits sampled Bellman cells of the device table
                         with the columns of ptm.PrimaryCols (entry list only, no dense table, no library code), then the split vector
                         and its definition-level total; the secondary scan's first layer and last row against Secondary.column;
  n = 250 000            past the sweep's default reach: the same audit on top of the forced sweep.

Also the routing of everything outside the gates, and the plaid callers.

Every case asserts its route: the stat of the path that ran equals K - 1, its profile slot ticks and the sweep's does not -- or the
reverse.  The reference tables of a (pattern, partition) are computed once and shared by the cases that need them."""
import contextlib
import functools

import numpy as np
import pytest

import bellman_audit as ba
import plaid_total_model as ptm
from util import cp, banded, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu
M = cp.models
SUM, MAX = M.CP_COMBINE_SUM, M.CP_COMBINE_MAX
PRIM, SEC = ptm.PRIM, ptm.SEC
SP = cp.DynamicTotalSplitter
IN_GATE = [(0, 10, 1, 0, 100), (3, -2, 1, 5, 40), (0, 0, 0, 1, 1), (0, 0, 0, 7, 0), (1, -3, -1, 2, 2), (0, 0, 0, 100, 1), (0, 0, 0, 0, 1)]
ALPHAS = [5, 1, 9, 2, 7, 3, 8]
MODELS = {"i": [PRIM(*p) for p in IN_GATE], "f": [PRIM(*(float(v) for v in p)) for p in IN_GATE], "ak": [PRIM(3, -2, 1, 5, 40, alpha_k=ALPHAS)]}
SEC_SIGNS = [(3, 2, 1, 1, 7), (3, 2, 1, 4, 4), (0, -1, 2, 9, 2)]                  # b_local_net <, =, > b_remote_net
SEC_MODELS = [SEC(*p) for p in SEC_SIGNS] + [SEC(*(float(v) for v in SEC_SIGNS[0])), SEC(0, 1, 1, 2, 5, alpha_k=ALPHAS),
                                            SEC(0.0, 1.0, 1.0, 5.0, 2.0, alpha_k=[float(a) for a in ALPHAS])]

DEFAULTS = {"plaid_total": 1, "plaid_total_min_n": 1024, "plaid_scan_min_n": 1024, "plaid_total_scan_cells": 1 << 20,
            "plaid_total_scan_cols": 1024, "plaid_total_stair_cols": 1024, "force_brute": 0, "brute_max_n": 200000}
NEW = {"plaid_total_min_n": 0, "plaid_scan_min_n": 0}
SHRUNK = dict(NEW, plaid_total_scan_cells=8, plaid_total_scan_cols=4, plaid_total_stair_cols=4)


@contextlib.contextmanager
def options(hip, **opts):
    """set for a block; every option goes back to its default in a finally"""
    try:
        for name, v in opts.items():
            assert hip.set_option(name, v) == 0, name
        yield
    finally:
        for name in opts:
            hip.set_option(name, DEFAULTS[name])


@contextlib.contextmanager
def watched(hip):
    """-> a dict filled on exit: launches of the two slots and the two stats, counted from the start of the block"""
    seen = {}
    hip.set_option("stat_reset", 0)
    hip.prof_reset(); hip.prof_enable(True)
    try:
        yield seen
    finally:
        hip.prof_enable(False)
    p = hip.prof_get()
    seen.update(new=p["dp_plaid_total"]["launches"], brute=p["dp_brute"]["launches"], total=hip.get_stat("plaid_total_layers"),
                scan=hip.get_stat("plaid_scan_layers"))


def on_total(seen, K):
    return seen["total"] == K - 1 and seen["scan"] == 0 and seen["new"] > 0 and seen["brute"] == 0


def on_scan(seen, K):
    return seen["scan"] == K - 1 and seen["total"] == 0 and seen["new"] > 0 and seen["brute"] == 0


def on_sweep(seen):
    return seen["total"] == 0 and seen["scan"] == 0 and seen["new"] == 0 and seen["brute"] > 0


def tables(hip, A, K, mdl, Pi, combine=SUM):
    rp, keep = cp.api._rowpart(Pi)
    rc, ptr, cst = hip.dynamic_tables(A, K, combine, mdl.marshal(), rp)
    assert rc == 0, hip.last_error()
    return ptr, cst


def same_tables(K, a, b):
    (p1, c1), (p2, c2) = a, b
    n = p1.shape[0] - 1
    return (c1.dtype == c2.dtype and np.array_equal(c1[:, :K - 1], c2[:, :K - 1]) and np.array_equal(p1[:, :K - 1], p2[:, :K - 1])
            and c1[n, K - 1] == c2[n, K - 1] and p1[n, K - 1] == p2[n, K - 1])


def check_tables(got, want, K):
    """every cell of the layers < K and row n of layer K against ([cst of layer k], [ptr of layer k, 0-based])"""
    (ptr, cst), (wc, wp) = got, want
    n = ptr.shape[0] - 1
    for k in range(1, K):
        assert cst.dtype == wc[k - 1].dtype and np.array_equal(cst[:, k - 1], wc[k - 1]), k
        assert np.array_equal(ptr[:, k - 1], wp[k - 1] + 1), k
    assert cst[n, K - 1] == wc[K - 1][n] and ptr[n, K - 1] == wp[K - 1][n] + 1, K


def unravel(ptr, K):
    """the split vector of a (n + 1) x K argmin table (1-based, as the library's)"""
    at = ptr.shape[0] - 1
    spl = [at + 1]
    for k in range(K, 0, -1):
        at = int(ptr[at, k - 1]) - 1
        spl.append(at + 1)
    return spl[::-1]


# ---------------------------------------------------------------- patterns and partitions
def _from_dense(D):
    m, n = D.shape
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


@functools.lru_cache(maxsize=None)
def pattern(n, seed=1):
    """m = 400 + n % 7 rows (m != n), 30 % empty columns, one column of 400 entries"""
    rng = np.random.default_rng(seed + n)
    m = 400 + n % 7
    D = rng.random((m, n)) < 0.02
    D[:, rng.random(n) < 0.3] = False
    D[:400, n // 3] = True
    return _from_dense(D)


def split_part(m, K=7):
    """a SplitPartition with an empty part (4): that part holds no column at all, Lk = 0"""
    cuts = np.linspace(1, m + 1, K + 1).astype(np.int64)
    cuts[4] = cuts[3]
    return cp.SplitPartition(K, cuts)


def map_part(m, K=7, seed=5):
    """a MapPartition in no order whose part 3 owns nothing"""
    asg = np.random.default_rng(seed).integers(1, K + 1, m)
    asg[asg == 3] = 6
    return cp.MapPartition(K, asg.astype(np.int64))


PARTS = {"split": split_part, "map": map_part}


@functools.lru_cache(maxsize=None)
def counts(n, part):
    A = pattern(n)
    return ptm.Primary(A, PARTS[part](A.m))


@functools.lru_cache(maxsize=None)
def literal(n, part, which, mi, K=7):
    T = counts(n, part)
    mdl = MODELS[which][mi]
    return ptm.literal_dp(lambda k: T.table(mdl, k), K, n)


def band_owner(m, K, seed, stray=0.1):
    """K bands along the diagonal, one row in ten strayed to a random part"""
    rng = np.random.default_rng(seed)
    own = 1 + (np.arange(m, dtype=np.int64) * K) // m
    s = rng.random(m) < stray
    own[s] = rng.integers(1, K + 1, int(s.sum()))
    return cp.MapPartition(K, own)


# ---------------------------------------------------------------- 1. tables bit for bit against the literal DP
@pytest.mark.parametrize("part", ["split", "map"])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_tables_bit_for_bit_against_the_literal_dp(hip, orc, n, part):
    T = counts(n, part)
    A, Pi = T.A, T.Pi
    assert A.m != A.n and int(np.diff(A.colptr).max()) == 400 and int((np.diff(A.colptr) == 0).sum()) > 0
    assert any(not T.local[k].any() for k in T.local)                          # a part without any column
    cases = [("i", mi) for mi in range(len(MODELS["i"]))] + [("ak", 0)]
    if n <= 65:
        cases += [("f", mi) for mi in range(len(MODELS["f"]))]
    with options(hip, **SHRUNK):
        for which, mi in cases:
            mdl = MODELS[which][mi]
            wc, wp = literal(n, part, which, mi)
            for K in (2, 7):
                with watched(hip) as seen:
                    got = tables(hip, A, K, mdl, Pi)
                assert on_total(seen, K), (seen, which, mi, K)
                check_tables(got, (wc[:K], wp[:K]), K)
            with watched(hip) as seen:
                spl = cp.partition_stripe(A, 7, SP(mdl), Pi, backend=hip)
            assert on_total(seen, 7), seen
            assert spl.spl.tolist() == ptm.unravel(wp, n), (n, part, which, mi)
        for mdl in (MODELS["i"][0], MODELS["i"][1]):                           # the CPU oracle's split vector
            for K in (2, 7):
                assert cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip) == cp.partition_stripe(A, K, SP(mdl), Pi, backend=orc)


# ---------------------------------------------------------------- 2. chunks and level limits
def test_more_than_one_chunk_per_level_row(hip):
    n, K = 1000, 5
    T = counts(n, "map")
    with options(hip, **SHRUNK):
        for mi in (0, 1, 5):
            mdl = MODELS["i"][mi]
            wc, wp = literal(n, "map", "i", mi, K)
            with watched(hip) as seen:
                got = tables(hip, T.A, K, mdl, T.Pi)
            assert on_total(seen, K), seen
            check_tables(got, (wc, wp), K)


@pytest.mark.parametrize("n", [10500, 17000])
def test_defaults_against_the_device_sweep_with_the_launch_cap(hip, n):
    """the limits as shipped.  At n = 17 000 the depth-1 rectangle has more than 8 192 rows, so its first level has more than
    LWS_LDS_ROWS = 4 096 rows and takes the count-and-scan branch.  The device sweep is the second opinion."""
    K = 4
    A = suitesparse_shaped(n, 6, 3, m=n + 11)
    Pi = band_owner(A.m, K, 4)
    cap = ptm.launch_cap(n, DEFAULTS["plaid_total_stair_cols"])
    for mdl in (MODELS["i"][0], MODELS["i"][1], MODELS["ak"][0]):
        with options(hip, **NEW):
            with watched(hip) as seen:
                new = tables(hip, A, K, mdl, Pi)
            assert on_total(seen, K), seen
            with watched(hip) as two:
                tables(hip, A, 2, mdl, Pi)
            with watched(hip) as three:
                tables(hip, A, 3, mdl, Pi)
            # K = 3 adds one full layer (rows 0 .. n) to K = 2: within D (4 L + 2) + 1 and the two preparation steps
            assert 0 < three["new"] - two["new"] <= cap and 0 < two["new"] <= cap + 3, (two, three, cap)
            got = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
        with options(hip, force_brute=1):
            with watched(hip) as swept:
                old = tables(hip, A, K, mdl, Pi)
            assert on_sweep(swept), swept
        assert same_tables(K, new, old), mdl._params()
        assert got.spl.tolist() == unravel(old[0], K)


# ---------------------------------------------------------------- 3. the secondary scan
def sec_split(m, K, seed):
    rng = np.random.default_rng(seed)
    return cp.SplitPartition(K, np.concatenate([[1], np.sort(rng.integers(1, m + 2, K - 1)), [m + 1]]).astype(np.int64))


@pytest.mark.parametrize("n", [1022, 1023, 1024])
def test_scan_at_the_tile_edges(hip, n):
    """n + 1 one below, at and one above the scan's tile of 1024 values; K = 5 < Pi.K = 8"""
    A = suitesparse_shaped(n, 6, 21, m=500)
    Pi, K = sec_split(A.m, 8, 22), 5
    S = ptm.Secondary(A, Pi)
    for mdl in SEC_MODELS:
        want = ptm.scan_dp(S, mdl, K)
        with options(hip, **NEW):
            with watched(hip) as seen:
                got = tables(hip, A, K, mdl, Pi)
            assert on_scan(seen, K), seen
            spl = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
        check_tables(got, want, K)
        with options(hip, force_brute=1):
            with watched(hip) as swept:
                old = tables(hip, A, K, mdl, Pi)
            assert on_sweep(swept), swept
        assert same_tables(K, got, old), mdl._params()
        assert spl.spl.tolist() == unravel(old[0], K)


def test_scan_with_more_tiles_than_one_strip_of_the_second_level(hip):
    """n + 1 > 1024 * 1024, nnz = 3 n: the block aggregates are scanned in two strips with a carry.  Past brute_max_n the scan runs at
    the default options; the scan restated in numpy is the check."""
    n, m, K = 1024 * 1024 + 2, 1000, 3
    rng = np.random.default_rng(31)
    rows = np.sort(np.stack([rng.integers(1, 334, n), 333 + rng.integers(1, 334, n), 666 + rng.integers(1, 335, n)], axis=1), axis=1).reshape(-1)
    A = cp.SparseMatrixCSC(m, n, 1 + 3 * np.arange(n + 1, dtype=np.int64), rows.astype(np.int64))
    Pi = sec_split(m, 4, 32)
    S = ptm.Secondary(A, Pi)
    for mdl in (SEC(5, 1, 1, 1, 3), SEC(0.0, 0.0, 0.0, 4.0, 1.0)):
        with watched(hip) as seen:
            got = tables(hip, A, K, mdl, Pi)
        assert on_scan(seen, K), seen
        check_tables(got, ptm.scan_dp(S, mdl, K), K)


# ---------------------------------------------------------------- 4. routing
def test_routing(hip, orc):
    n, K = 2000, 4
    A = suitesparse_shaped(n, 6, 5, m=n + 3)
    Pi = band_owner(A.m, K, 6)
    T = cp.adjointpattern(A, backend=hip)
    Phi = sec_split(T.m, K, 7)

    def swept_answer(X, meth, P):
        with options(hip, force_brute=1):
            return cp.partition_stripe(X, K, meth, P, backend=hip)

    # on the new paths once asked for, with the sweep's answers
    with options(hip, **NEW):
        for mdl in (MODELS["i"][0], MODELS["f"][1]):
            with watched(hip) as seen:
                got = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
            assert on_total(seen, K), seen
            assert got == swept_answer(A, SP(mdl), Pi)
        with watched(hip) as seen:
            got = cp.partition_stripe(T, K, SP(SEC_MODELS[0]), Phi, backend=hip)
        assert on_scan(seen, K), seen
        assert got == swept_answer(T, SP(SEC_MODELS[0]), Phi)

    # at the defaults: on the new paths from the measured crossover on, on the sweep below it
    assert n >= DEFAULTS["plaid_total_min_n"] and n >= DEFAULTS["plaid_scan_min_n"]
    for X, mdl, P, on in ((A, MODELS["i"][0], Pi, on_total), (T, SEC_MODELS[0], Phi, on_scan)):
        with watched(hip) as seen:
            got = cp.partition_stripe(X, K, SP(mdl), P, backend=hip)
        assert on(seen, K), seen
        assert got == swept_answer(X, SP(mdl), P)
    B = suitesparse_shaped(DEFAULTS["plaid_total_min_n"] - 1, 6, 12, m=A.m)
    TB = cp.adjointpattern(suitesparse_shaped(n, 6, 12, m=DEFAULTS["plaid_scan_min_n"] - 1), backend=hip)      # (its columns: those rows)
    assert B.n < DEFAULTS["plaid_total_min_n"] and TB.n < DEFAULTS["plaid_scan_min_n"]
    for X, mdl, P in ((B, MODELS["i"][0], Pi), (TB, SEC_MODELS[0], sec_split(TB.m, K, 13))):
        with watched(hip) as seen:
            got = cp.partition_stripe(X, K, SP(mdl), P, backend=hip)
        assert on_sweep(seen), seen
        assert got == swept_answer(X, SP(mdl), P)

    # outside the gates: the sweep, its answers, and its refusal where no sweep is allowed
    stay = [(A, PRIM(0, 0, 0, -1, 1), Pi, {}), (A, PRIM(0, 0, 0, 1, -1), Pi, {}), (A, PRIM(0.5, 0.25, 1.0, 1.5, 2.5), Pi, {}),
            (A, MODELS["i"][0], Pi, {"plaid_total": 0}), (A, MODELS["i"][0], Pi, {"force_brute": 1}), (A, PRIM(2 ** 58, 0, 1, 3, 1), Pi, {}),
            (T, SEC(0.5, 0.25, 1.0, 1.5, 2.5), Phi, {}), (T, SEC_MODELS[0], Phi, {"plaid_total": 0}), (T, SEC(2 ** 58, 0, 1, 3, 1), Phi, {})]
    for X, mdl, P, opts in stay:
        with options(hip, **dict(NEW, **opts)):
            with watched(hip) as seen:
                got = cp.partition_stripe(X, K, SP(mdl), P, backend=hip)
            assert on_sweep(seen), (mdl._params(), opts, seen)
            with options(hip, brute_max_n=100):
                with pytest.raises(NotImplementedError, match="n too large"):
                    cp.partition_stripe(X, K, SP(mdl), P, backend=hip)
        assert got == swept_answer(X, SP(mdl), P), (mdl._params(), opts)
    assert cp.partition_stripe(A, K, SP(PRIM(0, 0, 0, -1, 1)), Pi, backend=hip) == cp.partition_stripe(A, K, SP(PRIM(0, 0, 0, -1, 1)), Pi, backend=orc)

    # the max objective never takes them
    for X, mdl, P in ((A, MODELS["i"][0], Pi), (T, SEC_MODELS[0], Phi)):
        with options(hip, **NEW):
            with watched(hip) as seen:
                got = cp.partition_stripe(X, K, cp.DynamicBottleneckSplitter(mdl), P, backend=hip)
            assert on_sweep(seen), seen
            ptr, cst = tables(hip, X, K, mdl, P, MAX)
        assert got.spl.tolist() == unravel(ptr, K)

    # constrained forms and the chunker order stay refused
    with options(hip, **NEW):
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, K, SP(cp.ConstrainedCost(MODELS["i"][0], cp.VertexCount(), 900)), Pi, backend=hip)
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, K, cp.DynamicTotalChunker(MODELS["i"][0]), Pi, backend=hip)


def test_brute_max_n_100_answers_inside_the_gate_and_refuses_outside(hip):
    n, K = 20000, 3
    A = suitesparse_shaped(n, 6, 8, m=n + 5)
    Pi = band_owner(A.m, K, 9)
    T = cp.adjointpattern(A, backend=hip)
    Phi = sec_split(T.m, K, 10)
    with options(hip, brute_max_n=100):
        with watched(hip) as seen:
            got = cp.partition_stripe(A, K, SP(MODELS["i"][0]), Pi, backend=hip)
        assert on_total(seen, K), seen
        with watched(hip) as seen:
            got2 = cp.partition_stripe(T, K, SP(SEC_MODELS[0]), Phi, backend=hip)
        assert on_scan(seen, K), seen
        for X, mdl, P in ((A, PRIM(0, 10, 1, -3, 100), Pi), (T, SEC(0.5, 0.25, 1.0, 1.5, 2.5), Phi)):
            with pytest.raises(NotImplementedError, match="n too large"):
                cp.partition_stripe(X, K, SP(mdl), P, backend=hip)
    with options(hip, force_brute=1):
        assert got == cp.partition_stripe(A, K, SP(MODELS["i"][0]), Pi, backend=hip)
        assert got2 == cp.partition_stripe(T, K, SP(SEC_MODELS[0]), Phi, backend=hip)



# ---------------------------------------------------------------- 5. the defaults against the definition (tests/bellman_audit.py)
def holed(n, seed):
    """suitesparse_shaped(n, 6, seed, m = n + 11) with a run of n // 40 consecutive columns emptied (a model without a vertex and a pin
    term ties there) and one column of n // 4 further entries"""
    B = suitesparse_shaped(n, 6, seed, m=n + 11)
    m = B.m
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(B.colptr))
    rows = np.asarray(B.rowval, dtype=np.int64) - 1
    lo, run, hub = n // 3, n // 40, (2 * n) // 3
    keep = ~((cols >= lo) & (cols < lo + run))
    pick = np.random.default_rng(seed).choice(m, n // 4, replace=False)
    key = np.unique(np.concatenate([cols[keep], np.full(pick.size, hub)]) * m + np.concatenate([rows[keep], pick]))
    c, r = key // m, key % m
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, r + 1)


def check_holed(A):
    n, deg = A.n, np.diff(A.colptr)
    lo, run = n // 3, n // 40
    assert A.m == n + 11 and run > 0 and not deg[lo:lo + run].any() and deg[lo - 1] > 0 and deg[lo + run] > 0
    assert int(deg.max()) >= n // 4 and int(deg.argmax()) == (2 * n) // 3


@functools.lru_cache(maxsize=None)
def sized(n):
    A = holed(n, 3)
    check_holed(A)
    return A


def lead_split(m):
    """a SplitPartition of 7 parts whose first ones are 600 rows each (a few widths of the pattern's band), part 4 empty: the parts of a
    K = 5 run then have their rows in front of nearly every audited row, and a part that follows its rows beats one part for all"""
    return cp.SplitPartition(7, np.array([1, 601, 1201, 1801, 1801, 2401, 3001, m + 1], dtype=np.int64))


AUDIT_PARTS = {"band": lambda m: band_owner(m, 5, 4), "lead_split": lead_split}
AUDIT_MODELS = {"i0": MODELS["i"][0], "i1": MODELS["i"][1], "no_vertex": MODELS["i"][5], "alpha_k": MODELS["ak"][0], "float64": MODELS["f"][1]}


def audit_primary(hip, A, Pi, mdl, K, seed, nrand):
    """one run at the options as they stand: route, sampled Bellman cells, split vector, definition-level total -> the audit's counts"""
    n = A.n
    with watched(hip) as seen:
        ptr, cst = tables(hip, A, K, mdl, Pi)
    assert on_total(seen, K), seen
    C = ptm.PrimaryCols(A, Pi, mdl)
    rows = ba.audit_rows(n, DEFAULTS["plaid_total_stair_cols"], seed, nrand)
    counts = ba.audit(ptr, cst, K, C.row, C.column, rows)
    assert len(rows) >= 24 and counts["cells"] == len(rows) * (K - 2) + 1, (len(rows), counts)
    with watched(hip) as seen:
        got = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
    assert on_total(seen, K), seen
    spl = got.spl.tolist()
    assert spl == unravel(ptr, K)
    with np.errstate(over="ignore"):
        total = sum(C.row(spl[k], k + 1, upto=spl[k + 1])[-1] for k in range(K))
    assert total == cst[n, K - 1], (total, cst[n, K - 1])
    return counts


@pytest.mark.parametrize("part", list(AUDIT_PARTS))
def test_audit_at_the_default_limits(hip, part):
    """n = 17 001 (the depth-1 rectangle takes the count-and-scan branch past LWS_LDS_ROWS), K = 5, no option set: sampled Bellman cells
    against the definition at the rows where the engine changes its path and at 32 random rows.  (The chunker order of this kind is
    refused, test_routing, so there is no third closing check.)  Under lead_split the model i0 has an interior argmin in more than
    half of its audited cells (164 of 283; a DP in numpy over PrimaryCols columns alone gives the same share); under the five even
    bands no model does, because a fifth of the pattern's entries are spread over all rows and one part for everything wins.  The
    model without vertex and pin terms ties."""
    A, K = sized(17_001), 5
    assert A.n > DEFAULTS["plaid_total_min_n"]
    Pi = AUDIT_PARTS[part](A.m)
    for name, mdl in AUDIT_MODELS.items():
        counts = audit_primary(hip, A, Pi, mdl, K, 17, 32)
        print(part, name, "audited", counts)
        if name == "no_vertex":
            assert counts["tied"] >= 1, counts
        if name == "i0" and part == "lead_split":
            assert 2 * counts["interior"] >= counts["cells"], counts


def test_audit_with_layers_whose_part_owns_no_row(hip):
    """K = Pi.K + 2 = 7: the layers 6 and 7 belong to parts that own no row (every net remote)"""
    A = sized(17_001)
    Pi = band_owner(A.m, 5, 4)
    for name in ("i1", "alpha_k"):
        counts = audit_primary(hip, A, Pi, AUDIT_MODELS[name], Pi.K + 2, 18, 32)
        print(name, "audited", counts)
        assert counts["interior"] >= 1, counts


def test_secondary_first_layer_and_last_row_against_the_definition(hip):
    """the scan's first layer (every cell) and its last row, with f(j, j', k) straight from the definition (Secondary.column)"""
    T = cp.adjointpattern(sized(17_001), backend=hip)
    K = 5
    Phi = sec_split(T.m, K, 23)
    S = ptm.Secondary(T, Phi)
    for mdl in SEC_MODELS:
        with watched(hip) as seen:
            ptr, cst = tables(hip, T, K, mdl, Phi)
        assert on_scan(seen, K), seen
        counts = ba.audit(ptr, cst, K, lambda j, k: S.first(mdl), lambda jp, k: S.column(mdl, jp, k), [])
        assert counts["cells"] == 1


@pytest.mark.parametrize("part", ["band7", "split"])
def test_primary_oracle_against_the_definition_at_20011(hip, part):
    """the cells the sweep and the rectangle engine both evaluate: cp.oracle_stripe on 64 whole columns and 16 whole rows of the cost
    table (the fixed ends: 1, 2, n, n + 1, columns where colptr crosses a multiple of 2048, random) against ptm.PrimaryCols"""
    A = sized(20_011)
    n = A.n
    assert (n + 2).bit_length() == 15 and A.nnz + n > 10 * 2048               # H = cllog2(n + 2) = 15 wavelet levels
    Pi = {"band7": band_owner(A.m, 7, 5), "split": split_part(A.m)}[part]
    rng = np.random.default_rng(2011)
    ends, starts = ba.fixed_ends(A, rng, 64), ba.fixed_ends(A, rng, 16)
    j, jp = ba.line_pairs(n, ends, starts)
    assert j.size >= 700_000
    cases = [(MODELS["i"][1], 2), (MODELS["ak"][0], 3), (MODELS["f"][1], Pi.K), (MODELS["i"][0], 4)]
    for mdl, k in cases:
        C = ptm.PrimaryCols(A, Pi, mdl)
        want = np.concatenate([C.column(int(e), k) for e in ends] + [C.row(int(s), k) for s in starts])
        got = cp.oracle_stripe(cp.NoHint(), mdl, A, Pi, backend=hip)(j, jp, k)
        bad = np.nonzero(got != want)[0]
        assert got.dtype == want.dtype and bad.size == 0, (part, mdl._params(), k, j[bad[:5]], jp[bad[:5]], got[bad[:5]], want[bad[:5]])
    # a part number past Pi.K is a violated precondition of the oracle entry; the DP evaluates such layers itself
    # (test_audit_with_layers_whose_part_owns_no_row)
    with pytest.raises(AssertionError, match="out of range"):
        cp.oracle_stripe(cp.NoHint(), MODELS["i"][1], A, Pi, backend=hip)(j[:4], jp[:4], Pi.K + 1)


# ---------------------------------------------------------------- 6. at size
@pytest.fixture(scope="module")
def large():
    A = banded(250_000, 5, 0.9, 1)
    return A, band_owner(A.m, 3, 2)


def test_primary_past_brute_max_n(hip, large):
    """n = 250 000 > brute_max_n, the defaults: CP_EUNSUPPORTED ("n too large") before this path existed"""
    (A, Pi), K = large, 3
    n, mdl = A.n, PRIM(0, 10, 1, 0, 100)
    assert 9 * n <= A.nnz <= 11 * n and n > DEFAULTS["brute_max_n"]
    with watched(hip) as seen:
        got = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
    assert on_total(seen, K), seen
    spl = got.spl.tolist()
    assert spl[0] == 1 and spl[-1] == n + 1 and all(a < b for a, b in zip(spl, spl[1:])), spl      # K distinct parts, not [1, n + 1, ...]
    ptr, cst = tables(hip, A, K, mdl, Pi)
    assert cst[n, K - 1] == cp.total_value(A, got, mdl, Pi, backend=hip)
    with options(hip, force_brute=1, brute_max_n=1 << 20):
        with watched(hip) as swept:
            old = tables(hip, A, K, mdl, Pi)
        assert on_sweep(swept), swept
    assert same_tables(K, (ptr, cst), old) and spl == unravel(old[0], K)
    # optimality, from the definition: sampled Bellman cells of the full layer and the last row
    C = ptm.PrimaryCols(A, Pi, mdl)
    rows = ba.audit_rows(n, DEFAULTS["plaid_total_stair_cols"], 250, 8)
    counts = ba.audit(ptr, cst, K, C.row, C.column, rows)
    print("audited", counts)
    assert len(rows) >= 24 and counts["cells"] == len(rows) * (K - 2) + 1 and counts["interior"] >= 1, (len(rows), counts)


def test_secondary_past_brute_max_n(hip, large):
    (A, _), K = large, 3
    T = cp.adjointpattern(A, backend=hip)
    n, mdl = T.n, SEC(0, 10, 1, 0, 100)
    Phi = cp.SplitPartition(K, np.linspace(1, T.m + 1, K + 1).astype(np.int64))
    with watched(hip) as seen:
        got = cp.partition_stripe(T, K, SP(mdl), Phi, backend=hip)
    assert on_scan(seen, K), seen
    spl = got.spl.tolist()
    assert spl[0] == 1 and spl[-1] == n + 1 and all(a < b for a, b in zip(spl, spl[1:])), spl
    ptr, cst = tables(hip, T, K, mdl, Phi)
    assert cst[n, K - 1] == cp.total_value(T, got, mdl, Phi, backend=hip)
    with options(hip, force_brute=1, brute_max_n=1 << 20):
        with watched(hip) as swept:
            old = tables(hip, T, K, mdl, Phi)
        assert on_sweep(swept), swept
    assert same_tables(K, (ptr, cst), old) and spl == unravel(old[0], K)


# ---------------------------------------------------------------- 7. callers
def test_alternating_partitioner_on_the_new_routes(hip):
    n, K = 12000, 4
    A = suitesparse_shaped(n, 6, 11)
    net, comm, local = cp.AffineConnectivityModel(0, 10, 1, 100), PRIM(0, 10, 1, 0, 100), SEC(0, 10, 1, 0, 100)
    meth = cp.AlternatingPartitioner(SP(net), SP(local), SP(comm))
    with options(hip, **NEW):
        with watched(hip) as seen:
            got = cp.partition_plaid(A, K, meth, backend=hip)
    assert seen["total"] == K - 1 and seen["scan"] == K - 1 and seen["brute"] == 0, seen
    with options(hip, plaid_total=0):
        with watched(hip) as seen:
            want = cp.partition_plaid(A, K, meth, backend=hip)
    assert seen["total"] == 0 and seen["scan"] == 0 and seen["brute"] > 0, seen
    assert all(a == b for a, b in zip(got, want))


def test_permuting_partitioner_with_a_row_partition(hip):
    """the relation of tests/test_gpu_permuting.py (PermutingPartitioner.jl:27-34), on the new route"""
    A = golden_matrices()["LPnetlib/lp_etamacro"]
    K = 4
    rcm = cp.CuthillMcKeePermuter()
    Pi = cp.partition_stripe(cp.adjointpattern(A, backend=hip), K, cp.EquiSplitter())
    inner = SP(PRIM(0, 10, 1, 100, 50))
    tau = cp.permute_stripe(A, rcm, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    with options(hip, **NEW):
        with watched(hip) as seen:
            got = cp.partition_stripe(A, K, cp.PermutingPartitioner(rcm, inner), Pi, backend=hip)
        assert on_total(seen, K), seen
        assert got == tau[cp.partition_stripe(B, K, inner, Pi, backend=hip)]
    with options(hip, force_brute=1):
        assert got == cp.partition_stripe(A, K, cp.PermutingPartitioner(rcm, inner), Pi, backend=hip)
