"""GPU tests of the total objective of the symmetric cost family on the divide and conquer of csrc/sym_total.hip (path SymTotal).

What referees what, by size:

  n <= 1000     tables bit for bit against the literal DP over the dense count tables of tests/sym_model.py, with the limits shrunk so
                that small patterns run levels, stair scans and whole-scanned rectangles, in both launch forms ("sym_total_batch" 1
                and 0); more than one 256-column chunk per level row;
  n = 17 000    the defaults as shipped past the LDS level limit against the device sweep (which counts with the same device
                structures), with the launch cap of the batched form;
  n = 17 001    the defaults again, now against the DEFINITION: tests/bellman_audit.py audits sampled Bellman cells of the device table
                with the columns of sm.Sym (entry list only, no dense table, no library code), then the split vector, its
                definition-level total and the chunker order;
  n = 250 000   past the sweep's reach: the same audit on top of the older inequalities.

Inside the gate of SymTotal every cost is alpha_k plus a subadditive function g of the column range (net and dianet are subadditive,
selfpin is superadditive with a non-positive weight, everything else is additive), so appending an empty part never costs more than
any other last part: cst[r, k] = alpha_1 + .. + alpha_k + g(0, r), the candidates p = 0 and p = r both attain it and the largest
minimiser is p = r.  No in-gate model of this family has an interior argmin; the audits therefore assert the whole closed form (every
cell of every layer, from Sym.row) next to the sampled cells, and that every audited cell with r >= 1 is tied.

Also: the routing of everything outside the gate, and the plaid callers.  The reference tables of a (pattern, model) are computed once
and shared by every case that needs them."""
import contextlib
import functools

import numpy as np
import pytest

import bellman_audit as ba
import sym_model as sm
import sym_total_model as stm
from test_gpu_symmetric import pattern, tables, MODELS_I, VARIANTS
from util import cp, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu
M = cp.models
SUM, MAX = M.CP_COMBINE_SUM, M.CP_COMBINE_MAX
SC, MSC, SEC = cp.AffineSymmetricConnectivityModel, cp.AffineMonotonizedSymmetricConnectivityModel, cp.AffineSymmetricEdgeCutModel
IN_GATE = [(SC, (3, -2, 1, 5, 40)), (SC, (0, 0, 0, 0, 1)), (SC, (0, 1, 0, 2, 2)), (MSC, (0, 0, 1, 100, 2)), (MSC, (1, -3, -1, 1, 0)),
           (SEC, (1, 2, 3, 7)), (SEC, (0, 0, 0, 1)), (SEC, (0, -1, -2, -2))]
MODELS_IN = [c(*p) for c, p in IN_GATE]
MODELS_IN_F = [c(*(float(v) for v in p)) for c, p in IN_GATE]                # the integer-valued Float64 twins
ALPHAS = [5, 1, 9, 2, 7, 3, 8]
MODELS_AK = [SC(3, -2, 1, 5, 40, alpha_k=ALPHAS), MSC(0, 0, 1, 100, 2, alpha_k=ALPHAS), SEC(1, 2, 3, 7, alpha_k=ALPHAS)]
OUT_OF_GATE = [SC(0, 0, 0, 3, 1), MSC(0, 0, 1, -1, 2), SEC(0, 0, 1, 0)]
ONE_PER_KIND = [MODELS_IN[0], MODELS_IN[3], MODELS_IN[5]]
assert [type(a) for a in ONE_PER_KIND] == [type(a) for a in MODELS_I]

DEFAULTS = {"sym_total": 1, "sym_total_batch": 1, "sym_total_min_n": 10240, "sym_total_scan_cells": 1 << 20, "sym_total_scan_cols": 1024,
            "sym_total_stair_cols": 1024, "force_brute": 0, "brute_max_n": 200000}
SHRUNK = {"sym_total_min_n": 0, "sym_total_scan_cells": 8, "sym_total_scan_cols": 4, "sym_total_stair_cols": 4}


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
    """-> a dict filled on exit: launches of the two slots and the stat, counted from the start of the block"""
    seen = {}
    hip.set_option("stat_reset", 0)
    hip.prof_reset(); hip.prof_enable(True)
    try:
        yield seen
    finally:
        hip.prof_enable(False)
    p = hip.prof_get()
    seen.update(sym=p["dp_sym_total"]["launches"], brute=p["dp_brute"]["launches"], layers=hip.get_stat("sym_total_layers"))


@functools.lru_cache(maxsize=None)
def literal(n, variant, which, mi, K):
    """the literal DP in splitter order: ([cst of layer k], [ptr of layer k, 0-based]) for k = 1 .. K"""
    mdl = {"i": MODELS_IN, "f": MODELS_IN_F, "ak": MODELS_AK}[which][mi]
    T = tables(n, variant)
    cst, ptr = [sm.cost_table(T, mdl, 1)[0, :].copy()], [np.zeros(n + 1, dtype=np.int64)]
    for k in range(2, K + 1):
        c, p = sm.brute.layer(cst[-1], sm.cost_table(T, mdl, k))
        cst.append(c); ptr.append(p)
    return cst, ptr


def check_tables(hip, A, mdl, K, want):
    """every cell of the layers < K and row n of layer K; the run is SymTotal's: K - 1 layers, its slot ticks, the sweep's does not"""
    wc, wp = want
    n = A.n
    with watched(hip) as seen:
        rc, ptr, cst = hip.dynamic_tables(A, K, SUM, mdl.marshal(), None)
    assert rc == 0, hip.last_error()
    assert seen["layers"] == K - 1 and seen["sym"] > 0 and seen["brute"] == 0, seen
    for k in range(1, K):
        assert cst.dtype == wc[k - 1].dtype and np.array_equal(cst[:, k - 1], wc[k - 1]), (n, k, mdl._params())
        assert np.array_equal(ptr[:, k - 1], wp[k - 1] + 1), (n, k, mdl._params())
    assert cst[n, K - 1] == wc[K - 1][n] and ptr[n, K - 1] == wp[K - 1][n] + 1, (n, K, mdl._params())


@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_tables_bit_for_bit_against_the_literal_dp(hip, n, batch):
    v = VARIANTS[n % len(VARIANTS)]
    A, T = pattern(n, v), tables(n, v)
    cases = [("i", mi) for mi in range(len(MODELS_IN))] + [("ak", mi) for mi in range(len(MODELS_AK))]
    if n <= 65:
        cases += [("f", mi) for mi in range(len(MODELS_IN_F))]
    with options(hip, sym_total_batch=batch, **SHRUNK):
        for which, mi in cases:
            mdl = {"i": MODELS_IN, "f": MODELS_IN_F, "ak": MODELS_AK}[which][mi]
            for K in (2, 7):
                wc, wp = literal(n, v, which, mi, 7)
                check_tables(hip, A, mdl, K, (wc[:K], wp[:K]))
                orders = ("splitter",) if which == "ak" else ("splitter", "chunker")
                for order in orders:
                    meth = cp.DynamicTotalSplitter if order == "splitter" else cp.DynamicTotalChunker
                    with watched(hip) as seen:
                        got = cp.partition_stripe(A, K, meth(mdl), backend=hip)
                    assert seen["layers"] == K - 1 and seen["brute"] == 0, (seen, order)
                    assert np.array_equal(got.spl, sm.dp_partition(T, mdl, K, "sum", order)[0]), (n, which, mi, K, order)


@pytest.mark.parametrize("batch", [1, 0])
def test_more_than_one_chunk_per_level_row(hip, batch):
    n, K = 1000, 5
    A, T = pattern(n, "partial"), tables(n, "partial")
    with options(hip, sym_total_batch=batch, **SHRUNK):
        for mi in (0, 3, 5):
            mdl = MODELS_IN[mi]
            check_tables(hip, A, mdl, K, literal(n, "partial", "i", mi, K))
            got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
            assert np.array_equal(got.spl, sm.dp_partition(T, mdl, K, "sum")[0]), mi


def symmetrised(n, deg, seed, nnz=None):
    """the bench generator's pattern united with its transpose"""
    B = suitesparse_shaped(n, deg, seed, nnz=nnz)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(B.colptr))
    rows = np.asarray(B.rowval, dtype=np.int64) - 1
    key = np.unique(np.concatenate([cols * n + rows, rows * n + cols]))      # (column, row), sorted by column then row
    c, r = key // n, key % n
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, r + 1)


def same_tables(K, a, b):
    (rc1, p1, c1), (rc2, p2, c2) = a, b
    n = p1.shape[0] - 1
    return (rc1 == 0 and rc2 == 0 and np.array_equal(c1[:, :K - 1], c2[:, :K - 1]) and np.array_equal(p1[:, :K - 1], p2[:, :K - 1])
            and c1[n, K - 1] == c2[n, K - 1] and p1[n, K - 1] == p2[n, K - 1])


def unravel(ptr, K):
    """the split vector of a (n + 1) x K argmin table (1-based, as the library's)"""
    at = ptr.shape[0] - 1
    spl = [at + 1]
    for k in range(K, 0, -1):
        at = int(ptr[at, k - 1]) - 1
        spl.append(at + 1)
    return spl[::-1]


def test_defaults_past_the_lds_level_limit(hip):
    """n = 17 000: the depth-1 rectangle has more than 8 192 rows, so its first level has more than LWS_LDS_ROWS = 4 096 rows and takes
    the count-and-scan branch.  The device sweep is the second opinion (the Python tables are out of reach at this n)."""
    n, K = 17000, 4
    A = symmetrised(n, 6, 3)
    for mdl in ONE_PER_KIND:
        with watched(hip) as seen:
            new = hip.dynamic_tables(A, K, SUM, mdl.marshal(), None)
        assert seen["layers"] == K - 1 and seen["brute"] == 0, seen
        # K - 2 full layers and the last row, each within the cap of the batched form
        assert 0 < seen["sym"] <= (K - 1) * stm.launch_cap(n, DEFAULTS["sym_total_stair_cols"]), seen
        got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
        with options(hip, force_brute=1):
            with watched(hip) as swept:
                old = hip.dynamic_tables(A, K, SUM, mdl.marshal(), None)
            assert swept["layers"] == 0 and swept["sym"] == 0 and swept["brute"] > 0, swept
        assert same_tables(K, new, old), mdl._params()
        assert got.spl.tolist() == unravel(old[1], K)                       # the sweep's split vector, read off its argmin table


def test_full_layer_launch_cap(hip):
    """one full layer (rows 0 .. n) of the batched form stays within D (4 L + 2) + 1 launches: K = 3 runs one full layer and the last row"""
    n = 17000
    A = symmetrised(n, 6, 3)
    cap = stm.launch_cap(n, DEFAULTS["sym_total_stair_cols"])
    with watched(hip) as two:
        assert hip.dynamic_tables(A, 2, SUM, MODELS_IN[5].marshal(), None)[0] == 0
    with watched(hip) as three:
        assert hip.dynamic_tables(A, 3, SUM, MODELS_IN[5].marshal(), None)[0] == 0
    assert 0 < three["sym"] - two["sym"] <= cap and 0 < two["sym"] <= cap, (two, three, cap)
    with options(hip, sym_total_batch=0):
        with watched(hip) as each:
            assert hip.dynamic_tables(A, 3, SUM, MODELS_IN[5].marshal(), None)[0] == 0
    assert each["sym"] >= three["sym"], (each, three)                       # the per-rectangle form never launches less



# ---------------------------------------------------------------- the defaults against the definition (tests/bellman_audit.py)
def holed(n, seed):
    """symmetrised(n, 6, seed) with the columns and rows of n // 40 consecutive indices emptied (a model without a vertex term ties
    there) and one column and row of n // 4 further entries"""
    B = symmetrised(n, 6, seed)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(B.colptr))
    rows = np.asarray(B.rowval, dtype=np.int64) - 1
    lo, run, hub = n // 3, n // 40, (2 * n) // 3
    keep = ~(((cols >= lo) & (cols < lo + run)) | ((rows >= lo) & (rows < lo + run)))
    pick = np.random.default_rng(seed).choice(np.setdiff1d(np.arange(n), np.arange(lo, lo + run)), n // 4, replace=False)
    c = np.concatenate([cols[keep], np.full(pick.size, hub), pick])
    r = np.concatenate([rows[keep], pick, np.full(pick.size, hub)])
    key = np.unique(c * n + r)
    c, r = key // n, key % n
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, r + 1)


def check_holed(A):
    """the properties the audits rely on: symmetric, an empty run of n // 40 columns and rows, one column of at least n // 4 entries"""
    n = A.n
    deg = np.diff(A.colptr)
    cols = np.repeat(np.arange(n, dtype=np.int64), deg)
    rows = np.asarray(A.rowval, dtype=np.int64) - 1
    lo, run = n // 3, n // 40
    assert np.array_equal(np.sort(cols * n + rows), np.sort(rows * n + cols))
    assert run > 0 and not deg[lo:lo + run].any() and not ((rows >= lo) & (rows < lo + run)).any()
    assert deg[lo - 1] > 0 and deg[lo + run] > 0 and int(deg.max()) >= n // 4 and int(deg.argmax()) == (2 * n) // 3


@functools.lru_cache(maxsize=None)
def audit_pattern():
    A = holed(17_001, 3)
    check_holed(A)
    return A


def alpha_sums(mdl, K, dt):
    ak = mdl.alpha_k
    return np.cumsum(np.array([mdl.alpha if ak is None else ak[k] for k in range(K)], dtype=dt))


def audit_tables(A, mdl, K, ptr, cst, seed, nrand):
    """the sampled Bellman cells, and the closed form of the whole table (module docstring) -> the audit's counts"""
    n = A.n
    S = sm.Sym(A, mdl)
    rows = ba.audit_rows(n, DEFAULTS["sym_total_stair_cols"], seed, nrand)
    counts = ba.audit(ptr, cst, K, S.row, S.column if mdl.alpha_k is not None else ba.same_for_all_k(S.column), rows)
    assert len(rows) >= 24 and counts["cells"] == len(rows) * (K - 2) + 1, (len(rows), counts)
    # every audited cell with r >= 1 has the two minimisers p = 0 and p = r, and none is interior
    assert counts["tied"] == counts["cells"] - (K - 2) * int(rows[0] == 0) and counts["interior"] == 0, counts
    sums = alpha_sums(mdl, K, cst.dtype)
    for k in range(2, K):
        assert np.array_equal(cst[:, k - 1], S.row(1, k) + sums[k - 2]), k
        assert np.array_equal(ptr[:, k - 1], np.arange(1, n + 2)), k
    assert cst[n, K - 1] == S.row(1, K)[n] + sums[K - 2] and ptr[n, K - 1] == n + 1
    return counts, S


AUDITED = {"sym_conn": (ONE_PER_KIND[0], 1), "mono_sym": (ONE_PER_KIND[1], 1), "edge_cut": (ONE_PER_KIND[2], 1), "alpha_k": (MODELS_AK[1], 1),
           "float64": (MODELS_IN_F[0], 1), "ties": (SEC(0, 0, 0, 1), 1), "per_rectangle": (ONE_PER_KIND[0], 0)}


@pytest.mark.parametrize("case", list(AUDITED))
def test_audit_at_the_default_limits(hip, case):
    """n = 17 001 (the depth-1 rectangle takes the count-and-scan branch past LWS_LDS_ROWS), K = 5, no option set but the launch form:
    sampled Bellman cells against the definition at the rows where the engine changes its path and at 32 random rows; the split
    vector is the table's, its total summed from definition-level part costs is cst[n, K - 1]; the chunker order, which fills the same
    tables for a model without alpha_k, returns the same split."""
    (mdl, batch), K = AUDITED[case], 5
    A = audit_pattern()
    n = A.n
    assert n > DEFAULTS["sym_total_min_n"]
    with options(hip, sym_total_batch=batch):
        with watched(hip) as seen:
            rc, ptr, cst = hip.dynamic_tables(A, K, SUM, mdl.marshal(), None)
        assert rc == 0, hip.last_error()
        assert seen["layers"] == K - 1 and seen["sym"] > 0 and seen["brute"] == 0, seen
        counts, S = audit_tables(A, mdl, K, ptr, cst, 17, 32)
        print(case, "audited", counts)
        orders = (cp.DynamicTotalSplitter,) if mdl.alpha_k is not None else (cp.DynamicTotalSplitter, cp.DynamicTotalChunker)
        for meth in orders:
            with watched(hip) as seen:
                got = cp.partition_stripe(A, K, meth(mdl), backend=hip)
            assert seen["layers"] == K - 1 and seen["sym"] > 0 and seen["brute"] == 0, (seen, meth.__name__)
            spl = got.spl.tolist()
            assert spl == unravel(ptr, K), meth.__name__
    with np.errstate(over="ignore"):
        total = sum(S.row(spl[k], k + 1, upto=spl[k + 1])[-1] for k in range(K))
    assert total == cst[n, K - 1], (total, cst[n, K - 1])


def test_routing(hip):
    n, K = 2000, 4
    A = symmetrised(n, 6, 5)
    SP, CH = cp.DynamicTotalSplitter, cp.DynamicTotalChunker

    def swept_answer(mdl, meth):
        with options(hip, force_brute=1):
            return cp.partition_stripe(A, K, meth(mdl), backend=hip)

    # refused before this path existed: no sweep allowed, default sym_total_min_n, an in-gate model of each kind (n is below the default
    # sym_total_min_n, the measured crossover with the sweep; where the sweep is refused the path runs from 1024 columns on)
    for mdl in ONE_PER_KIND + [MODELS_IN_F[0]]:
        for meth in (SP, CH):
            with options(hip, brute_max_n=0):
                with watched(hip) as seen:
                    got = cp.partition_stripe(A, K, meth(mdl), backend=hip)
            assert seen["layers"] == K - 1 and seen["sym"] > 0 and seen["brute"] == 0, seen
            assert got == swept_answer(mdl, meth), mdl._params()

    # where the sweep is allowed it keeps the sizes below the crossover
    assert n < DEFAULTS["sym_total_min_n"]
    for mdl in ONE_PER_KIND:
        with watched(hip) as seen:
            got = cp.partition_stripe(A, K, SP(mdl), backend=hip)
        assert seen["layers"] == 0 and seen["sym"] == 0 and seen["brute"] > 0, seen
        assert got == swept_answer(mdl, SP)

    # on the sweep, with the sweep's answers, and refused where no sweep is allowed
    B = pattern(257, "partial")
    stay = [(A, mdl, {}) for mdl in OUT_OF_GATE]
    stay += [(A, ONE_PER_KIND[0], {"sym_total": 0}), (A, ONE_PER_KIND[2], {"force_brute": 1}),
             (A, SC(0.5, 0.25, 0.0, 1.5, 2.5), {}), (A, MSC(0, 1, 2, 2**58, 1), {}), (A, SEC(0, 1, -2**58, 3), {}),
             (B, ONE_PER_KIND[1], {})]
    for X, mdl, opts in stay:
        with options(hip, **opts):
            with watched(hip) as seen:
                got = cp.partition_stripe(X, K, SP(mdl), backend=hip)
            assert seen["layers"] == 0 and seen["sym"] == 0 and seen["brute"] > 0, (mdl._params(), opts, seen)
            with options(hip, brute_max_n=0):
                with pytest.raises(NotImplementedError, match="n too large"):
                    cp.partition_stripe(X, K, SP(mdl), backend=hip)
        with options(hip, force_brute=1):
            assert got == cp.partition_stripe(X, K, SP(mdl), backend=hip)
    want = sm.dp_partition(tables(257, "partial"), ONE_PER_KIND[1], K, "sum")[0]
    assert np.array_equal(cp.partition_stripe(B, K, SP(ONE_PER_KIND[1]), backend=hip).spl, want)

    # the max objective never takes it
    for mdl in ONE_PER_KIND:
        with options(hip, sym_total_min_n=0):
            with watched(hip) as seen:
                cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(mdl), backend=hip)
        assert seen["layers"] == 0 and seen["sym"] == 0, seen


@pytest.fixture(scope="module")
def large():
    return symmetrised(250_000, 5, 1, nnz=1_300_000)


@pytest.mark.parametrize("mdl", [SEC(0, 0, 0, 1), MSC(0, 0, 1, 100, 2)], ids=["edge_cut", "mono_sym"])
def test_past_brute_max_n(hip, large, mdl):
    """n = 250 000 > brute_max_n: CP_EUNSUPPORTED before this path existed"""
    A, K = large, 8
    n = A.n
    assert 9 * n <= A.nnz <= 11 * n
    with watched(hip) as seen:
        rc, ptr, cst = hip.dynamic_tables(A, K, SUM, mdl.marshal(), None)
    assert rc == 0, hip.last_error()
    assert seen["layers"] == K - 1 and seen["brute"] == 0, seen
    got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
    spl = got.spl.tolist()
    assert spl == sorted(spl) and spl[0] == 1 and spl[-1] == n + 1 and len(spl) == K + 1
    value = cp.total_value(A, got, mdl, backend=hip)
    assert cst[n, K - 1] == value
    assert value <= cp.total_value(A, cp.partition_stripe(A, K, cp.EquiSplitter(), backend=hip), mdl, backend=hip)
    if isinstance(mdl, MSC):
        assert value <= cp.total_value(A, cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(mdl), backend=hip), mdl, backend=hip)
    rc4, _, cst4 = hip.dynamic_tables(A, 4, SUM, mdl.marshal(), None)       # alpha = 0: more parts never cost more
    assert rc4 == 0 and value <= cst4[n, 3]
    # optimality, from the definition: sampled Bellman cells of the six full layers and the last row, and the closed form of every cell
    counts, _ = audit_tables(A, mdl, K, ptr, cst, 250, 8)
    print("audited", counts)
    assert spl == unravel(ptr, K)


def test_through_the_public_callers(hip):
    A = golden_matrices()["HB/can_292"]
    edge_cut = SEC(0, 0, 0, 1)
    for K in (4, 9):
        for prt in (cp.SymmetricPartitioner(cp.DynamicTotalSplitter(edge_cut)),
                    cp.PermutingPartitioner(cp.CuthillMcKeePermuter(), cp.SymmetricPartitioner(cp.DynamicTotalSplitter(edge_cut)))):
            with options(hip, sym_total_min_n=0):
                with watched(hip) as seen:
                    got = cp.partition_plaid(A, K, prt, backend=hip)
            assert seen["layers"] == K - 1 and seen["brute"] == 0, seen
            with options(hip, force_brute=1):
                want = cp.partition_plaid(A, K, prt, backend=hip)
            assert all(a == b for a, b in zip(got, want))
