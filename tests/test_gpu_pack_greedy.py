"""pack_stripe(A, StrictChunker(w_max) | OverlapChunker(rho, w_max)) and pack_plaid over them on the device (csrc/chunk_greedy.hip):
split vector, K and n_nets bit for bit against the literal loops of tests/greedy_model.py."""
import functools

import numpy as np
import pytest

from util import cp, golden_matrices, suitesparse_shaped
from greedy_model import strict_chunks, overlap_chunks, copy_columns, from_columns, transpose

gpu = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)      # wave and block edges; n + 1 = 2^r - 1, 2^r, 2^r + 1 doubling rounds
SHAPES = {"short": (12, 0.3), "long": (300, 0.5)}                  # m, density: columns of a few rows / lengths that cross 64 and 128
STRICT_W = (8, 0, 3)
OVERLAP = ((0.9, 8), (0.7, 0), (1.0, 3), (0.5, 100))
FAMILY = [(shape, n) for shape in SHAPES for n in SIZES]


@functools.lru_cache(maxsize=None)
def family_case(shape, n):
    """the pattern and the model's answers, computed once for the tests that share them"""
    m, density = SHAPES[shape]
    A = copy_columns(m, n, density, 7000 + 13 * n + m)
    return A, {w: strict_chunks(A, w) for w in STRICT_W}, {rw: overlap_chunks(A, *rw) for rw in OVERLAP}


def check_strict(hip, A, w_max, want=None):
    want = strict_chunks(A, w_max) if want is None else want
    got = cp.pack_stripe(A, cp.StrictChunker(w_max), backend=hip)
    assert got.K == len(want) - 1 and np.array_equal(got.spl, want), (A, w_max, got.spl[:10], want[:10])


def check_overlap(hip, A, rho, w_max, want=None):
    spl, nn = overlap_chunks(A, rho, w_max) if want is None else want
    ref = [None]
    got = cp.pack_stripe(A, cp.OverlapChunker(rho, w_max), n_nets=ref, backend=hip)
    assert got.K == len(spl) - 1 and np.array_equal(got.spl, spl), (A, rho, w_max, got.spl[:10], spl[:10])
    assert ref[0].dtype == np.int64 and np.array_equal(ref[0], nn), (A, rho, w_max)
    return got


def test_random_families_are_not_degenerate():
    """a condition on the inputs, from the model's own output: in each family at least half the cases have 2 <= K < n"""
    for shape in SHAPES:
        good = total = 0
        for n in SIZES:
            _, strict, overlap = family_case(shape, n)
            for spl in list(strict.values()) + [v[0] for v in overlap.values()]:
                total += 1
                good += 2 <= len(spl) - 1 < n
        assert 2 * good >= total, (shape, good, total)


@gpu
@pytest.mark.parametrize("shape,n", FAMILY)
def test_random_family(hip, shape, n):
    A, strict, overlap = family_case(shape, n)
    for w, want in strict.items():
        check_strict(hip, A, w, want)
    for (rho, w), want in overlap.items():
        got = check_overlap(hip, A, rho, w, want)
        assert cp.pack_stripe(A, cp.OverlapChunker(rho, w), backend=hip) == got          # without n_nets: the same split vector


@gpu
def test_all_columns_empty(hip):
    n = 257
    A = from_columns(5, [np.zeros(0, dtype=np.int64)] * n)
    for w in (8, 0):
        check_strict(hip, A, w)
        for rho in (0.9, 1.0):                                       # 0 < rho * 0 is false: empties merge up to w_max
            got = check_overlap(hip, A, rho, w)
            assert got.K == (33 if w == 8 else 1)


@gpu
def test_all_columns_identical(hip):
    n = 257
    A = from_columns(9, [np.array([1, 4, 6])] * n)
    for w, K in ((0, 1), (1, n), (8, 33), (n, 1), (n + 5, 1)):
        check_strict(hip, A, w)
        got = check_overlap(hip, A, 1.0, w)
        assert got.K == K and cp.pack_stripe(A, cp.StrictChunker(w), backend=hip).K == K


@gpu
def test_long_columns_that_differ_at_either_end(hip):
    base = np.arange(0, 10000, 2)                                    # 5000 rows
    last = base.copy(); last[-1] += 1
    first = base.copy(); first[0] += 1
    A = from_columns(10001, [base, base, base, last, first])
    for w in (0, 2, 8):
        check_strict(hip, A, w)
    assert cp.pack_stripe(A, cp.StrictChunker(0), backend=hip).spl.tolist() == [1, 4, 5, 6]
    for rho, w in ((1.0, 0), (0.9999, 0), (0.9997, 0), (1.0, 2), (0.0, 8)):
        check_overlap(hip, A, rho, w)


@gpu
@pytest.mark.parametrize("name", sorted(golden_matrices()))
def test_golden_matrices_and_adjoints(hip, name):
    A = golden_matrices()[name]
    for B in (A, transpose(A)):
        for w in (1, 2, 4, 8):
            check_strict(hip, B, w)
            for rho in (0.0, 0.7, 0.8, 0.9, 1.0):
                check_overlap(hip, B, rho, w)


@gpu
def test_bench_shaped_and_mid_degree(hip):
    A = suitesparse_shaped(3000, 12, 11)
    B = copy_columns(50, 300, 0.5, 5)                                # mean column of 25 rows: 32 lanes per start
    for M in (A, B):
        for w in (8, 0):
            check_strict(hip, M, w)
        for rho, w in ((0.9, 8), (0.3, 8), (0.3, 0)):
            check_overlap(hip, M, rho, w)


@gpu
def test_scans_span_blocks_and_fifteen_doubling_rounds(hip):
    A = copy_columns(12, 20000, 0.3, 99)
    spl = strict_chunks(A, 8)
    assert 2 <= len(spl) - 1 < A.n
    check_strict(hip, A, 8, spl)
    check_strict(hip, A, 0)
    want = overlap_chunks(A, 0.9, 8)
    assert 2 <= len(want[0]) - 1 < A.n
    check_overlap(hip, A, 0.9, 8, want)
    check_overlap(hip, A, 0.7, 0)


@gpu
def test_float64_threshold(hip):
    """rho * min is evaluated in Float64 as written: 0.28 * 25 = 7.000000000000001 > 7 splits, 0.6 * 25 = 15 merges; integer
    cross-multiplication or Float32 decide one of the two differently"""
    first = np.arange(25)
    for shared, rho, K in ((7, 0.28, 2), (15, 0.6, 1)):
        other = np.concatenate([np.arange(shared), 100 + np.arange(25 - shared)])
        A = from_columns(200, [first, other])
        for w in (0, 8):
            assert check_overlap(hip, A, rho, w).K == K


@gpu
def test_first_column_cardinality_is_never_refreshed(hip):
    """c stays |col(1)| = 1 after the w_max split: the 10-row columns that share one row with their part's start merge at rho = 0.9"""
    cols = [np.array([0])] + [np.concatenate([[0], np.arange(1, 10) + 10 * j]) for j in range(1, 7)]
    A = from_columns(80, cols)
    got = check_overlap(hip, A, 0.9, 2)
    assert got.spl.tolist() == [1, 3, 5, 7, 8]


@gpu
def test_pack_plaid_over_the_greedy_chunkers(hip):
    g = golden_matrices()
    for name in ("HB/west0132", "LPnetlib/lp_blend"):
        A = g[name]
        T = transpose(A)
        D = cp.adjointpattern(A, backend=hip)
        assert np.array_equal(D.colptr, T.colptr) and np.array_equal(D.rowval, T.rowval)
        Pi, Phi = cp.pack_plaid(A, cp.AlternatingPacker(cp.StrictChunker(8), cp.StrictChunker(8)), backend=hip)
        assert np.array_equal(Phi.spl, strict_chunks(A, 8)) and np.array_equal(Pi.spl, strict_chunks(T, 8))
        mtds = (cp.OverlapChunker(0.9, 8), cp.OverlapChunker(0.9, 8))
        Pi, Phi = cp.pack_plaid(A, cp.AlternatingPacker(*mtds), backend=hip)
        assert np.array_equal(Phi.spl, overlap_chunks(A, 0.9, 8)[0]) and np.array_equal(Pi.spl, overlap_chunks(T, 0.9, 8)[0])
        assert cp.pack_plaid(A, cp.AlternatingPacker(*mtds, cp.StrictChunker(2)), adj_A=D, backend=hip)[1].spl.tolist() == strict_chunks(A, 2).tolist()
        if A.m == A.n:
            Pi, Phi = cp.pack_plaid(A, cp.SymmetricPacker(cp.StrictChunker(8), cp.OverlapChunker(0.7, 4), cp.OverlapChunker(0.7, 4)), backend=hip)
            assert Pi == Phi and np.array_equal(Pi.spl, overlap_chunks(T, 0.7, 4)[0])


@gpu
def test_no_columns_is_einval(hip):
    A = cp.SparseMatrixCSC(3, 0, np.ones(1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    spl, K = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    assert hip.pack_strict(A, 8, spl, K) == 1                        # CP_EINVAL
    assert hip.pack_overlap(A, 0.9, 8, spl, K) == 1
    for meth in (cp.StrictChunker(8), cp.OverlapChunker(0.9, 8)):
        with pytest.raises(AssertionError):
            cp.pack_stripe(A, meth, backend=hip)


@gpu
def test_intersection_counter_and_profile_slots(hip):
    n = 257
    A = from_columns(9, [np.array([1, 4, 6])] * n)
    hip.set_option("stat_reset", 1)
    hip.prof_reset(); hip.prof_enable(True)
    try:
        cp.pack_stripe(A, cp.OverlapChunker(1.0, 8), backend=hip)
        cp.pack_stripe(A, cp.StrictChunker(8), backend=hip)
    finally:
        hip.prof_enable(False)
    nx = np.minimum(np.arange(n) + 8, n)                             # every start runs into the width limit or the end: no test fires
    assert hip.get_stat("overlap_isect") == int((nx - np.arange(n) - 1).sum())
    pr = hip.prof_get()
    assert all(pr[k]["launches"] > 0 for k in ("chunk_col_neq", "chunk_overlap_next", "chunk_orbit", "chunk_compact"))
