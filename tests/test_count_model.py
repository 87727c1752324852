"""tests/count_model.py against the per-pair definitions of tests/util.py and against dense double cumulative sums, so the model
is pinned before tests/test_gpu_count_edges.py lets it judge a kernel."""
import math
from fractions import Fraction

import numpy as np

import count_model as cm
from test_gpu_counts import DIMS
from util import sprand, dense_mask, ref_dominancecount, ref_netcount, ref_selfnetcount


def _grid():
    rng = np.random.default_rng(0xC0FFEE)
    return [sprand(m, n, p, rng) for m in DIMS for n in DIMS for p in (0.5, 0.15)]


def test_dom_tables_equal_the_per_pair_definition():
    rng = np.random.default_rng(5)
    for A in _grid():
        D = dense_mask(A)
        val = rng.integers(-2 ** 62, 2 ** 62, A.nnz)
        Cn, P = cm.dom_tables(A, val)
        W = np.zeros((A.m, A.n), dtype=np.int64)
        W[A.rowval - 1, np.repeat(np.arange(A.n), np.diff(A.colptr))] = val
        assert Cn.shape == P.shape == (A.m + 1, A.n + 1) and P.dtype == np.int64
        for i in range(1, A.m + 2):
            for j in range(1, A.n + 2):
                assert Cn[i - 1, j - 1] == ref_dominancecount(D, i, j)
                assert int(P[i - 1, j - 1]) == (int(sum(int(v) for v in W[:i - 1, :j - 1].ravel())) + 2 ** 63) % 2 ** 64 - 2 ** 63
        assert cm.dom_tables(A)[1] is None and np.array_equal(cm.dom_tables(A)[0], Cn)


def test_dom_tables_wrap_unsigned_words():
    rng = np.random.default_rng(6)
    A = sprand(9, 8, 0.6, rng)
    val = rng.integers(0, 2 ** 63, A.nnz, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    _, P = cm.dom_tables(A, val)
    assert P.dtype == np.uint64
    W = np.zeros((9, 8), dtype=object)
    W[A.rowval - 1, np.repeat(np.arange(8), np.diff(A.colptr))] = [int(v) for v in val]
    for i in range(1, 11):
        for j in range(1, 10):
            assert int(P[i - 1, j - 1]) == int(W[:i - 1, :j - 1].sum()) % 2 ** 64
    assert int(W.sum()) >= 2 ** 64                       # the sums do wrap


def test_net_tables_equal_the_per_pair_definitions():
    for A in _grid():
        D = dense_mask(A)
        net, snet = cm.net_tables(A)
        assert net.shape == snet.shape == (A.n + 1, A.n + 1)
        for j in range(1, A.n + 2):
            for jp in range(j, A.n + 2):
                assert net[j - 1, jp - 1] == ref_netcount(D, j, jp)
                assert snet[j - 1, jp - 1] == ref_selfnetcount(D, j, jp)


def test_net_pairs_in_blocks_equal_the_tables():
    rng = np.random.default_rng(7)
    A = sprand(37, 29, 0.1, rng)
    net, snet = cm.net_tables(A)
    j = rng.integers(1, 31, 500); jp = rng.integers(1, 31, 500)
    j, jp = np.minimum(j, jp), np.maximum(j, jp)
    got = cm.net_pairs(dense_mask(A), j, jp, chunk=37 * 7)      # 7 pairs per block
    assert np.array_equal(got[0], net[j - 1, jp - 1]) and np.array_equal(got[1], snet[j - 1, jp - 1])


def _dense_rook(N, idx, val, dtype):
    B = np.zeros((N, N), dtype=dtype)
    B[idx - 1, np.arange(N)] = val
    P = np.zeros((N + 1, N + 1), dtype=dtype)
    with np.errstate(over="ignore"):
        P[1:, 1:] = np.cumsum(np.cumsum(B, axis=0, dtype=dtype), axis=1, dtype=dtype)
    return P


def test_rook_queries_equal_a_dense_double_cumsum():
    rng = np.random.default_rng(8)
    for N in list(range(1, 17)) + [31, 32, 33, 63, 64, 65]:
        for idx in (rng.permutation(N) + 1, np.arange(1, N + 1), np.arange(N, 0, -1)):
            val = rng.integers(0, 2 ** 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            ii, jj = (x.ravel() for x in np.meshgrid(np.arange(1, N + 2), np.arange(1, N + 2), indexing="ij"))
            for block in (cm.ROOK_BLOCK, 16, 5):         # one band, and bands that end inside the pattern
                cnt, sm = cm.rook_queries(N, idx, val, ii, jj, block=block)
                assert np.array_equal(cnt, _dense_rook(N, idx, 1, np.int64)[ii - 1, jj - 1])
                assert sm.dtype == np.uint64 and np.array_equal(sm, _dense_rook(N, idx, val, np.uint64)[ii - 1, jj - 1])
            sval = val.view(np.int64)
            assert np.array_equal(cm.rook_queries(N, idx, sval, ii, jj)[1], _dense_rook(N, idx, sval, np.int64)[ii - 1, jj - 1])
            assert cm.rook_queries(N, idx, None, ii, jj)[1] is None


def test_rook_queries_across_bands_at_full_band_size():
    rng = np.random.default_rng(9)
    N = 1030                                              # two bands of ROOK_BLOCK rows
    idx = rng.permutation(N) + 1
    val = rng.integers(-2 ** 62, 2 ** 62, N)
    i = np.concatenate([rng.integers(1, N + 2, 4000), [1, N + 1, cm.ROOK_BLOCK, cm.ROOK_BLOCK + 1, cm.ROOK_BLOCK + 2]])
    j = np.concatenate([rng.integers(1, N + 2, 4000), [N + 1, N + 1, N + 1, N + 1, N + 1]])
    cnt, sm = cm.rook_queries(N, idx, val, i, j)
    assert np.array_equal(cnt, _dense_rook(N, idx, 1, np.int64)[i - 1, j - 1])
    assert np.array_equal(sm, _dense_rook(N, idx, val, np.int64)[i - 1, j - 1])


def test_exact_sums_are_exact():
    """the limb sums against math.fsum (correctly rounded) and against rational arithmetic on a small pattern"""
    rng = np.random.default_rng(10)
    A = sprand(23, 19, 0.4, rng)
    val = rng.standard_normal(A.nnz) * 10.0 ** rng.integers(-6, 7, A.nnz)
    val[:3] = [0.0, 5e-324, -1.7976931348623157e308]     # zero, the smallest subnormal, the largest magnitude
    assert all(Fraction(float(v)) == f for v, f in zip(val, cm.exact(val)))
    ii, jj = (x.ravel() for x in np.meshgrid(np.arange(1, 25), np.arange(1, 21), indexing="ij"))
    ref, S = cm.dom_sum_exact(A, val, ii, jj)
    W = np.zeros((23, 19), dtype=object)
    W[:] = Fraction(0)
    W[A.rowval - 1, np.repeat(np.arange(19), np.diff(A.colptr))] = [Fraction(float(v)) for v in val]
    assert S == sum(abs(Fraction(float(v))) for v in val)
    for t in range(ii.size):
        assert ref[t] == sum(W[:ii[t] - 1, :jj[t] - 1].ravel(), Fraction(0))
    val = val[3:3 + 23]
    idx = rng.permutation(23) + 1
    ref, S = cm.rook_sum_exact(23, idx, val, ii[ii <= 24], np.minimum(jj[ii <= 24], 24))
    for t in range(0, ref.size, 7):
        i, j = ii[t], min(jj[t], 24)
        sel = [float(val[c]) for c in range(23) if c + 1 < j and idx[c] < i]
        assert float(ref[t]) == math.fsum(sel)
    assert float(S) == math.fsum(abs(float(v)) for v in val)
