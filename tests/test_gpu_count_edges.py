"""GPU tests of the counting layer under the partitioners -- the wavelet counters of csrc/wavelet.hip and the dianet / selfpin
builders of csrc/sym.hip -- against tests/count_model.py and tests/sym_model.py, at the sizes where these kernels change path:

  * the weighted prefix scan (k_wsum_reduce / k_wsum_blocks / k_wsum_apply) works in blocks of 2048 over Nk + 1 outputs, so
    Nk = 2047, 2048, 2049, 4095, 4096, 4097, 6145 gives 1 .. 4 blocks with the tail before, on and after a block edge;
  * k_wt_bits / k_wt_scatter handle 2048 keys per block, eight 64-key words per wave: Nk = 63, 64, 65, 2047, 2048, 2049, 4096, 4097
    (at Nk % 64 == 0 the rank of position Nk reads the extra word W - 1);
  * the net-type counters have H = cllog2(n + 2) levels: at n = 2^H - 2 the top key n + 1 is 2^H - 1, the last key of the last
    bucket of every level; dominancecount has H = cllog2(m + 1), the same edge at m = 2^H - 1;
  * one key shared by every entry (a dense row), every key distinct (a dense column), and the per-wave count of the hot key n + 1 of
    the dianet build at n = 2049.

Integer sums are equal to the model; Float64 sums are bit-equal where every partial sum is representable, and within a bound derived
from the kernels' addition chains (float64_bound) where it is not."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import count_model as cm
import greedy_model as gm
from test_gpu_symmetric import pattern, tables
from util import cp

pytestmark = pytest.mark.gpu
M = cp.models

SCAN_NK = [2047, 2048, 2049, 4095, 4096, 4097, 6145]
SCAN_SHAPE = {2047: (200, 300), 2048: (255, 301), 2049: (256, 299), 4095: (300, 300), 4096: (255, 307), 4097: (257, 293), 6145: (263, 311)}
ROOK_N = [2047, 2048, 2049, 4097]
WORD_NK = [63, 64, 65, 2047, 2048, 2049, 4096, 4097]
LEVEL_N = [6, 14, 30, 62, 126, 254]
LEVEL_M = [15, 31, 63, 127, 255]


# ---------------------------------------------------------------- patterns with an exact entry count
def exact_pattern(m, n, Nk, seed, rows=None):
    """m x n pattern with exactly Nk entries: columns 0, n - 1 and every ninth one empty, one column of 97 entries where there is
    room, the other lengths uneven.  rows: the entries lie in these rows only and every one of them is used (needs Nk >= len(rows))."""
    rng = np.random.default_rng(seed)
    R = np.arange(m) if rows is None else np.asarray(rows)
    free = np.array([c for c in range(n) if c not in (0, n - 1) and c % 9 != 4])
    lens = np.zeros(n, dtype=np.int64)
    if Nk >= 400 and R.size >= 97:
        lens[free[free.size // 3]] = 97
        free = np.delete(free, free.size // 3)
    base, extra = divmod(Nk - int(lens.sum()), free.size)
    lens[free] = base
    lens[rng.choice(free, extra, replace=False)] += 1
    for a, b in rng.choice(free, (200, 2)):              # uneven lengths, the total unchanged
        d = min(int(lens[a]), R.size - int(lens[b]), int(rng.integers(0, 4))) if a != b else 0
        lens[a] -= d; lens[b] += d
    assert lens.sum() == Nk and lens.max() <= R.size
    must = rng.permutation(R) if rows is not None else R[:0]
    cols = []
    for c in range(n):
        k = min(int(lens[c]), must.size)
        take, must = must[:k], must[k:]
        rest = rng.choice(np.setdiff1d(R, take), int(lens[c]) - k, replace=False)
        cols.append(np.sort(np.concatenate([take, rest])))
    assert must.size == 0
    A = gm.from_columns(m, cols)
    assert A.nnz == Nk and (A.m, A.n) == (m, n)
    return A


@functools.lru_cache(maxsize=None)
def scan_pattern(Nk):
    m, n = SCAN_SHAPE[Nk]
    A = exact_pattern(m, n, Nk, 7000 + Nk)
    lens = np.diff(A.colptr)
    assert lens.max() > 64 and (lens == 0).sum() >= 3
    return A


@functools.lru_cache(maxsize=None)
def rook_perms(N):
    return {"seeded": np.random.default_rng(9000 + N).permutation(N) + 1, "identity": np.arange(1, N + 1, dtype=np.int64),
            "reversal": np.arange(N, 0, -1, dtype=np.int64)}


def wrap_weights(rng, k):
    """UInt words with the top bit in use: the sums wrap"""
    return rng.integers(0, 2 ** 63, k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, k).astype(np.uint64)


def signed_weights(rng, k):
    return rng.integers(-2 ** 63, 2 ** 63 - 1, k)


def dyadic_weights(rng, k):
    """integer multiples of 2^-10 below 2^20 in magnitude, mixed signs: a sum of at most 2^13 of them is below 2^33 and a multiple
    of 2^-10, 43 significant bits, so every partial sum in any order is exact in binary64"""
    return rng.integers(-2 ** 30 + 1, 2 ** 30, k) / 1024.0


def general_weights(rng, k):
    return rng.standard_normal(k) * 10.0 ** rng.integers(-6, 7, k)


def grid(m, n):
    ii, jj = np.meshgrid(np.arange(1, m + 2), np.arange(1, n + 2), indexing="ij")
    return ii.ravel().astype(np.int64), jj.ravel().astype(np.int64)


def domsum(hip, A, val, i, j, unsigned=False):
    h, dt = hip.domsum_build(A, val)
    try:
        return hip.wsum_query(h, dt, i, j, unsigned=unsigned)
    finally:
        hip.wsum_free(h)


def rooks(hip, N, idx, val, i, j, unsigned=False):
    h, dt = hip.rook_build(N, idx, val)
    try:
        return hip.wsum_query(h, dt, i, j, unsigned=unsigned)
    finally:
        hip.wsum_free(h)


@functools.lru_cache(maxsize=None)
def rook_grid(N):
    """20 000 seeded queries, every query with i or j in {1, 2, N, N + 1} and every query with j in {2048, 2049, 2050}"""
    rng = np.random.default_rng(100 + N)
    i, j = [rng.integers(1, N + 2, 20000)], [rng.integers(1, N + 2, 20000)]
    every = np.arange(1, N + 2)
    for e in (1, 2, N, N + 1):
        i += [np.full(N + 1, e), every]; j += [every, np.full(N + 1, e)]
    for e in (2048, 2049, 2050):
        if e <= N + 1:
            i.append(every); j.append(np.full(N + 1, e))
    return np.concatenate(i).astype(np.int64), np.concatenate(j).astype(np.int64)


# ---------------------------------------------------------------- a. weighted sums across scan blocks
@pytest.mark.parametrize("Nk", SCAN_NK)
def test_domsum_across_scan_blocks(hip, Nk):
    A = scan_pattern(Nk)
    rng = np.random.default_rng(Nk)
    i, j = grid(A.m, A.n)
    for val, unsigned in ((wrap_weights(rng, Nk), True), (signed_weights(rng, Nk), False)):
        Cn, P = cm.dom_tables(A, val)
        cnt, sm = domsum(hip, A, val, i, j, unsigned=unsigned)
        assert np.array_equal(cnt, Cn[i - 1, j - 1])
        assert sm.dtype == P.dtype and np.array_equal(sm, P[i - 1, j - 1])


@pytest.mark.parametrize("N", ROOK_N)
def test_rooks_across_scan_blocks(hip, N):
    rng = np.random.default_rng(N)
    i, j = rook_grid(N)
    for name, idx in rook_perms(N).items():
        val = wrap_weights(rng, N) if name != "reversal" else signed_weights(rng, N)
        wc, ws = cm.rook_queries(N, idx, val, i, j)
        cnt, sm = rooks(hip, N, idx, val, i, j, unsigned=val.dtype == np.uint64)
        assert np.array_equal(cnt, wc), name
        assert sm.dtype == ws.dtype and np.array_equal(sm, ws), name
        cnt, sm = rooks(hip, N, idx, None, i, j)
        assert np.array_equal(cnt, wc) and not sm.any(), name


# ---------------------------------------------------------------- b. Float64, exactly
@pytest.mark.parametrize("Nk", SCAN_NK)
def test_domsum_float64_exact(hip, Nk):
    A = scan_pattern(Nk)
    val = dyadic_weights(np.random.default_rng(2 * Nk), Nk)
    assert (val < 0).any() and (val > 0).any()
    i, j = grid(A.m, A.n)
    Cn, P = cm.dom_tables(A, val)
    cnt, sm = domsum(hip, A, val, i, j)
    assert np.array_equal(cnt, Cn[i - 1, j - 1])
    assert sm.dtype == np.float64 and sm.tobytes() == P[i - 1, j - 1].tobytes()


@pytest.mark.parametrize("N", ROOK_N)
def test_rooks_float64_exact(hip, N):
    rng = np.random.default_rng(2 * N)
    i, j = rook_grid(N)
    for name, idx in rook_perms(N).items():
        val = dyadic_weights(rng, N)
        wc, ws = cm.rook_queries(N, idx, val, i, j)
        cnt, sm = rooks(hip, N, idx, val, i, j)
        assert np.array_equal(cnt, wc), name
        assert sm.dtype == np.float64 and sm.tobytes() == ws.tobytes(), name


# ---------------------------------------------------------------- c. Float64, general
def float64_bound(Nk, H, S):
    """The largest error a Float64 query can have, from the kernels of csrc/wavelet.hip.  u = 2^-53, S = sum(|w|) over the structure.

    A stored prefix value (an element of a Z plane or of P0) is a sum of weights, some of them masked to 0, evaluated by wsum_scan
    over nb = ceil((Nk + 1) / 2048) blocks.  A sum evaluated by any tree of additions in which no term passes through more than D
    additions differs from the exact sum by at most gamma(D) * sum(|terms|) <= gamma(D) * S, gamma(D) = D u / (1 - D u).  The longest
    path of a term into an output of the last block (nb >= 2):
        k_wsum_reduce   7   the thread's 8 terms in sequence (the first one is added to 0: no rounding)
                        8   the 256-lane tree, 128 -> 1
        k_wsum_blocks   nb - 2   block 0's sum is carried to block nb - 1 through nb - 1 additions, the first of them to 0
        k_wsum_apply    1   bsum[block] + (the lanes before this one)
                        7   the up to 7 terms of the same thread in front of the output
    so D = nb + 21.  (A term of the same block takes 7 + 8 through the thread sum and the 8 scan steps, + 1 + 7 as above: 23 <= D.)

    wt_sum_le combines 2 (H + 1) such values a_k (errors <= E = gamma(D) S, true magnitudes <= S) by H + 1 subtractions
    Z[q2] - Z[q1], P0[..] - P0[..] and the chain sum_out += difference, whose first addition is to 0: 2 H + 1 further operations,
    of which no a_k passes through more than H + 1 (its subtraction and the at most H additions after it).  Hence
        |result - exact| <= 2 (H + 1) E  +  gamma(H + 1) * 2 (H + 1) * (S + E).
    Returned as a Fraction, with D."""
    u = Fraction(1, 2 ** 53)
    nb = -(-(Nk + 1) // 2048)
    assert nb >= 2
    D = nb + 21
    E = D * u * S / (1 - D * u)
    g = (H + 1) * u / (1 - (H + 1) * u)
    return 2 * (H + 1) * E + g * 2 * (H + 1) * (S + E), D


def cllog2(x):
    return int(x - 1).bit_length()


def _check_bound(what, got, ref, S, Nk, H):
    bound, D = float64_bound(Nk, H, S)
    err = np.abs(cm.exact(got) - ref)
    worst = max(err)
    print(f"{what}: Nk = {Nk}, H = {H}, D = {D}, sum|w| = {float(S):.6g}, bound = {float(bound):.6g}, "
          f"largest error = {float(worst):.6g}, error / bound = {float(worst / bound):.6g}")
    assert worst > 0                                     # (these weights do round: an all-exact run would mean the wrong weights)
    assert worst <= bound


def test_domsum_float64_general_within_the_derived_bound(hip):
    A = scan_pattern(6145)
    val = general_weights(np.random.default_rng(61450), 6145)
    i, j = grid(A.m, A.n)
    ref, S = cm.dom_sum_exact(A, val, i, j)
    cnt, sm = domsum(hip, A, val, i, j)
    assert np.array_equal(cnt, cm.dom_tables(A)[0][i - 1, j - 1])
    _check_bound("domsum", sm, ref, S, 6145, cllog2(A.m + 1))


def test_rooks_float64_general_within_the_derived_bound(hip):
    N = 4097
    idx = rook_perms(N)["seeded"]
    val = general_weights(np.random.default_rng(40970), N)
    i, j = rook_grid(N)
    ref, S = cm.rook_sum_exact(N, idx, val, i, j)
    cnt, sm = rooks(hip, N, idx, val, i, j)
    assert np.array_equal(cnt, cm.rook_queries(N, idx, None, i, j)[0])
    _check_bound("rooks", sm, ref, S, N, cllog2(N + 1))


# ---------------------------------------------------------------- d. degenerate weighted structures
def _degenerate():
    e = np.zeros(0, dtype=np.int64)
    return {"m=0": lambda: cp.SparseMatrixCSC(0, 5, np.ones(6, dtype=np.int64), e),
            "n=0": lambda: cp.SparseMatrixCSC(7, 0, np.ones(1, dtype=np.int64), e),
            "nnz=0": lambda: cp.SparseMatrixCSC(6, 9, np.ones(10, dtype=np.int64), e),
            "dense row": lambda: gm.from_columns(5, [np.array([3])] * 2049),
            "dense column": lambda: gm.from_columns(2049, [e, np.arange(2049), e]),
            "Nk=64": lambda: exact_pattern(20, 30, 64, 64),
            "Nk=128": lambda: exact_pattern(20, 30, 128, 128)}


@pytest.mark.parametrize("case", list(_degenerate()))
def test_degenerate_weighted_structures(hip, case):
    A = _degenerate()[case]()
    rng = np.random.default_rng(len(case))
    i, j = grid(A.m, A.n)
    corners = {(1, 1), (1, A.n + 1), (A.m + 1, 1), (A.m + 1, A.n + 1)}
    assert corners <= set(zip(i.tolist(), j.tolist()))
    for val, unsigned in ((wrap_weights(rng, A.nnz), True), (signed_weights(rng, A.nnz), False), (dyadic_weights(rng, A.nnz), False)):
        Cn, P = cm.dom_tables(A, val)
        cnt, sm = domsum(hip, A, val, i, j, unsigned=unsigned)
        assert np.array_equal(cnt, Cn[i - 1, j - 1])
        assert sm.dtype == P.dtype and sm.tobytes() == P[i - 1, j - 1].tobytes()
    if A.nnz:
        assert Cn[A.m, A.n] == A.nnz


# ---------------------------------------------------------------- e. query preconditions are status returns
def test_wsum_query_preconditions_are_status_returns(hip):
    A = exact_pattern(20, 30, 128, 128)
    val = signed_weights(np.random.default_rng(1), 128)
    _, P = cm.dom_tables(A, val)
    N = 33
    idx = np.random.default_rng(2).permutation(N) + 1
    rval = signed_weights(np.random.default_rng(3), N)
    for build, m, n, want in ((lambda: hip.domsum_build(A, val), A.m, A.n, lambda i, j: P[i - 1, j - 1]),
                              (lambda: hip.rook_build(N, idx, rval), N, N, lambda i, j: cm.rook_queries(N, idx, rval, i, j)[1])):
        h, dt = build()
        try:
            for bi, bj in ((0, 1), (m + 2, 1), (1, 0), (1, n + 2), (-1, n + 1), (m + 1, n + 2)):
                i = np.array([1, bi, m + 1], dtype=np.int64); j = np.array([1, bj, n + 1], dtype=np.int64)
                cnt = np.zeros(3, dtype=np.int64); sm = np.zeros(3, dtype=np.int64)
                assert hip.lib.cp_wsum_query(h, 3, i, j, cnt, sm, None) == M.CP_EINVAL, (bi, bj)
                i, j = grid(m, n)                         # the handle answers a sound query afterwards
                assert np.array_equal(hip.wsum_query(h, dt, i, j)[1], want(i, j))
        finally:
            hip.wsum_free(h)


# ---------------------------------------------------------------- f. unweighted counters at block and word edges
def column_pairs(n, seed):
    """all pairs j <= j' when n <= 130; otherwise 20 000 seeded pairs and every pair with j or j' in {1, 2, n, n + 1}"""
    every = np.arange(1, n + 2)
    if n <= 130:
        a, b = np.meshgrid(every, every, indexing="ij")
    else:
        rng = np.random.default_rng(seed)
        a, b = [rng.integers(1, n + 2, 20000)], [rng.integers(1, n + 2, 20000)]
        for e in (1, 2, n, n + 1):
            a += [np.full(n + 1, e), every]; b += [every, np.full(n + 1, e)]
        a, b = np.concatenate(a), np.concatenate(b)
    return np.minimum(a, b).ravel().astype(np.int64), np.maximum(a, b).ravel().astype(np.int64)


def check_counters(hip, A, seed):
    i, j = grid(A.m, A.n)
    assert np.array_equal(cp.dominancecount(A, backend=hip)(i, j), cm.dom_tables(A)[0][i - 1, j - 1])
    net, snet = cm.net_tables(A)
    j, jp = column_pairs(A.n, seed)
    assert np.array_equal(cp.netcount(A, backend=hip)(j, jp), net[j - 1, jp - 1])
    assert np.array_equal(cp.selfnetcount(A, backend=hip)(j, jp), snet[j - 1, jp - 1])


@pytest.mark.parametrize("Nk", WORD_NK)
def test_unweighted_counters_at_block_and_word_edges(hip, Nk):
    m, n = (40, 130) if Nk <= 65 else (120, 260)
    check_counters(hip, exact_pattern(m, n, Nk, 3000 + Nk), Nk)


@pytest.mark.parametrize("R", [64, 2048, 2049])
def test_selfnetcount_key_count_at_block_and_word_edges(hip, R):
    """the self-net counter has one key per non-empty row"""
    m, n, Nk = (120, 130, 300) if R == 64 else (2100, 260, 3000)
    rows = np.sort(np.random.default_rng(R).choice(m, R, replace=False))
    A = exact_pattern(m, n, Nk, 5000 + R, rows=rows)
    assert np.unique(A.rowval).size == R
    check_counters(hip, A, R)


# ---------------------------------------------------------------- g. level edges
@pytest.mark.parametrize("n0", LEVEL_N)
def test_net_type_counters_at_level_edges(hip, n0):
    """n0 = 2^H - 2: the top key n + 1 is the last key 2^H - 1; n0 + 1 adds a level, n0 - 1 does not"""
    assert n0 + 2 == 1 << cllog2(n0 + 2) and cllog2(n0 + 3) == cllog2(n0 + 2) + 1 and cllog2(n0 + 1) == cllog2(n0 + 2)
    for n in (n0 - 1, n0, n0 + 1):
        a, b = np.meshgrid(np.arange(1, n + 2), np.arange(1, n + 2), indexing="ij")
        j, jp = a[a <= b].astype(np.int64), b[a <= b].astype(np.int64)
        for v in ("partial", "dense"):
            A, T = pattern(n, v), tables(n, v)
            net, snet = cm.net_tables(A)
            assert np.array_equal(cp.netcount(A, backend=hip)(j, jp), net[j - 1, jp - 1]), (n, v)
            assert np.array_equal(cp.selfnetcount(A, backend=hip)(j, jp), snet[j - 1, jp - 1]), (n, v)
            assert np.array_equal(cp.dianetcount(A, backend=hip)(j, jp), T.get("dianet")[j - 1, jp - 1]), (n, v)
            assert np.array_equal(cp.selfpincount(A, backend=hip)(j, jp), T.get("selfpin")[j - 1, jp - 1]), (n, v)


@pytest.mark.parametrize("m0", LEVEL_M)
def test_dominancecount_at_level_edges(hip, m0):
    """m0 = 2^H - 1: the top key m is the last key 2^H - 1"""
    assert m0 + 1 == 1 << cllog2(m0 + 1)
    rng = np.random.default_rng(m0)
    for m in (m0 - 1, m0, m0 + 1):
        cols = [np.nonzero(rng.random(m) < 0.4)[0] for _ in range(9)]
        cols[4] = np.arange(m)                            # every key, the top one included
        cols[7] = np.array([m - 1])
        A = gm.from_columns(m, cols)
        i, j = grid(m, 9)
        assert np.array_equal(cp.dominancecount(A, backend=hip)(i, j), cm.dom_tables(A)[0][i - 1, j - 1]), m


# ---------------------------------------------------------------- h. the hot key above toy size
@pytest.mark.parametrize("rem", [1, 0])
def test_dianet_hot_key_above_toy_size(hip, rem):
    """n = 2049 with an empty diagonal, so D = A + I has Nd = nnz + n entries, Nd % 64 == rem.  The entries of A lie in the columns
    c with c % 256 >= 128, nearly all above the diagonal: a row's first occurrence is then its own diagonal entry, whose key is the
    hot key n + 1.  Every run of 128 columns without entries of A is 128 hot keys in a row (whole waves of them at any alignment),
    and the last entry of D, the diagonal of the last column, is hot: it ends a one-lane wave (rem 1) or a full one (rem 0).

    Reference: the definition |rows(A[:, j:j'-1]) united with {j .. j'-1}| computed directly from the dense mask of A + I
    (count_model.net_pairs) on 5 000 seeded pairs and the pairs with j or j' in {1, n + 1}; sym_model.Tables needs about 14 s for
    the table at this n, which is no test-sized reference."""
    n = 2049
    nnz = 1984 if rem == 1 else 1983
    assert (nnz + n) % 64 == rem
    rng = np.random.default_rng(20490 + rem)
    elig = np.array([c for c in range(n) if c % 256 >= 128])
    c = rng.choice(elig, 3 * nnz)
    r = (rng.random(3 * nnz) * c).astype(np.int64)       # row < column: above the diagonal
    low = rng.choice(elig[elig < n - 10], 40)
    c = np.concatenate([low, c]); r = np.concatenate([rng.integers(low + 1, n - 1), r])      # 40 below it, none in the last row
    _, first = np.unique(r * n + c, return_index=True)
    keep = np.sort(first)[:nnz]
    c, r = c[keep], r[keep]
    assert keep.size == nnz and not (c == r).any() and (r > c).sum() >= 30
    A = gm.from_columns(n, [np.sort(r[c == k]) for k in range(n)])
    assert A.nnz == nnz
    mask = np.eye(n, dtype=bool)
    mask[r, c] = True
    assert mask.sum() == nnz + n
    j = rng.integers(1, n + 2, 5000); jp = rng.integers(1, n + 2, 5000)
    every = np.arange(1, n + 2)
    j = np.concatenate([j, np.full(n + 1, 1), every]); jp = np.concatenate([jp, every, np.full(n + 1, n + 1)])
    j, jp = np.minimum(j, jp).astype(np.int64), np.maximum(j, jp).astype(np.int64)
    want = cm.net_pairs(mask, j, jp)[0]
    assert want[5000 + n] == n                            # the pair (1, n + 1)
    assert np.array_equal(cp.dianetcount(A, backend=hip)(j, jp), want)
