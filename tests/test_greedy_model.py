"""The literal StrictChunker / OverlapChunker loops of tests/greedy_model.py: the reference's own properties
(test_Partitioners.jl:242-245), n_nets against the brute-force distinct-row count, and the two parallel forms the device kernels
implement (csrc/chunk_greedy.hip) -- restated here in numpy -- against the literal loops."""
import numpy as np

from greedy_model import strict_chunks, overlap_chunks, part_nets, copy_columns, from_columns

W_MAXS = (-1, 0, 1, 2, 3, 4, 8, 50)
RHOS = (0.0, 0.5, 0.7, 0.9, 1.0)


def patterns():
    rng = np.random.default_rng(11)
    out = []
    for t in range(60):
        m, n = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        out.append(copy_columns(m, n, float(rng.choice([0.1, 0.5, 0.9])), 1000 + t, 0.5, 0.15))
    out.append(from_columns(5, [np.zeros(0, dtype=np.int64)] * 9))             # all columns empty
    out.append(from_columns(7, [np.array([1, 4, 6])] * 20))                     # all columns identical
    return out


def columns(A):
    return [A.rowval[A.colptr[j] - 1:A.colptr[j + 1] - 1] for j in range(A.n)]


# ---------------------------------------------------------------- the parallel forms (0-based columns; position n is the reference's n + 1)
def strict_closed_form(A, w_max):
    n = A.n
    col = columns(A)
    neq = np.ones(n, dtype=bool)
    for p in range(1, n):
        neq[p] = not np.array_equal(col[p], col[p - 1])
    start = np.maximum.accumulate(np.where(neq, np.arange(n), -1))              # the last flagged position <= p
    flag = neq.copy()
    if w_max >= 1:
        flag |= (np.arange(n) - start) % w_max == 0
    return np.concatenate([np.nonzero(flag)[0] + 1, [n + 1]]).astype(np.int64)


def overlap_next(A, rho, w_max):
    n = A.n
    col = [set(c.tolist()) for c in columns(A)]
    c = len(col[0])
    nxt = np.full(n + 1, n, dtype=np.int64)
    for p in range(n):
        jp = p + 1
        while jp < n:
            if jp - p == w_max or float(len(col[p] & col[jp])) < rho * float(min(c, len(col[jp]))):
                break
            jp += 1
        nxt[p] = jp
    return nxt


def orbit(nxt, n):
    """pointer doubling from column 0 over a double-buffered jump array"""
    mark = np.zeros(n + 1, dtype=bool)
    mark[0] = True
    jump = nxt.copy()
    rounds = 0
    while (1 << rounds) < n + 1:
        rounds += 1
    for _ in range(rounds):
        mark[jump[np.nonzero(mark)[0]]] = True
        jump = jump[jump]                                                         # a new array: every entry reads the old one
    return np.nonzero(mark[:n])[0]


def nets_from_links(A, starts):
    """n_nets[k] = entries of part k whose row's previous column lies before the part's first column"""
    n = A.n
    last = {}
    part = np.searchsorted(starts, np.arange(n), side="right") - 1
    out = np.zeros(len(starts), dtype=np.int64)
    for p, c in enumerate(columns(A)):
        for i in c.tolist():
            if last.get(i, -1) < starts[part[p]]:
                out[part[p]] += 1
            last[i] = p
    return out


def test_reference_properties_and_n_nets():
    for A in patterns():
        n = A.n
        for w_max in W_MAXS:
            cases = [strict_chunks(A, w_max)] + [overlap_chunks(A, rho, w_max)[0] for rho in RHOS]
            for spl in cases:
                assert spl[0] == 1 and spl[-1] == n + 1 and np.all(np.diff(spl) >= 1)
                if w_max >= 1:
                    assert np.all(np.diff(spl) <= w_max)
            for rho in RHOS:
                spl, nn = overlap_chunks(A, rho, w_max)
                assert np.array_equal(nn, part_nets(A, spl)), (n, rho, w_max)


def test_strict_parts_hold_copies_of_their_first_column():
    for A in patterns():
        col = columns(A)
        for w_max in W_MAXS:
            spl = strict_chunks(A, w_max)
            for a, b in zip(spl[:-1], spl[1:]):
                assert all(np.array_equal(col[a - 1], col[j - 1]) for j in range(a, b))
            # greedy: a part ends only at a different column or at the width limit
            for a, b in zip(spl[:-1], spl[1:-1]):
                assert not np.array_equal(col[a - 1], col[b - 1]) or b - a == w_max


def test_closed_form_equals_the_strict_loop():
    for A in patterns():
        for w_max in W_MAXS:
            assert np.array_equal(strict_closed_form(A, w_max), strict_chunks(A, w_max)), (A.n, w_max)


def test_orbit_of_next_equals_the_overlap_loop():
    nontrivial = total = 0
    for A in patterns():
        for w_max in (0, 1, 2, 3, 8, 100):
            for rho in RHOS:
                spl, nn = overlap_chunks(A, rho, w_max)
                starts = orbit(overlap_next(A, rho, w_max), A.n)
                assert np.array_equal(np.concatenate([starts + 1, [A.n + 1]]), spl), (A.n, rho, w_max)
                assert np.array_equal(nets_from_links(A, starts), nn), (A.n, rho, w_max)
                total += 1
                nontrivial += 2 <= len(spl) - 1 < A.n
    assert 2 * nontrivial >= total, (nontrivial, total)


def test_first_column_cardinality_is_never_refreshed():
    """a 1-row first column, then 10-row columns sharing one row with their part's start: with c = 1 they merge at rho = 0.9; a sweep
    that refreshed c at the w_max split would need 9 shared rows and split every column"""
    cols = [np.array([0])] + [np.concatenate([[0], np.arange(1, 10) + 10 * j]) for j in range(1, 7)]
    A = from_columns(80, cols)
    spl, nn = overlap_chunks(A, 0.9, 2)
    assert spl.tolist() == [1, 3, 5, 7, 8]
    assert nn.tolist() == [10, 19, 19, 10]


def test_float64_threshold_cases():
    first = np.arange(25)
    for shared, rho, splits in ((7, 0.28, True), (15, 0.6, False)):
        other = np.concatenate([np.arange(shared), 100 + np.arange(25 - shared)])
        A = from_columns(200, [first, other])
        spl, _ = overlap_chunks(A, rho, 0)
        assert (len(spl) == 3) == splits, (shared, rho, spl)
