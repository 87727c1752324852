"""The split of the link entries by bit plane (tests/own_split_model.py, the specification of cp_test_own_split) and the count
identity the own tiles of the total-cost DP rely on: for every plane b >= 8, every row r with bit b set and every column range
[a, B) inside the row's Fenwick block, the prefix-sum difference plus the plane's variable entries with next >= r is the direct
count of the entries with next >= r."""
import numpy as np
import pytest

import own_split_model as osm
from util import cp, suitesparse_shaped, banded

MATS = [("shaped513", lambda: suitesparse_shaped(513, 6, 11)), ("shaped1024", lambda: suitesparse_shaped(1024, 6, 12)),
        ("shaped1025", lambda: suitesparse_shaped(1025, 5, 7)), ("shaped3000", lambda: suitesparse_shaped(3000, 8, 1)),
        ("banded2500", lambda: banded(2500, 6, 0.5, 3))]


@pytest.mark.parametrize("name,make", MATS)
def test_split_arrays_are_a_partition_of_the_entries(name, make):
    A = make()
    n = A.n
    nb, vpos, vsa, vnext = osm.split(A)
    assert nb == osm.nbits_of(n) - osm.BMIN and nb >= 1
    cols, nxt = osm.next_links(A)
    h = osm.top_bit(cols ^ nxt)
    assert np.all(nxt > cols) and np.all(h < osm.nbits_of(n))              # (rows are deduplicated: a later column, or n)
    # every entry is variable in exactly one plane; the stored planes hold those of the planes >= BMIN
    assert vnext.size == int(np.sum(h >= osm.BMIN))
    for i in range(nb):
        assert vpos[i, 0] == (0 if i == 0 else osm.plane_end(vpos, vnext, i - 1))
        assert np.all(np.diff(vpos[i]) >= 0) and vpos[i, n] == osm.plane_end(vpos, vnext, i)
        assert vsa[i, 0] == 0 and np.all(np.diff(vsa[i]) >= 0) and vsa[i, n] == int(np.sum(h > osm.BMIN + i))


@pytest.mark.parametrize("name,make", MATS)
def test_count_identity_every_plane(name, make):
    A = make()
    n = A.n
    S = osm.split(A)
    cols, nxt = osm.next_links(A)
    rng = np.random.default_rng(17)
    checked = 0
    for b in range(osm.BMIN, osm.nbits_of(n)):
        rows = np.arange(1, n + 1)
        rows = rows[(rows >> b) & 1 == 1]
        assert rows.size > 0
        picks = list(rng.choice(rows, size=min(40, rows.size), replace=False)) + [int(rows[0]), int(rows[-1])]
        for r in picks:
            r = int(r)
            rb = (r >> b) << b
            lo, hi = rb - (1 << b), rb                                       # the block; columns [a, B) inside it
            for _ in range(4):
                a, B = sorted(int(x) for x in rng.integers(lo, hi + 1, 2))
                assert osm.split_count(S, b, a, B, r) == osm.direct_count(A, cols, nxt, a, B, r), (name, b, r, a, B)
                checked += 1
            assert osm.split_count(S, b, lo, hi, r) == osm.direct_count(A, cols, nxt, lo, hi, r)
    assert checked >= 4 * 3 * (osm.nbits_of(n) - osm.BMIN)


def test_no_stored_plane_below_256_columns():
    A = suitesparse_shaped(200, 4, 3)
    nb, vpos, vsa, vnext = osm.split(A)
    assert nb == 0 and vnext.size == 0
