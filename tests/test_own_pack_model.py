"""The packed form of the split link entries (tests/own_pack_model.py, the specification of cp_test_own_pack): the wide arrays of
tests/own_split_model.py come back from it exactly, the count identity of the own tiles holds on the reconstructed arrays and on the
words as a tile reads them, and the fit test sits where the 16-bit fields end."""
import numpy as np
import pytest

import own_pack_model as opm
import own_split_model as osm
from util import cp, suitesparse_shaped, banded

MATS = [("shaped511", lambda: suitesparse_shaped(511, 6, 31)), ("shaped512", lambda: suitesparse_shaped(512, 6, 32)),
        ("shaped513", lambda: suitesparse_shaped(513, 6, 11)), ("shaped1023", lambda: suitesparse_shaped(1023, 6, 13)),
        ("shaped1025", lambda: suitesparse_shaped(1025, 5, 7)), ("shaped3000", lambda: suitesparse_shaped(3000, 8, 1)),
        ("banded2500", lambda: banded(2500, 6, 0.5, 3))]


@pytest.mark.parametrize("name,make", MATS)
def test_wide_arrays_come_back_and_counts_agree(name, make):
    A = make()
    n = A.n
    S = osm.split(A)
    P = opm.pack(A)
    nb, vpk, vbase, info = P
    assert nb == S[0] and nb >= 1 and info["packed"] == 1 and info["blocks"] == -(-(n + 1) // 256)
    vpos, vsa = opm.unpack(n, vpk, vbase)
    assert np.array_equal(vpos, S[1]) and np.array_equal(vsa, S[2])
    R = (nb, vpos, vsa, S[3])
    cols, nxt = osm.next_links(A)
    rng = np.random.default_rng(23)
    checked = 0
    for b in range(osm.BMIN, osm.nbits_of(n)):
        rows = np.arange(1, n + 1)
        rows = rows[(rows >> b) & 1 == 1]
        for r in [int(x) for x in rng.choice(rows, size=min(30, rows.size), replace=False)] + [int(rows[0]), int(rows[-1])]:
            rb = (r >> b) << b
            lo, hi = rb - (1 << b), rb
            for _ in range(4):
                a, B = sorted(int(x) for x in rng.integers(lo, hi + 1, 2))
                assert osm.split_count(R, b, a, B, r) == osm.direct_count(A, cols, nxt, a, B, r), (name, b, r, a, B)
                # the same range tile by tile, each inside one block, from the words a tile reads
                got, x = 0, a
                while x < B:
                    e = min(B, (x // 256 + 1) * 256)
                    got += opm.packed_count(P, S, b, x, e, r)
                    x = e
                assert got == osm.direct_count(A, cols, nxt, a, B, r), (name, b, r, a, B)
                checked += 1
    assert checked >= 4 * 3 * nb


def test_last_base_entry_is_the_word_behind_the_plane():
    for n in (511, 767, 1023):                                 # n + 1 a multiple of 256
        A = suitesparse_shaped(n, 6, 40 + n)
        nb, vpos, vsa, vnext = osm.split(A)
        _, vpk, vbase, info = opm.pack(A)
        assert (n + 1) % 256 == 0 and info["blocks"] == (n + 1) // 256
        flat = np.concatenate([vpos.reshape(-1), [vnext.size]])
        for i in range(nb):
            assert vbase[i, info["blocks"], 0] == flat[(i + 1) * (n + 1)] and vbase[i, info["blocks"], 1] == 0


def test_sixteen_bit_boundary():
    for c, fits, largest in ((257, 1, 65535), (258, 0, 65790)):
        A = opm.boundary(c)
        assert A.n == 600 and np.all(np.diff(A.colptr)[512:] == 0)
        nb, vpk, vbase, info = opm.pack(A)
        assert nb == 2 and info == {"blocks": 3, "packed": fits, "max_start": largest, "max_prefix": largest}
        if fits:
            S = osm.split(A)
            vpos, vsa = opm.unpack(A.n, vpk, vbase)
            assert np.array_equal(vpos, S[1]) and np.array_equal(vsa, S[2])
