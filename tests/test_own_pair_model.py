"""The slots a wave of the paired own-tile stream takes (tests/own_pair_model.py) against the function the kernel calls
(own_pair_slots of csrc/dp_total_own.hip, through the host-only test entry cp_test_own_pair).  No device is needed."""
import ctypes as C

import numpy as np

import own_pair_model as opm
from util import cp


def device_slots(lib, w, nt):
    res = np.zeros(3, np.int64)
    assert lib.cp_test_own_pair(C.c_int64(nt), C.c_int64(w), res.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return bool(res[0]), int(res[1]), int(res[2])


def test_pairing_matches_the_specification():
    from chainpartitioners_jl_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cp_test_own_pair.restype = C.c_int32
    # every order of up to 70 tiles, the sizes around a workgroup of four waves, and orders beyond 2^31 slots
    for nt in list(range(0, 71)) + [255, 256, 257, 2**31 - 1, 2**31, 2**31 + 1, 2**40 + 1]:
        nw = -(-nt // 2)
        waves = range(0, nw + 5) if nt <= 257 else [0, 1, nw - 2, nw - 1, nw, nw + 1]
        seen, lone, full = [], 0, 0
        for w in waves:
            has, s0, s1 = device_slots(lib, w, nt)
            assert (has, s0, s1) == opm.pair_slots(w, nt) or (not has and not opm.pair_slots(w, nt)[0]), (nt, w)
            assert has == (w < nw), (nt, w)
            if has:
                assert 0 <= s0 < nt and 0 <= s1 < nt and s1 in (s0, s0 + 1)        # the partner is clamped into the order
                seen += [s0] if s1 == s0 else [s0, s1]
                lone += s1 == s0
                full += s1 != s0
        if nt <= 257:
            assert seen == list(range(nt))                                          # every tile once, in order
            assert (full, lone) == opm.pair_waves(nt)
            assert 4 * opm.grid(nt) >= nw and (nt == 0 or 4 * (opm.grid(nt) - 1) < nw)
    assert device_slots(lib, -1, 10)[0] is False
    assert lib.cp_test_own_pair(C.c_int64(4), C.c_int64(0), None) == 1             # CP_EINVAL


def test_round_a_tiles_of_the_test_sizes():
    """the sizes of tests/test_gpu_own_pair.py: round A alone gives a pair and, for most, a lone wave as well"""
    want = {513: 3, 600: 4, 767: 5, 768: 3, 769: 5}
    for n, nt in want.items():
        assert opm.round_a_tiles(n) == nt, n
        assert opm.round_a_tiles(n) >= 2
    assert opm.round_a_tiles(513, blk=0) == 3 and opm.round_a_tiles(769, blk=0) == 5
    assert opm.round_a_tiles(512) == 0 and opm.round_a_tiles(600, own_min=1000) == 0
