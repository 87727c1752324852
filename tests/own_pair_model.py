"""Executable specification of the paired own-tile stream of csrc/dp_total_own.hip (cp_set_option("own_pair"), cp_test_own_pair): with
the option on, wave w of k_lpass_own takes the slots 2 w and 2 w + 1 of the run order of a round's nt own tiles (own_blk 1: the
order of k_blk_order; own_blk 0: the tile ids).  A wave whose second slot lies beyond the order takes its first slot again and
stores one tile: a lone wave.  The gap rounds and the hyperedge costs keep one tile per wave.

round_a_tiles: the own tiles of round A of a full layer, the one round that is never a gap round -- the last row n in every plane
b above its lowest set bit, candidates [r_b - 2^b, r_b] (own_split_model's blocks), tiles by own_ntiles."""
from own_split_model import nbits_of

LT = 256


def pair_slots(w, nt):
    """(has work, first slot, second slot) of wave w among nt tiles"""
    s0 = 2 * w
    return (w >= 0 and s0 < nt), s0, (s0 + 1 if s0 + 1 < nt else s0)


def pair_waves(nt):
    """(waves that run two tiles, waves that run one) for nt tiles"""
    return nt // 2, nt % 2


def grid(capacity):
    """workgroups of four waves that cover `capacity` tiles in pairs"""
    return -(-(-(-capacity // 2)) // 4)


def own_ntiles(blk, B, L):
    return B // LT - (B - L + 1) // LT + 1 if blk else -(-L // LT)


def round_a_tiles(n, own_min=64, blk=1):
    """own tiles of round A of a full layer over n columns (tasks of fewer than own_min steps are flattened or finished in setup)"""
    lowest = (n & -n).bit_length() - 1
    nt = 0
    for b in range(lowest + 1, nbits_of(n)):
        if (n >> b) & 1:
            B = (n >> b) << b
            L = (1 << b) + 1
            if L >= own_min:
                nt += own_ntiles(blk, B, L)
    return nt
