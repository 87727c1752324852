"""Executable specification (numpy) of the packed form of the split link entries (cp_set_option("own_pack"), cp_test_own_pack;
csrc/dp_total.hpp, SplitLinks), derived from tests/own_split_model.py.

An own tile of the geometry own_blk 1 lies inside one 256-column block, and vpos / vsa of own_split_model.split only enter it as
differences inside that block.  With c0 = p - p % 256, k = p // 256 and blocks = ceil((n + 1) / 256), per stored plane i:
    vpk[i][p]    = ((vpos[i][p] - vpos[i][c0]) & 0xffff) | ((vsa[i][p] - vsa[i][c0]) & 0xffff) << 16        p = 0 .. n
    vbase[i][k]  = (vpos[i][256 k], vsa[i][256 k])                                                           k = 0 .. blocks - 1
    vbase[i][blocks] = (end of plane i's entries in vnext, 0)
The last entry is what the wide arrays hold one word behind the plane's last column (the next plane's first words) where n + 1 is a
multiple of 256; it exists for every n, so that the block after a tile's always has an entry.
The pattern runs packed iff both offsets are below 2^16 everywhere; both grow with p inside a block.
"""
import numpy as np

import own_split_model as osm
from util import cp

BLK = 256


def boundary(c, n=600):
    """m = 256 c rows, row i in the columns i % 256 and 256 + i % 256; the columns 512 .. n - 1 are empty.  Every entry of a column
    p < 256 is variable in plane 8 and every entry of 256 + p in plane 9: the largest in-block offset of both fields is 255 c."""
    m = 256 * c
    i = np.arange(m, dtype=np.int64)
    cols = np.concatenate([i % 256, 256 + i % 256])
    rows = np.concatenate([i, i])
    order = np.lexsort((rows, cols))
    cols, rows = cols[order], rows[order]
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows + 1)



def pack(A, bmin=osm.BMIN):
    """(nb, vpk[nb, n + 1] uint32, vbase[nb, blocks + 1, 2] int32, info) with info = {blocks, packed, max_start, max_prefix}"""
    n = A.n
    nb, vpos, vsa, vnext = osm.split(A, bmin)
    blocks = (n + 1 + BLK - 1) // BLK
    c0 = (np.arange(n + 1) // BLK) * BLK
    vpk = np.zeros((nb, n + 1), dtype=np.uint32)
    vbase = np.zeros((nb, blocks + 1, 2), dtype=np.int32)
    max_start = max_prefix = 0
    for i in range(nb):
        op = vpos[i].astype(np.int64) - vpos[i, c0]
        os_ = vsa[i].astype(np.int64) - vsa[i, c0]
        assert np.all(op >= 0) and np.all(os_ >= 0)
        vpk[i] = ((op & 0xffff) | ((os_ & 0xffff) << 16)).astype(np.uint32)
        vbase[i, :blocks, 0] = vpos[i, ::BLK]
        vbase[i, :blocks, 1] = vsa[i, ::BLK]
        vbase[i, blocks] = (osm.plane_end(vpos, vnext, i), 0)
        max_start, max_prefix = max(max_start, int(op.max())), max(max_prefix, int(os_.max()))
    info = {"blocks": blocks, "packed": int(max_start <= 0xffff and max_prefix <= 0xffff), "max_start": max_start, "max_prefix": max_prefix}
    return nb, vpk, vbase, info


def unpack(n, vpk, vbase):
    """(vpos, vsa) of own_split_model.split from the packed form (exact where the pattern runs packed)"""
    k = np.arange(n + 1) // BLK
    w = vpk.astype(np.int64)
    vpos = vbase[:, :, 0].astype(np.int64)[:, k] + (w & 0xffff)
    vsa = vbase[:, :, 1].astype(np.int64)[:, k] + (w >> 16)
    return vpos.astype(np.int32), vsa.astype(np.int32)


def tile_ends(vpk, vbase, i, a, B, head):
    """What a tile of plane i over the columns a .. B of one block reads: (Q_lo, Q_hi, ptop) -- the run of vnext it streams and the
    prefix sum its steps start from, relative to the block's base.  head: the tile's first step is the candidate B itself, the run
    ends in front of column B; otherwise B is the block's last column and the run ends where the next block starts."""
    k = a // BLK
    assert B // BLK == k and (head or B % BLK == BLK - 1)
    bp, bs = (int(v) for v in vbase[i, k])
    q_lo = bp + (int(vpk[i, a]) & 0xffff)
    if head:
        return q_lo, bp + (int(vpk[i, B]) & 0xffff), int(vpk[i, B]) >> 16
    return q_lo, int(vbase[i, k + 1, 0]), int(vbase[i, k + 1, 1]) - bs


def packed_count(P, S, b, a, B, r, bmin=osm.BMIN):
    """own_split_model.split_count for the columns [a, B) of ONE 256-column block, from the packed form: B itself is the head
    column (a head tile), or B is the first column of the next block (a tile that ends at its block's last column)"""
    nb, vpk, vbase, info = P
    vnext = S[3]
    i = b - bmin
    if a == B:
        return 0
    if B % BLK == 0:
        q_lo, q_hi, ptop = tile_ends(vpk, vbase, i, a, B - 1, False)
    else:
        q_lo, q_hi, ptop = tile_ends(vpk, vbase, i, a, B, True)
    return ptop - (int(vpk[i, a]) >> 16) + int(np.sum(vnext[q_lo:q_hi] >= r))
