"""Executable specification (numpy) of the link entries split by bit plane, as the own tiles of csrc/dp_total_own.hip stream them
(cp_set_option("own_split"), cp_test_own_split).  0-based columns p = 0 .. n - 1; entry q of column p has next[q] = the next column
that holds q's row, n when there is none.

A left step of a DP task (row r, plane b) over column p counts #{q in p : next[q] >= r}.  The task's columns lie in the Fenwick
block [r_b - 2^b, r_b), r_b = r with its low b bits cleared, and r in [r_b, r_b + 2^b).  With x = next[q] and h = the highest bit in
which p and x differ (-1 when x == p):
    h < b : x lies in p's own block, x < r_b <= r            -> no row of the rectangle counts q
    h > b : x >= r_b + 2^b > r                               -> every row counts q
    h == b: x lies in the sibling block [r_b, r_b + 2^b)     -> the count depends on r: q is "variable in plane b"
so for columns [a, B) inside the block
    #{q in [a, B) : next[q] >= r}  =  vsa[b][B] - vsa[b][a]  +  #{variable entries of plane b in [a, B) : next >= r}.
The planes b = BMIN .. nbits - 1 are stored (index b - BMIN):
    vnext       the variable entries' next values: plane-major, column-major inside a plane, entry order inside a column
    vpos[b][p]  p = 0 .. n: where column p's plane-b entries start in vnext
    vsa[b][p]   #{entries of the columns < p with h > b}
"""
import numpy as np

BMIN = 8


def nbits_of(n):
    return max(1, int(n).bit_length())


def next_links(A):
    """(cols, next) per entry, in storage order"""
    n = A.n
    rows = np.asarray(A.rowval, dtype=np.int64) - 1
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(A.colptr, dtype=np.int64)))
    order = np.lexsort((cols, rows))                       # by (row, column)
    nxt = np.full(rows.size, n, dtype=np.int64)
    same = rows[order][1:] == rows[order][:-1]
    nxt[order[:-1][same]] = cols[order[1:][same]]
    return cols, nxt


def top_bit(v):
    """floor(log2(v)) per element, -1 for 0"""
    v = np.asarray(v, dtype=np.int64)
    out = np.full(v.shape, -1, dtype=np.int64)
    for b in range(63):
        out[(v >> b) > 0] = b
    return out


def split(A, bmin=BMIN):
    """(nb, vpos[nb, n + 1], vsa[nb, n + 1], vnext) as int32 arrays"""
    n = A.n
    nb = max(0, nbits_of(n) - bmin)
    cols, nxt = next_links(A)
    h = top_bit(cols ^ nxt)
    vpos = np.zeros((nb, n + 1), dtype=np.int64); vsa = np.zeros((nb, n + 1), dtype=np.int64)
    parts = []
    base = 0
    for i in range(nb):
        b = bmin + i
        sel = h == b
        cnt = np.bincount(cols[sel], minlength=n + 1)[:n + 1]
        vpos[i] = base + np.concatenate([[0], np.cumsum(cnt)[:-1]])
        parts.append(nxt[sel])                             # (boolean selection keeps the storage order: column-major, entry order)
        base += int(sel.sum())
        above = np.bincount(cols[h > b], minlength=n + 1)[:n + 1]
        vsa[i] = np.concatenate([[0], np.cumsum(above)[:-1]])
    vnext = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return nb, vpos.astype(np.int32), vsa.astype(np.int32), vnext.astype(np.int32)


def plane_end(vpos, vnext, i):
    """end of plane i's entries in vnext"""
    return int(vpos[i + 1, 0]) if i + 1 < vpos.shape[0] else int(vnext.size)


def direct_count(A, cols, nxt, a, B, r):
    pos = np.asarray(A.colptr, dtype=np.int64) - 1
    return int(np.sum(nxt[pos[a]:pos[B]] >= r))


def split_count(S, b, a, B, r, bmin=BMIN):
    """the same count from the split arrays, for columns [a, B) inside the block of (r, b)"""
    nb, vpos, vsa, vnext = S
    i = b - bmin
    lo, hi = int(vpos[i, a]), int(vpos[i, B])
    return int(vsa[i, B]) - int(vsa[i, a]) + int(np.sum(vnext[lo:hi] >= r))
