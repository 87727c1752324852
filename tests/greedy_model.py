"""Literal Python restatement of the reference's two greedy chunkers, loop for loop; it shares no code with the device kernels.

  strict_chunks(A, w_max)        StrictChunker.jl:5-54
  overlap_chunks(A, rho, w_max)  OverlapChunker.jl:6-75, with its hst bookkeeping (:41-56), n_nets (:59, :67) and the first
                                 column's cardinality c, which the sweep never refreshes at a split (:58-63 set d = c' only)

Arrays are used 1-based as the reference uses them (index 0 is padding).  Also here: the seeded column-copying generator the tests of
the chunkers draw their patterns from, the host transpose, and the brute-force distinct-row count of a part."""
import numpy as np

import cpamd

cp = cpamd.load()


def _one_based(A):
    pos = [0] + [int(x) for x in A.colptr]
    idx = [0] + [int(x) for x in A.rowval]
    return pos, idx


def strict_chunks(A, w_max):
    n = A.n
    pos, idx = _one_based(A)
    spl = [0] * (n + 2)
    c = pos[2] - pos[1]
    j = 1
    K = 0
    spl[1] = 1
    for jp in range(2, n + 1):
        cp_ = pos[jp + 1] - pos[jp]
        w = jp - j
        d = True
        if c == cp_ and w != w_max:
            lp = pos[jp]
            for l in range(pos[j], pos[j + 1]):
                if idx[l] != idx[lp]:
                    d = False
                    break
                lp += 1
        else:
            d = False
        if not d:
            K += 1
            spl[K + 1] = jp
            j = jp
            c = cp_
    K += 1
    spl[K + 1] = n + 1
    return np.array(spl[1:K + 2], dtype=np.int64)


def overlap_chunks(A, rho, w_max):
    """-> (spl, n_nets)"""
    m, n = A.m, A.n
    pos, idx = _one_based(A)
    rho = float(rho)
    hst = [0] * (m + 1)
    spl = [0] * (n + 2)
    n_nets = [0] * (n + 1)
    d = pos[2] - pos[1]
    c = pos[2] - pos[1]
    j = 1
    K = 0
    spl[1] = 1
    for q in range(pos[1], pos[2]):
        hst[idx[q]] = 1
    for jp in range(2, n + 1):
        cp_ = pos[jp + 1] - pos[jp]
        dp = d
        cc = 0
        for q in range(pos[jp], pos[jp + 1]):
            i = idx[q]
            h = hst[i]
            if abs(h) == j:
                cc += 1
                hst[i] = -jp
            elif j < h:
                hst[i] = jp
            elif h < -j:
                cc += 1
                hst[i] = -jp
            else:
                dp += 1
                hst[i] = jp
        w = jp - j
        if w == w_max or float(cc) < rho * float(min(c, cp_)):
            K += 1
            spl[K + 1] = jp
            n_nets[K] = d
            j = jp
            d = cp_
        else:
            d = dp
    K += 1
    n_nets[K] = d
    spl[K + 1] = n + 1
    return np.array(spl[1:K + 2], dtype=np.int64), np.array(n_nets[1:K + 1], dtype=np.int64)


def part_nets(A, spl):
    """distinct rows of every part, by brute force"""
    return np.array([len(set(A.rowval[A.colptr[a - 1] - 1:A.colptr[b - 1] - 1].tolist())) for a, b in zip(spl[:-1], spl[1:])], dtype=np.int64)


def from_columns(m, cols):
    """cols: one ascending array of 0-based rows per column"""
    colptr = np.concatenate([[1], 1 + np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rowval = (np.concatenate(cols).astype(np.int64) + 1) if len(cols) and colptr[-1] > 1 else np.zeros(0, dtype=np.int64)
    return cp.SparseMatrixCSC(m, len(cols), colptr, rowval)


def copy_columns(m, n, density, seed, p_copy=0.5, p_flip=0.15):
    """Columns of i.i.d. entries at `density`; a column copies its left neighbour with probability p_copy, and copies it with one
    entry flipped with probability p_flip -- runs of identical columns for StrictChunker, near-copies for OverlapChunker."""
    rng = np.random.default_rng(seed)
    D = rng.random((n, m)) < density
    u = rng.random(n)
    flip = rng.integers(0, m, n)
    for j in range(1, n):
        if u[j] < p_copy:
            D[j] = D[j - 1]
        elif u[j] < p_copy + p_flip:
            D[j] = D[j - 1]
            D[j, flip[j]] ^= True
    return from_columns(m, [np.nonzero(D[j])[0] for j in range(n)])


def transpose(A):
    """adjointpattern(A) on the host (util.jl:67-95): rows of every column ascending"""
    cols = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(A.colptr))
    rows = np.asarray(A.rowval, dtype=np.int64) - 1
    order = np.lexsort((cols, rows))
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(rows, minlength=A.m))]).astype(np.int64)
    return cp.SparseMatrixCSC(A.n, A.m, colptr, cols[order] + 1)
