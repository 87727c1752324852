"""Host models of the reordering layer (reference src/CuthillMcKeePermuter.jl, src/Permutations.jl), in the way of greedy_model.py.

Model A -- symrcm_loops / rctrcm_loops / permute_plaid_loops: the reference's loops restated statement by statement (1-based values in
0-based numpy arrays; `deg`, `bkt`, `ord`, `prm`, `vst` are its arrays), the block reordering with `deg` / `bkt` included.

Model B -- rcm_keys: the closed statement the device implements (csrc/rcm.hip).  A breadth-first walk in which the children of a
vertex are its unvisited neighbours in (degree, index) order and a new tree starts at the unvisited vertex of least (degree, index);
equivalently a vertex's place in the queue is fixed by (queue position of its parent, degree, index).

Both take a graph as (pos, adj): vertex v (0-based) has the neighbours adj[pos[v]:pos[v + 1]] (0-based), as listed.
tests/test_rcm_model.py holds A against B on patterns built to tie.
"""
import numpy as np

from util import cp


# ---------------------------------------------------------------- graphs
def sym_graph(A):
    """the graph symrcm walks: vertex j has the rows of column j (needs m == n)"""
    return A.colptr - 1, A.rowval - 1, A.n


def transpose(A):
    order = np.lexsort((np.repeat(np.arange(A.n), np.diff(A.colptr)), A.rowval))
    cols = np.repeat(np.arange(1, A.n + 1, dtype=np.int64), np.diff(A.colptr))[order]
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(A.rowval - 1, minlength=A.m))]).astype(np.int64)
    return cp.SparseMatrixCSC(A.n, A.m, colptr, cols)


def bip_graph(A, T=None):
    """the graph rctrcm walks: rows 0 .. m-1 with neighbours m + j (from the adjoint), columns m .. m+n-1 with neighbours i"""
    T = transpose(A) if T is None else T
    pos = np.concatenate([T.colptr - 1, A.nnz + A.colptr[1:] - 1])
    adj = np.concatenate([A.m + T.rowval - 1, A.rowval - 1])
    return pos, adj, A.m + A.n


def is_symmetric(A):
    if A.m != A.n:
        return False
    T = transpose(A)
    return np.array_equal(A.colptr, T.colptr) and np.array_equal(A.rowval, T.rowval)


# ---------------------------------------------------------------- model A: the loops
def rcm_loops(pos, adj, V):
    """symrcm (CuthillMcKeePermuter.jl:7-84) on the graph; rctrcm (:86-197) is the same text over the bipartite graph.
    -> (prm 0-based, number of trees)"""
    if V == 0:
        return np.zeros(0, dtype=np.int64), 0
    dg = np.diff(pos)
    # counting sort of the vertices by degree: ord (:14-29)
    cnt = np.zeros(int(dg.max()) + 3, dtype=np.int64)
    cnt[0] = 0
    for v in range(V):
        cnt[dg[v] + 1] += 1
    start = np.cumsum(cnt)
    ord_ = np.zeros(V, dtype=np.int64)
    for v in range(V):
        ord_[start[dg[v]]] = v
        start[dg[v]] += 1
    deg = np.zeros(V + 2, dtype=np.int64)
    bkt = np.zeros(V + 2, dtype=np.int64)
    prm = np.zeros(V + 2, dtype=np.int64)        # positions 1 .. V as in the reference
    vst = np.zeros(V, dtype=bool)
    k_start = 0
    k_current = 0
    k_frontier = 0
    trees = 0
    while k_frontier < V:
        k_current += 1
        if k_current > k_frontier:
            while vst[ord_[k_start]]:
                k_start += 1
            j = ord_[k_start]
            prm[k_current] = j
            k_frontier = k_current
            vst[j] = True
            trees += 1
        else:
            j = prm[k_current]
        kf = k_frontier
        for q in range(pos[j], pos[j + 1]):
            i = adj[q]
            if not vst[i]:
                kf += 1
                prm[kf] = i
                vst[i] = True
        if kf > k_frontier:
            deg[kf] = dg[prm[kf]]
            bkt[kf] = kf
            for k0 in range(kf - 1, k_frontier, -1):
                k = k0
                i = prm[k]
                d = dg[i]
                while k != kf and d > deg[k + 1]:
                    deg[k] = deg[bkt[k + 1]]
                    prm[k] = prm[bkt[k + 1]]
                    bkt[k] = bkt[k + 1] - (1 if d != deg[k + 1] else 0)
                    k = bkt[k + 1]
                prm[k] = i
                deg[k] = d
                bkt[k] = k
            k_frontier = kf
    return prm[1:V + 1].copy(), trees


# ---------------------------------------------------------------- model B: the keys
def rcm_keys(pos, adj, V):
    """-> (prm 0-based, number of trees, number of levels expanded before the queue is full)"""
    dg = np.diff(pos)
    ord_ = np.lexsort((np.arange(V), dg))
    visited = np.zeros(V, dtype=bool)
    queue = []
    k_start = trees = levels = 0
    lo = 0
    while len(queue) < V:
        if lo == len(queue):
            while visited[ord_[k_start]]:
                k_start += 1
            visited[ord_[k_start]] = True
            queue.append(int(ord_[k_start]))
            trees += 1
            continue
        hi = len(queue)
        par = {}
        for p in range(lo, hi):
            for v in adj[pos[queue[p]]:pos[queue[p] + 1]]:
                if not visited[v] and int(v) not in par:
                    par[int(v)] = p
        for v in sorted(par, key=lambda v: (par[v], dg[v], v)):
            visited[v] = True
            queue.append(v)
        levels += 1
        lo = hi
    return np.asarray(queue, dtype=np.int64), trees, levels


# ---------------------------------------------------------------- permute_plaid
def permute_plaid_model(A, reverse=False, assumesymmetry=False, checksymmetry=True, walk=rcm_loops):
    """permute_plaid(A, CuthillMcKeePermuter(...)) (:221-265) -> (iprm, jprm, symmetric path taken, trees), 1-based"""
    if assumesymmetry or (checksymmetry and is_symmetric(A)):
        assert A.m == A.n
        prm, trees = walk(*sym_graph(A))[:2]
        prm = prm + 1
        if reverse:
            prm = prm[::-1].copy()
        return prm, prm, True, trees
    m, n = A.m, A.n
    prm, trees = walk(*bip_graph(A))[:2]
    iprm = np.zeros(m, dtype=np.int64)
    jprm = np.zeros(n, dtype=np.int64)
    if reverse:
        i, j = m - 1, n - 1
        for v in prm:
            if v < m:
                iprm[i] = v + 1
                i -= 1
            else:
                jprm[j] = v - m + 1
                j -= 1
    else:
        i = j = 0
        for v in prm:
            if v < m:
                iprm[i] = v + 1
                i += 1
            else:
                jprm[j] = v - m + 1
                j += 1
    return iprm, jprm, False, trees


# ---------------------------------------------------------------- A[sigma, tau], bandwidth
def permuted(A, rowprm=None, colprm=None):
    """A[rowprm, colprm] by numpy (1-based permutations; None: the identity), rows ascending inside each column"""
    m, n = A.m, A.n
    rowprm = np.arange(1, m + 1) if rowprm is None else np.asarray(rowprm)
    colprm = np.arange(1, n + 1) if colprm is None else np.asarray(colprm)
    inv = np.zeros(m + 1, dtype=np.int64)
    inv[rowprm] = np.arange(1, m + 1)
    cols = []
    for c in colprm:
        cols.append(np.sort(inv[A.rowval[A.colptr[c - 1] - 1:A.colptr[c] - 1]]))
    colptr = np.concatenate([[1], 1 + np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rowval = np.concatenate(cols).astype(np.int64) if cols and colptr[-1] > 1 else np.zeros(0, dtype=np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rowval)


def bandwidth(A):
    """test/test_CuthillMcKee.jl:1-23"""
    m, n = A.m, A.n
    bot = np.zeros(n + 1, dtype=np.int64)
    bot[n] = m + 1
    for j in range(n - 1, -1, -1):
        bot[j] = min(bot[j + 1], A.rowval[A.colptr[j] - 1]) if A.colptr[j] < A.colptr[j + 1] else bot[j + 1]
    top = np.zeros(n + 1, dtype=np.int64)
    for j in range(n):
        top[j + 1] = max(top[j], A.rowval[A.colptr[j + 1] - 2]) if A.colptr[j] < A.colptr[j + 1] else top[j]
    return int((top[1:] - bot[:n]).max())


# ---------------------------------------------------------------- seeded patterns that tie
def from_mask(D):
    """pattern of a dense boolean matrix D[row, col]"""
    m, n = D.shape
    cols, rows = np.nonzero(D.T)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, rows.astype(np.int64) + 1)


def tying_pattern(seed, symmetric, nmax=40):
    """few distinct degrees, disconnected pieces, empty rows and columns, diagonal-only columns -- by seed"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, nmax + 1))
    m = n if symmetric or rng.random() < 0.3 else int(rng.integers(1, nmax + 1))
    style = int(rng.integers(0, 4))
    D = np.zeros((m, n), dtype=bool)
    if style == 0:                                   # every column draws its length from two or three values
        lens = rng.choice([0, 1, 2, 3][: int(rng.integers(2, 5))], size=n)
        for j in range(n):
            D[rng.choice(m, size=min(int(lens[j]), m), replace=False), j] = True
    elif style == 1:                                 # blocks on the diagonal: disconnected pieces
        b = int(rng.integers(1, 6))
        for j in range(n):
            lo = (j // b) * b
            rows = np.arange(lo, min(lo + b, m))
            if len(rows):
                D[rows[rng.random(len(rows)) < 0.6], j] = True
    elif style == 2:                                 # sparse uniform
        D = rng.random((m, n)) < float(rng.choice([0.03, 0.08, 0.2]))
    else:                                            # a band with holes
        h = int(rng.integers(1, 4))
        for j in range(n):
            rows = np.arange(max(0, j - h), min(m, j + h + 1))
            if len(rows):
                D[rows[rng.random(len(rows)) < 0.7], j] = True
    if symmetric:
        D = D | D.T
    k = min(m, n)
    dia = rng.random(k) < 0.3                        # diagonal entries count towards the degree
    D[np.arange(k)[dia], np.arange(k)[dia]] = True
    empty = rng.random(n) < 0.15
    D[:, empty] = False
    if symmetric:
        D[empty, :] = False
    else:
        D[rng.random(m) < 0.15, :] = False
    only = rng.random(k) < 0.1                       # diagonal-only columns
    for j in np.arange(k)[only]:
        D[:, j] = False
        if symmetric:
            D[j, :] = False
        D[j, j] = True
    return from_mask(D)
