"""Audit of a device DP table against the Bellman recurrence, cell by sampled cell, with the costs handed in by the caller as
definition-level rows and columns (sym_model.Sym, plaid_total_model.PrimaryCols, envelope_model.Env): no dense table, so any n, and
no code of the library on the referee's side.  Pure numpy.

  audit(ptr, cst, K, row_of, column_of, rows)     library-shaped tables (n + 1) x K, ptr 1-based (DynamicSplitter.jl:15-50)
      layer 1        every cell: cst[:, 0] == row_of(1, 1), ptr[:, 0] == 1
      layer 2..K-1   for each r in rows: v = cst[:r + 1, k - 2] + column_of(r + 1, k); cst[r, k - 1] == min v and ptr[r, k - 1] - 1 is
                     the LARGEST minimiser (:37-43)
      layer K        row n alone
      -> {"cells", "interior", "tied"}: audited cells of the layers >= 2, those whose argmin p has 0 < p < r, those with two or more
         minimisers -- all three from column_of's values, none from the table alone, so a caller can assert that the audit decided
         something
  audit_rows(n, stair_cols, seed, nrand)          the rows where the rectangle engine changes its path, and nrand seeded random ones

  fixed_ends / line_pairs                         whole rows and columns of a count or cost table as one batch of (j, j') queries

row_of(j, k) is f(j, j', k) for j' = j .. n + 1, column_of(j', k) is f(j, j', k) for j = 1 .. j'.  The loop runs the layers inside the
rows, so a column_of that remembers its last column (same_for_all_k) costs one O(nnz) pass per row."""
import numpy as np

PATH_EDGES = (256, 1024, 4096, 8192)       # one column chunk of a level row, LWS_STAIR_COLS / LWS_BRUTE_COLS, LWS_LDS_ROWS, twice that
TREE_DEPTH = 3


def tree_rows(n, stair_cols, depth=TREE_DEPTH):
    """jm, jm + 1, jm + 2 of every block [ja, jb] of the column tree of csrc/lws_decomp.hpp down to `depth`: the tree starts at [0, n]
    and splits a block of at least stair_cols + 1 columns at jm = (ja + jb) // 2 into [ja, jm] and [jm + 1, jb]; these are the first
    and last rows of the full rectangles"""
    out, blocks = [], [(0, n)]
    for _ in range(depth + 1):
        nxt = []
        for ja, jb in blocks:
            if jb - ja < stair_cols:
                continue
            jm = (ja + jb) // 2
            out += [jm, jm + 1, jm + 2]
            nxt += [(ja, jm), (jm + 1, jb)]
        blocks = nxt
    return [r for r in out if r <= n]


def structural_rows(n, stair_cols):
    rows = [0, 1, 2, n - 1, n] + [c + d for c in PATH_EDGES for d in (-1, 0, 1)] + tree_rows(n, stair_cols)
    return np.unique([r for r in rows if 0 <= r <= n]).astype(np.int64)


def audit_rows(n, stair_cols, seed, nrand):
    rnd = np.random.default_rng(seed).integers(0, n + 1, nrand)
    return np.unique(np.concatenate([structural_rows(n, stair_cols), rnd])).astype(np.int64)


def same_for_all_k(column_of):
    """a column_of for a model without alpha_k: the column is computed for the first k asked and kept while j' stays"""
    kept = {}

    def f(jp, k):
        if kept.get("jp") != jp:
            kept.update(jp=jp, v=column_of(jp, k))
        return kept["v"]
    return f


def _cell(ptr, cst, r, k, column_of, counts):
    with np.errstate(over="ignore"):
        v = cst[:r + 1, k - 2] + column_of(r + 1, k)
    assert v.dtype == cst.dtype and v.size == r + 1, (v.dtype, cst.dtype, v.size, r)
    best = v.min()
    at = np.nonzero(v == best)[0]
    assert cst[r, k - 1] == best, ("cst", r, k, cst[r, k - 1], best)
    assert ptr[r, k - 1] - 1 == at[-1], ("ptr", r, k, int(ptr[r, k - 1]) - 1, int(at[-1]))
    counts["cells"] += 1
    counts["interior"] += int(0 < at[-1] < r)
    counts["tied"] += int(at.size >= 2)


def audit(ptr, cst, K, row_of, column_of, rows):
    n = cst.shape[0] - 1
    assert ptr.shape[0] == n + 1 and ptr.shape[1] >= K and cst.shape[1] >= K
    first = row_of(1, 1)
    assert first.dtype == cst.dtype and np.array_equal(cst[:, 0], first), "layer 1 cst"
    assert np.array_equal(ptr[:, 0], np.ones(n + 1, dtype=ptr.dtype)), "layer 1 ptr"
    counts = {"cells": 0, "interior": 0, "tied": 0}
    rows = [int(r) for r in rows]
    assert all(0 <= r <= n for r in rows)
    for r in rows:
        for k in range(2, K):
            _cell(ptr, cst, r, k, column_of, counts)
    if K >= 2:
        _cell(ptr, cst, n, K, column_of, counts)
    return counts


def fixed_ends(A, rng, count, blk=2048):
    """`count` 1-based boundaries: 1, 2, n, n + 1, up to a third of them where colptr crosses a multiple of blk (the keys of one block of
    the wavelet build), the rest random"""
    n = A.n
    pos = np.asarray(A.colptr, dtype=np.int64) - 1
    cross = np.nonzero(np.diff(pos // blk) > 0)[0] + 1
    ends = [1, 2, n, n + 1] + rng.choice(cross, min(cross.size, count // 3), replace=False).tolist()
    ends = np.unique([e for e in ends if 1 <= e <= n + 1])
    while ends.size < count:
        ends = np.unique(np.concatenate([ends, rng.integers(1, n + 2, count - ends.size)]))
    return ends.astype(np.int64)


def line_pairs(n, ends, starts):
    """every (j, e) with j = 1 .. e for e in ends, then every (s, j') with j' = s .. n + 1 for s in starts, as two int64 vectors"""
    j = [np.arange(1, e + 1, dtype=np.int64) for e in ends] + [np.full(n + 2 - s, s, dtype=np.int64) for s in starts]
    jp = [np.full(e, e, dtype=np.int64) for e in ends] + [np.arange(s, n + 2, dtype=np.int64) for s in starts]
    return np.concatenate(j), np.concatenate(jp)
