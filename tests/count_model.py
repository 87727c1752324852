"""Definitions of the counting structures in plain numpy; nothing here is shared with the device kernels or the host binding.

  dominance   Cn[i, j] = nnz(A[1:i-1, 1:j-1]),  P[i, j] = sum(A[1:i-1, 1:j-1])        (test_SparsePrefixMatrices.jl:14-15)
  rooks       the same over the N x N pattern with the one point (idx[c], c) per column c                           (:41-71)
  net         rows with an entry in the columns j : j'-1                                      (test_SparseColorArrays.jl:1-4)
  selfnet     non-empty rows whose entries all lie in the columns j : j'-1                                            (:5-9)

Tables are indexed by 0-based boundaries: T[a, b] is the value over the rows < a (or the columns >= a) and the columns < b, that
is the 1-based query (a + 1, b + 1).  Integer weights are summed as 64-bit words with wrap-around; Float64 sums that are not
exactly representable are produced exactly, as fractions (dom_sum_exact, rook_sum_exact).

The dianet / selfpin tables are sym_model.Tables; they are not restated here."""
import fractions

import numpy as np

ROOK_BLOCK = 1024          # rook_queries holds a (ROOK_BLOCK + 1) x (N + 1) table at a time, never N x N
LIMB = 30                  # exact sums: 30-bit limbs, so up to 2^33 terms add up in int64 without overflow


def _columns(A):
    return np.repeat(np.arange(A.n), np.diff(A.colptr))


def _prefix2(D, dtype):
    """T[a, b] = sum(D[:a, :b]) in dtype (integers wrap)"""
    T = np.zeros((D.shape[0] + 1, D.shape[1] + 1), dtype=dtype)
    with np.errstate(over="ignore"):
        T[1:, 1:] = np.cumsum(np.cumsum(D, axis=0, dtype=dtype), axis=1, dtype=dtype)
    return T


def dom_tables(A, val=None):
    """(Cn, P): (m+1) x (n+1) tables of the entry counts (int64) and of the weight sums in val's dtype (uint64 and int64 wrap,
    float64 is summed by cumsum: exact whenever every partial sum is representable).  P is None without weights."""
    rows, cols = A.rowval - 1, _columns(A)
    M = np.zeros((A.m, A.n), dtype=np.int64)
    M[rows, cols] = 1
    Cn = _prefix2(M, np.int64)
    if val is None:
        return Cn, None
    val = np.asarray(val)
    D = np.zeros((A.m, A.n), dtype=val.dtype)
    D[rows, cols] = val
    return Cn, _prefix2(D, val.dtype)


def rook_queries(N, idx, val, i, j, block=ROOK_BLOCK):
    """(count, sum) of the points (idx[c], c + 1), c = 0 .. N-1, with c + 1 < j and idx[c] < i, for arrays of 1-based queries.
    The rows are cut into bands of `block`; a band's dense prefix table answers its share of every query at once.  sum is in val's
    dtype (as dom_tables), None without weights."""
    idx = np.asarray(idx, dtype=np.int64)
    a = np.asarray(i, dtype=np.int64) - 1                # rows (0-based) < a
    b = np.asarray(j, dtype=np.int64) - 1                # columns (0-based) < b
    cnt = np.zeros(a.shape, dtype=np.int64)
    sm = None if val is None else np.zeros(a.shape, dtype=np.asarray(val).dtype)
    rows = idx - 1
    for r0 in range(0, N, block):
        r1 = min(r0 + block, N)
        c = np.nonzero((rows >= r0) & (rows < r1))[0]
        x = np.clip(a - r0, 0, r1 - r0)
        M = np.zeros((r1 - r0, N), dtype=np.int64)
        M[rows[c] - r0, c] = 1
        cnt += _prefix2(M, np.int64)[x, b]
        if val is not None:
            D = np.zeros((r1 - r0, N), dtype=sm.dtype)
            D[rows[c] - r0, c] = np.asarray(val)[c]
            with np.errstate(over="ignore"):
                sm = sm + _prefix2(D, sm.dtype)[x, b]
    return cnt, sm


# ---------------------------------------------------------------- Float64 sums without rounding
def _limbs(val):
    """val[k] = sign * sum_l limbs[l][k] * 2^(LIMB * l + e0), exactly: (list of int64 arrays carrying the sign, e0)"""
    val = np.asarray(val, dtype=np.float64)
    assert np.all(np.isfinite(val))
    mant, ex = np.frexp(np.abs(val))
    mant = (mant * 2.0 ** 53).astype(np.int64)           # |val| = mant * 2^(ex - 53), mant < 2^53: exact
    nz = mant != 0
    e0 = int((ex[nz] - 53).min()) if nz.any() else 0
    big = mant.astype(object) << np.where(nz, ex - 53 - e0, 0).astype(object)
    sign = np.where(val < 0, -1, 1).astype(np.int64)
    out = []
    while True:
        out.append((big & ((1 << LIMB) - 1)).astype(np.int64) * sign)
        big = big >> LIMB
        if not big.any():
            return out, e0


def _fractions(parts, e0):
    """object array of the exact values sum_l parts[l] * 2^(LIMB * l + e0)"""
    tot = np.zeros(parts[0].shape, dtype=object)
    for l, p in enumerate(parts):
        tot = tot + (p.astype(object) << (LIMB * l))
    unit = fractions.Fraction(2) ** e0
    return tot * unit


def exact(x):
    """float64 array -> object array of the same values as fractions"""
    limbs, e0 = _limbs(x)
    return _fractions(limbs, e0)


def dom_sum_exact(A, val, i, j):
    """(sums, S) for Float64 weights that do not add up exactly: sums[t] = sum(A[1:i[t]-1, 1:j[t]-1]) as a Fraction with no
    rounding at all (every weight is cut into 30-bit integer limbs, the limbs are summed as dom_tables sums Int64 weights, and the
    limb sums are put together as Python integers), S = sum(|val|), a Fraction as well."""
    limbs, e0 = _limbs(val)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    parts = [dom_tables(A, l)[1][i - 1, j - 1] for l in limbs]
    return _fractions(parts, e0), _fractions([np.abs(l).sum(keepdims=True) for l in limbs], e0)[0]


def rook_sum_exact(N, idx, val, i, j):
    """dom_sum_exact for a rook pattern (through rook_queries)"""
    limbs, e0 = _limbs(val)
    parts = [rook_queries(N, idx, l, i, j)[1] for l in limbs]
    return _fractions(parts, e0), _fractions([np.abs(l).sum(keepdims=True) for l in limbs], e0)[0]


# ---------------------------------------------------------------- nets
def row_cumcounts(mask):
    """C[row, b] = number of entries of the row in the columns < b; mask: m x n bool"""
    C = np.zeros((mask.shape[0], mask.shape[1] + 1), dtype=np.int32)
    C[:, 1:] = np.cumsum(mask, axis=1, dtype=np.int32)
    return C


def net_pairs(mask, j, jp, chunk=1 << 22):
    """(net, selfnet) of the 1-based column ranges [j, j') for arrays of pairs with j <= j': a row is a net of the range if it has
    an entry there, a self net if it is not empty and all its entries lie there"""
    C = row_cumcounts(mask)
    tot = C[:, -1][:, None]
    p, r = np.asarray(j, dtype=np.int64) - 1, np.asarray(jp, dtype=np.int64) - 1
    net = np.zeros(p.shape, dtype=np.int64)
    snet = np.zeros(p.shape, dtype=np.int64)
    step = max(1, chunk // max(mask.shape[0], 1))
    for s in range(0, p.size, step):                     # (blocks of pairs, to bound the m x pairs scratch)
        inside = C[:, r[s:s + step]] - C[:, p[s:s + step]]
        net[s:s + step] = (inside > 0).sum(axis=0)
        snet[s:s + step] = ((inside == tot) & (tot > 0)).sum(axis=0)
    return net, snet


def net_tables(A):
    """(net, selfnet) as (n+1) x (n+1) tables over 0-based boundaries p <= r (zero below the diagonal)"""
    mask = np.zeros((A.m, A.n), dtype=bool)
    mask[A.rowval - 1, _columns(A)] = True
    p, r = np.triu_indices(A.n + 1)
    net = np.zeros((A.n + 1, A.n + 1), dtype=np.int64)
    snet = np.zeros((A.n + 1, A.n + 1), dtype=np.int64)
    net[p, r], snet[p, r] = net_pairs(mask, p + 1, r + 1)
    return net, snet
