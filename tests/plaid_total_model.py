"""Executable statement (numpy / plain Python) of csrc/plaid_total.hip: the cost tables of the plaid connectivity pair from
their DEFINITION (the rows of a column range, owners from Pi), the primary layer as the unconstrained two-staircase layer of
tests/budget_model.py, the secondary layer as a prefix-min scan, and the literal K-layer DP both are compared with (small n); PrimaryCols and Secondary.column give rows and columns of the same cost
tables from the entry list alone, at any n, for the audits of tests/bellman_audit.py.

0-based indices as in budget_model: row r = j' - 1, candidate p = j - 1, F[p, r] = cost of the columns [p, r) as part k."""
import numpy as np

import brute
import sym_total_model as stm
from util import cp

PRIM, SEC = cp.AffinePrimaryConnectivityModel, cp.AffineSecondaryConnectivityModel
PREP_LAUNCHES = 2          # per layer >= 2 in front of the plan: the flag scatter and the scan of Lk, one timed step each


def dense(A):
    D = np.zeros((A.m, A.n), dtype=bool)
    cols = np.repeat(np.arange(A.n), np.diff(A.colptr))
    D[np.asarray(A.rowval, dtype=np.int64) - 1, cols] = True
    return D


def owners(Pi, m):
    """1-based part of every row"""
    if isinstance(Pi, cp.MapPartition):
        return np.asarray(Pi.asg, dtype=np.int64)
    spl = np.asarray(Pi.spl, dtype=np.int64)
    return np.searchsorted(spl, np.arange(1, m + 1), side="right").astype(np.int64)


def _dt(mdl):
    return np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64


def _alpha(mdl, k):
    return mdl.alpha if mdl.alpha_k is None else mdl.alpha_k[k - 1]


def _apply(mdl, k, nv, npins, local, remote):
    """alpha + nv*b_vertex + np*b_pin + local*b_local_net + remote*b_remote_net, left to right in the model's element type"""
    dt = _dt(mdl)
    F = np.full(np.shape(nv), _alpha(mdl, k), dtype=dt)
    F = F + np.asarray(nv).astype(dt) * dt(mdl.beta_vertex)
    F = F + np.asarray(npins).astype(dt) * dt(mdl.beta_pin)
    F = F + np.asarray(local).astype(dt) * dt(mdl.beta_local_net)
    return F + np.asarray(remote).astype(dt) * dt(mdl.beta_remote_net)


class Primary:
    """count tables of (A, Pi), built once: nets[p, r] the rows with an entry in the columns [p, r), local[k][p, r] those Pi gives to k"""

    def __init__(self, A, Pi):
        self.A, self.Pi = A, Pi
        D, n = dense(A), A.n
        own = owners(Pi, A.m)
        self.n = n
        self.pins = np.zeros((n + 1, n + 1), dtype=np.int64)
        self.nets = np.zeros((n + 1, n + 1), dtype=np.int64)
        self.local = {k: np.zeros((n + 1, n + 1), dtype=np.int64) for k in range(1, Pi.K + 1)}
        pos = np.concatenate([[0], np.cumsum(D.sum(axis=0))]).astype(np.int64)
        owned = np.stack([own == k for k in range(1, Pi.K + 1)]).astype(np.int64)       # K x m
        for p in range(n):
            seen = np.logical_or.accumulate(D[:, p:], axis=1)            # seen[i, t]: row i has an entry in the columns [p, p + t]
            self.pins[p, p + 1:] = pos[p + 1:] - pos[p]
            self.nets[p, p + 1:] = seen.sum(axis=0)
            loc = owned @ seen.astype(np.int64)
            for k in self.local:
                self.local[k][p, p + 1:] = loc[k - 1]

    def table(self, mdl, k):
        P, R = np.meshgrid(np.arange(self.n + 1), np.arange(self.n + 1), indexing="ij")
        loc = self.local[k] if k in self.local else np.zeros_like(self.nets)
        return np.triu(_apply(mdl, k, R - P, self.pins, loc, self.nets - loc))


class Secondary:
    """A: the pattern whose columns are split (the adjoint in the plaid callers), Pi: a SplitPartition of its rows.  has[k][c]: column c
    holds a row of part k; nv / w / d: the rows, pins and columns of part k.  From the entry list, so any size"""

    def __init__(self, A, Pi):
        self.A, self.Pi, self.n = A, Pi, A.n
        own = owners(Pi, A.m)
        cols = np.repeat(np.arange(A.n), np.diff(A.colptr))
        entry_owner = own[np.asarray(A.rowval, dtype=np.int64) - 1]
        self.has = {k: np.bincount(cols[entry_owner == k], minlength=A.n) > 0 for k in range(1, Pi.K + 1)}
        self.nv = {k: int((own == k).sum()) for k in self.has}
        self.w = {k: int((entry_owner == k).sum()) for k in self.has}
        self.d = {k: int(self.has[k].sum()) for k in self.has}

    def prefix(self, k):
        """P_k[c] = the columns < c that hold a row of part k, c = 0 .. n"""
        return np.concatenate([[0], np.cumsum(self.has[k])]).astype(np.int64)

    def first(self, mdl):
        """layer 1: f(0, r, 1) for r = 0 .. n"""
        Pk = self.prefix(1)
        return _apply(mdl, 1, np.full_like(Pk, self.nv[1]), np.full_like(Pk, self.w[1]), Pk, self.d[1] - Pk)

    def column(self, mdl, jp, k):
        """f(j, j', k) for j = 1 .. j' without the table: the columns [j - 1, j' - 1) that hold a row of part k are local, the part's
        other columns remote"""
        Pk = self.prefix(k)
        L = Pk[jp - 1] - Pk[:jp]
        return _apply(mdl, k, np.full_like(L, self.nv[k]), np.full_like(L, self.w[k]), L, self.d[k] - L)

    def table(self, mdl, k):
        Pk = self.prefix(k)
        L = Pk[None, :] - Pk[:, None]
        nv = np.full_like(L, self.nv[k]); w = np.full_like(L, self.w[k])
        return np.triu(_apply(mdl, k, nv, w, L, self.d[k] - L))


def scan_layer(W, S, mdl, k):
    """the secondary layer as the device runs it: cst[r] = const_k + S_k[r] + the prefix minimum of W[p] - S_k[p], the rightmost
    minimiser; S_k[c] = P_k[c]*b_local_net - P_k[c]*b_remote_net"""
    dt = _dt(mdl)
    Pk = S.prefix(k)
    Sk = Pk.astype(dt) * dt(mdl.beta_local_net) + (-Pk).astype(dt) * dt(mdl.beta_remote_net)
    const = dt(_alpha(mdl, k)) + dt(S.nv[k]) * dt(mdl.beta_vertex) + dt(S.w[k]) * dt(mdl.beta_pin) + dt(S.d[k]) * dt(mdl.beta_remote_net)
    v = np.asarray(W, dtype=dt) - Sk
    run = np.minimum.accumulate(v)
    # rightmost argmin of every prefix: the last position where the value equals the running minimum
    idx = np.where(v == run, np.arange(v.size), -1)
    ptr = np.maximum.accumulate(idx)
    return (const + Sk) + run, ptr.astype(np.int64)


def literal_dp(table_of_k, K, n):
    """DynamicSplitter.jl:15-50 in splitter order: ([cst of layer k], [ptr of layer k, 0-based]) for k = 1 .. K"""
    cst, ptr = [table_of_k(1)[0, :].copy()], [np.zeros(n + 1, dtype=np.int64)]
    for k in range(2, K + 1):
        c, p = brute.layer(cst[-1], table_of_k(k))
        cst.append(c); ptr.append(p)
    return cst, ptr


def scan_dp(S, mdl, K):
    """the same by scan_layer (sizes the literal DP cannot reach)"""
    cst, ptr = [S.first(mdl)], [np.zeros(S.n + 1, dtype=np.int64)]
    for k in range(2, K + 1):
        c, p = scan_layer(cst[-1], S, mdl, k)
        cst.append(c); ptr.append(p)
    return cst, ptr


def unravel(ptrs, n):
    """the 1-based split vector of 0-based argmin rows (unravel_splits, DynamicSplitter.jl:89-99)"""
    spl = [n]
    for p in reversed(ptrs):
        spl.append(int(p[spl[-1]]))
    return [s + 1 for s in reversed(spl)]


def launch_cap(n, stair):
    """launches of the profile slot for one layer >= 2 of the primary path: the plan's D (4 L + 2) + 1 and the preparation steps"""
    return stm.launch_cap(n, stair) + PREP_LAUNCHES


class PrimaryCols:
    """f(j, j', k) of the primary model along a row (j fixed) or a column (j' fixed) of its cost table from the entry list alone, so at
    any n: one stable sort of the entries by row gives every entry the previous and the next column that holds its row, and a call
    reads the entries of its window's columns once.  nets(p, r) counts the rows whose last column below r is >= p (for a fixed p: whose
    first column >= p is below r); local(p, r, k) those of them that Pi gives to part k.  Pi: a MapPartition or a SplitPartition
    (through owners); a part number past Pi.K owns no row.  The element type and the operand order are _apply's."""

    def __init__(self, A, Pi, mdl=None):
        self.A, self.Pi, self.mdl, self.n = A, Pi, mdl, A.n
        self.own = owners(Pi, A.m)
        self.pos = np.asarray(A.colptr, dtype=np.int64) - 1
        self.rows = np.asarray(A.rowval, dtype=np.int64) - 1
        self.cols = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(self.pos))
        nnz = self.rows.size
        order = np.argsort(self.rows, kind="stable")
        rs, cs = self.rows[order], self.cols[order]
        same = rs[1:] == rs[:-1]
        self.prev = np.full(nnz, -1, dtype=np.int64); self.prev[order[1:][same]] = cs[:-1][same]
        self.next = np.full(nnz, A.n, dtype=np.int64); self.next[order[:-1][same]] = cs[1:][same]

    def counts_col(self, r, k, p0=0):
        """(nets, local of part k) of the columns [p, r) for p = p0 .. r"""
        sl = slice(self.pos[p0], self.pos[r])
        last = self.next[sl] >= r
        c, mine = self.cols[sl][last], self.own[self.rows[sl][last]] == k
        at_least = lambda x: np.cumsum(np.bincount(x - p0, minlength=r - p0 + 1)[::-1])[::-1].astype(np.int64)
        return at_least(c), at_least(c[mine])

    def counts_row(self, p, k, r1=None):
        """the same for the columns [p, r), r = p .. r1"""
        r1 = self.n if r1 is None else r1
        sl = slice(self.pos[p], self.pos[r1])
        first = self.prev[sl] < p
        c, mine = self.cols[sl][first], self.own[self.rows[sl][first]] == k
        below = lambda x: np.concatenate([[0], np.cumsum(np.bincount(x - p, minlength=r1 - p))]).astype(np.int64)
        return below(c), below(c[mine])

    def row(self, j, k, upto=None):
        """f(j, j', k) for j' = j .. upto (n + 1 by default)"""
        p, r1 = j - 1, (self.n if upto is None else upto - 1)
        t = np.arange(p, r1 + 1, dtype=np.int64)
        nets, loc = self.counts_row(p, k, r1)
        return _apply(self.mdl, k, t - p, self.pos[t] - self.pos[p], loc, nets - loc)

    def column(self, jp, k, frm=1):
        """f(j, j', k) for j = frm .. j'"""
        r, p0 = jp - 1, frm - 1
        t = np.arange(p0, r + 1, dtype=np.int64)
        nets, loc = self.counts_col(r, k, p0)
        return _apply(self.mdl, k, r - t, self.pos[r] - self.pos[t], loc, nets - loc)
