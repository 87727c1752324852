"""Pure-Python / numpy statement of the plaid edge-cut costs, written from the definitions and the reference's loops; it shares no
code with the device kernels or with the host mirror's marshalling.

  primary    f(j, j', k) = alpha_k + (j' - j)*b_vertex + l*b_self_pin + (w - l)*b_cut_pin      PrimaryEdgeCutCosts.jl:18, :51-57
  secondary  f(i, i', k) = alpha_k + nv_k*b_vertex + l*b_self_pin + (w_k - l)*b_cut_pin        SecondaryEdgeCutCosts.jl:18, :78-85
  l = #{entries of the columns [j, j') whose row part k of Pi owns}, counted entry by entry
  the literal K-layer DP (DynamicSplitter.jl:15-50, ties: the largest j), the scan formulation of DESIGN 5d restated in numpy,
  the three bound_stripe forms, and the [Flip]BisectCost / [Flip]BisectIndex loops over any f(j, j', k).

Costs are evaluated left to right in the model's element type (Int64 wraps).  Tables are indexed by 0-based boundaries."""
import math

import numpy as np

from sym_model import _acc, _is_int_model


def owner_of(Pi, m):
    """the 1-based part of every row, from a SplitPartition or a MapPartition"""
    if hasattr(Pi, "asg"):
        return np.asarray(Pi.asg, dtype=np.int64)
    own = np.zeros(m, dtype=np.int64)
    for k in range(Pi.K):
        own[int(Pi.spl[k]) - 1:int(Pi.spl[k + 1]) - 1] = k + 1
    return own


def prefix_counts(A, own, K):
    """L[k - 1, c] = entries of the columns < c whose row part k owns: one entry at a time"""
    L = np.zeros((K, A.n + 1), dtype=np.int64)
    for c in range(A.n):
        L[:, c + 1] = L[:, c]
        for q in range(int(A.colptr[c]) - 1, int(A.colptr[c + 1]) - 1):
            L[own[int(A.rowval[q]) - 1] - 1, c + 1] += 1
    return L


class Cut:
    """the oracle of one (pattern, row partition, model)"""

    def __init__(self, A, Pi, mdl):
        self.A, self.Pi, self.mdl = A, Pi, mdl
        self.secondary = type(mdl).__name__ == "AffineSecondaryEdgeCutModel"
        assert self.secondary or type(mdl).__name__ == "AffinePrimaryEdgeCutModel"
        self.dt = np.int64 if _is_int_model(mdl) else np.float64
        self.pos = (np.asarray(A.colptr) - 1).astype(np.int64)
        self.L = prefix_counts(A, owner_of(Pi, A.m), Pi.K)
        if self.secondary:
            deg = np.zeros(A.m + 1, dtype=np.int64)                     # pins of every row
            for i in np.asarray(A.rowval)[:A.nnz]:
                deg[int(i)] += 1
            rpos = np.cumsum(deg)
            s = np.asarray(Pi.spl, dtype=np.int64)
            self.nv = s[1:] - s[:-1]
            self.w = rpos[s[1:] - 1] - rpos[s[:-1] - 1]
        self._tab = {}

    def alpha(self, k):
        ak = getattr(self.mdl, "alpha_k", None)
        return self.mdl.alpha if ak is None else ak[k - 1]

    def table(self, k):
        """F[p, r] = f(p + 1, r + 1, k) for p <= r, zeros below the diagonal"""
        if k not in self._tab:
            n, m = self.A.n, self.mdl
            P, R = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
            l = self.L[k - 1][R] - self.L[k - 1][P]
            if self.secondary:
                nv = np.full_like(l, self.nv[k - 1]); w = np.full_like(l, self.w[k - 1])
            else:
                nv = (R - P).astype(np.int64); w = self.pos[R] - self.pos[P]
            self._tab[k] = np.triu(_acc(self.dt, self.alpha(k), [(nv, m.beta_vertex), (l, m.beta_self_pin), (w - l, m.beta_cut_pin)]))
        return self._tab[k]

    def f(self, j, jp, k):
        return self.table(k)[j - 1, jp - 1].item()


def objective(C, spl, combine):
    vals = [C.f(int(spl[k]), int(spl[k + 1]), k + 1) for k in range(len(spl) - 1)]
    if combine == "max":
        return max(vals)
    acc = np.zeros(1, dtype=C.dt)
    with np.errstate(over="ignore"):
        for v in vals:
            acc = acc + np.array([v], dtype=C.dt)
    return acc[0].item()


def dp(C, K, combine):
    """the literal DP: cst[r, k] = min over p <= r of g(cst[p, k - 1], f(p, r, k)), the largest p among equals (`<=` while p grows).
    -> (spl 1-based, cst[k - 1][r], ptr[k - 1][r] 0-based)"""
    n = C.A.n
    csts = [C.table(1)[0, :].copy()]
    ptrs = [np.zeros(n + 1, dtype=np.int64)]
    for k in range(2, K + 1):
        F, W = C.table(k), csts[-1]
        new = np.zeros_like(W); ptr = np.zeros(n + 1, dtype=np.int64)
        for r in range(n + 1):
            with np.errstate(over="ignore"):
                v = W[:r + 1] + F[:r + 1, r] if combine == "sum" else np.maximum(W[:r + 1], F[:r + 1, r])
            i = v.size - 1 - int(np.argmin(v[::-1]))
            new[r] = v[i]; ptr[r] = i
        csts.append(new); ptrs.append(ptr)
    spl = [0] * (K + 1)
    at = n
    spl[K] = n + 1
    for k in range(K, 0, -1):
        at = int(ptrs[k - 1][at])
        spl[k - 1] = at + 1
    return np.array(spl, dtype=np.int64), csts, ptrs


def dp_scan(A, Pi, mdl, K):
    """the total-cost DP as K prefix-minimum scans (exact models only): per layer flag the entries part k owns, scan the flags,
    read the scan at the column starts, scan v[p] = W[p] - S_k[p] for its running minimum and the rightmost argmin.
    -> (spl 1-based, cst[k - 1][r], ptr[k - 1][r] 0-based)"""
    n = A.n
    sec = type(mdl).__name__ == "AffineSecondaryEdgeCutModel"
    dt = np.int64 if _is_int_model(mdl) else np.float64
    pos = (np.asarray(A.colptr) - 1).astype(np.int64)
    own = owner_of(Pi, A.m)[np.asarray(A.rowval[:A.nnz], dtype=np.int64) - 1]
    bv, bs, bc = (dt(x) for x in (mdl.beta_vertex, mdl.beta_self_pin, mdl.beta_cut_pin))
    ak = getattr(mdl, "alpha_k", None)
    if sec:
        deg = np.bincount(np.asarray(A.rowval[:A.nnz], dtype=np.int64), minlength=A.m + 1)
        rpos = np.cumsum(deg)
        s = np.asarray(Pi.spl, dtype=np.int64)
    cols = np.arange(n + 1, dtype=np.int64)
    csts, ptrs = [], []
    for k in range(1, K + 1):
        Lq = np.concatenate([[0], np.cumsum(own == k)]).astype(np.int64)
        Lc = Lq[pos]
        alpha = dt(mdl.alpha if ak is None else ak[k - 1])
        if sec:
            S = Lc.astype(dt) * bs - Lc.astype(dt) * bc
            const = alpha + dt(s[k] - s[k - 1]) * bv + dt(rpos[s[k] - 1] - rpos[s[k - 1] - 1]) * bc
        else:
            S = cols.astype(dt) * bv + Lc.astype(dt) * bs + (pos - Lc).astype(dt) * bc
            const = alpha
        if k == 1:
            csts.append(const + S - S[0]); ptrs.append(np.zeros(n + 1, dtype=np.int64))
            continue
        v = csts[-1] - S
        run = np.minimum.accumulate(v)
        arg = np.maximum.accumulate(np.where(v == run, cols, -1))       # the last p <= r that set or tied the running minimum
        csts.append(const + S + run); ptrs.append(arg)
    spl = [0] * (K + 1)
    at = n
    spl[K] = n + 1
    for k in range(K, 0, -1):
        at = int(ptrs[k - 1][at])
        spl[k - 1] = at + 1
    return np.array(spl, dtype=np.int64), csts, ptrs


# ---------------------------------------------------------------- bound_stripe
def _fld(a, K, is_int):
    return a // K if is_int else math.floor(a / K)


def bound_primary(A, K, mdl):
    """PrimaryEdgeCutCosts.jl:28-39"""
    assert mdl.beta_vertex >= 0 and mdl.beta_self_pin >= 0 and mdl.beta_cut_pin >= 0
    c_hi = mdl.alpha + mdl.beta_vertex * A.n + max(mdl.beta_self_pin, mdl.beta_cut_pin) * A.nnz
    c_lo = mdl.alpha + _fld(mdl.beta_vertex * A.n + min(mdl.beta_self_pin, mdl.beta_cut_pin) * A.nnz, K, _is_int_model(mdl))
    return c_lo, c_hi


def _parts(A, Pi):
    deg = np.bincount(np.asarray(A.rowval[:A.nnz], dtype=np.int64), minlength=A.m + 1)
    rpos = np.cumsum(deg)
    s = [int(x) for x in Pi.spl]
    return [(s[k + 1] - s[k], int(rpos[s[k + 1] - 1] - rpos[s[k] - 1])) for k in range(Pi.K)]


def bound_secondary_model(A, K, Pi, mdl):
    """SecondaryEdgeCutCosts.jl:20-28: the work bottleneck of the adjoint under Pi, b_self_pin below and b_cut_pin above, all parts"""
    assert mdl.beta_vertex >= 0 and mdl.beta_self_pin >= 0 and mdl.beta_cut_pin >= 0
    pr = _parts(A, Pi)
    c_hi = max(mdl.alpha + nv * mdl.beta_vertex + w * mdl.beta_cut_pin for nv, w in pr)
    c_lo = max(mdl.alpha + nv * mdl.beta_vertex + w * mdl.beta_self_pin for nv, w in pr)
    return c_lo, c_hi


def bound_secondary_oracle(A, K, Pi, mdl):
    """SecondaryEdgeCutCosts.jl:40-57: parts 1..K, min / max of the two betas, from 0"""
    assert mdl.beta_vertex >= 0 and mdl.beta_self_pin >= 0 and mdl.beta_cut_pin >= 0
    c_lo = c_hi = 0
    for nv, w in _parts(A, Pi)[:K]:
        c_lo = max(c_lo, mdl.alpha + nv * mdl.beta_vertex + w * min(mdl.beta_self_pin, mdl.beta_cut_pin))
        c_hi = max(c_hi, mdl.alpha + nv * mdl.beta_vertex + w * max(mdl.beta_self_pin, mdl.beta_cut_pin))
    return c_lo, c_hi


def bisect_bounds(C, K):
    """what the Bisect splitters start from: bound_stripe(A, K, Pi, ocl) (BisectCostBottleneckSplitter.jl:39)"""
    return bound_secondary_oracle(C.A, K, C.Pi, C.mdl) if C.secondary else bound_primary(C.A, K, C.mdl)


# ---------------------------------------------------------------- the Bisect loops over any f(j, j', k)
def _search(f, flip, j, lo, hi, k, c):
    lo = max(j, lo)
    while lo <= hi:
        mid = (lo + hi) >> 1
        if (f(j, mid, k) <= c) != bool(flip):
            lo = mid + 1
        else:
            hi = mid - 1
    return lo if flip else hi


def _chain(f, flip, n, K, spl, spl_lo, spl_hi, k0, c):
    """the searches for the parts k0 .. K - 1 from spl[k0 - 1]; -> feasible"""
    for k in range(k0, K):
        j = spl[k - 1]
        rr = _search(f, flip, j, spl_lo[k], spl_hi[k], k, c)
        spl[k] = rr
        if (rr > n + 1) if flip else (rr < j):
            for t in range(k, K):
                spl[t] = (n + 1) if flip else j
            return False
    return f(spl[K - 1], spl[K], K) <= c


def bisect_cost(f, n, K, eps, c_lo, c_hi, flip=0):
    """BisectCostBottleneckSplitter.jl:6-63, flip :70-127"""
    c_lo, c_hi = c_lo / 1, c_hi / 1
    spl_lo = [1] * (K + 1); spl_hi = [n + 1] * (K + 1); spl = [0] * (K + 1)
    spl_lo[K] = n + 1; spl_hi[0] = 1; spl[0] = 1; spl[K] = n + 1
    probes = 0
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        assert probes <= 4096, "the bisection does not terminate on these bounds"
        spl[0] = 1
        if _chain(f, flip, n, K, spl, spl_lo, spl_hi, 1, c):
            c_hi = c
            if flip:
                spl_lo = list(spl)
            else:
                spl_hi = list(spl)
        else:
            c_lo = c
            if flip:
                spl_hi = list(spl)
            else:
                spl_lo = list(spl)
    return np.array(spl_lo if flip else spl_hi, dtype=np.int64)


def bisect_index(f, n, K, c_lo, c_hi, flip=0):
    """BisectIndexBottleneckSplitter.jl:5-83, flip :85-166"""
    c_lo, c_hi = c_lo / 1, c_hi / 1
    spl_lo = [1] * (K + 1); spl_hi = [n + 1] * (K + 1); spl = [0] * (K + 1)
    spl_lo[K] = n + 1; spl_hi[0] = 1; spl[0] = 1; spl[K] = n + 1
    for k in range(1, K + 1):
        jhi = spl_hi[k]
        jlo = max(spl[k - 1], spl_lo[k])
        while jlo <= jhi:
            jp = (jlo + jhi) >> 1
            c = f(spl[k - 1], jp, k)
            if c_lo <= c < c_hi:
                spl[k] = jp
                ok = _chain(f, flip, n, K, spl, spl_lo, spl_hi, k + 1, c)
                if ok:
                    c_hi = c
                    if flip:
                        jlo = jp + 1; spl_lo = list(spl)
                    else:
                        jhi = jp - 1; spl_hi = list(spl)
                else:
                    c_lo = c
                    if flip:
                        jhi = jp - 1; spl_hi = list(spl)
                    else:
                        jlo = jp + 1; spl_lo = list(spl)
            elif c >= c_hi:
                if flip:
                    jlo = jp + 1
                else:
                    jhi = jp - 1
            else:
                if flip:
                    jhi = jp - 1
                else:
                    jlo = jp + 1
        if flip:
            if jlo > n + 1:
                break
            spl[k] = jlo
        else:
            if jhi < spl[k - 1]:
                break
            spl[k] = jhi
    return np.array(spl_lo if flip else spl_hi, dtype=np.int64)
