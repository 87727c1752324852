"""The envelope cost family in pure Python / numpy, restated from the reference's text: the implicit tree and its getindex
(EnvelopeMatrices.jl:10-57), the definition it stands for, the oracle and both compute_objective loops (EnvelopeCosts.jl:66-125),
the model-form bounds (:43-53), the literal K-part DP for both combines with its full cst / ptr tables (DynamicSplitter.jl:15-50),
the literal BisectCost and BisectIndex loops, and the valley search the device runs for the bottleneck objective.

All indices are 1-based as the reference writes them.  Costs are computed in the model's element type, left to right, one
conversion per product; Int64 sums wrap."""
import math

import numpy as np

I64_MAX = np.iinfo(np.int64).max


def cllog2(x):
    """util.jl:6-8 for x >= 1"""
    return (x - 1).bit_length()


def is_int_model(mdl):
    return mdl.dtype == 0


# ---------------------------------------------------------------- the structure
def leaves(A):
    """per column (first stored row, last stored row), (m + 1, 0) for an empty column (EnvelopeMatrices.jl:15-21)"""
    cp_, rv = np.asarray(A.colptr, dtype=np.int64), np.asarray(A.rowval, dtype=np.int64)
    lo = np.full(A.n, A.m + 1, dtype=np.int64); hi = np.zeros(A.n, dtype=np.int64)
    for j in range(A.n):
        if cp_[j] < cp_[j + 1]:
            lo[j] = rv[cp_[j] - 1]; hi[j] = rv[cp_[j + 1] - 2]
    return lo, hi


def build_tree(A):
    """rowenvelope (EnvelopeMatrices.jl:10-33) -> (H, tree) with tree[t] = (lo, hi) of node t, tree[0] unused"""
    m, n = A.m, A.n
    H = cllog2(n)
    tree = [None] * (1 << (H + 1))
    lo, hi = leaves(A)
    for j in range(1, n + 1):
        tree[(1 << H) - 1 + j] = (int(lo[j - 1]), int(hi[j - 1]))
    for j in range((1 << H) + n, (1 << (H + 1))):
        tree[j] = (m + 1, 0)
    for j in range((1 << (H + 1)) - 2, 0, -2):
        (a, b), (c, d) = tree[j], tree[j + 1]
        tree[j >> 1] = (min(a, c), max(b, d))
    return H, tree


def getindex(H, m, tree, j, jp):
    """EnvelopeMatrices.jl:35-57"""
    lo, hi = m + 1, 0
    j = ((1 << H) - 1) + j
    jp = ((1 << H) - 1) + (jp - 1)
    while j <= jp:
        (a, b), (c, d) = tree[j], tree[jp]
        lo, hi = min(lo, a, c), max(hi, b, d)
        j = (j + 1) >> 1
        jp = (jp - 1) >> 1
    return lo, hi


def definition(A, j, jp):
    """extrema of rowval over the columns j : j'-1, (m + 1, 0) if there is none (test_EnvelopeMatrices.jl:12-16)"""
    r = np.asarray(A.rowval)[A.colptr[j - 1] - 1:A.colptr[jp - 1] - 1]
    return (int(r.min()), int(r.max())) if r.size else (A.m + 1, 0)


def span_table(A):
    """D[j - 1, j' - 1] = d(j, j') = max(hi - lo, 0) for 1 <= j <= j' <= n + 1 (0 below the diagonal), from the leaves"""
    n = A.n
    lo, hi = leaves(A)
    D = np.zeros((n + 1, n + 1), dtype=np.int64)
    for j in range(n):
        rl = np.minimum.accumulate(lo[j:]); rh = np.maximum.accumulate(hi[j:])
        D[j, j + 1:] = np.maximum(rh - rl, 0)
    return D


# ---------------------------------------------------------------- the oracle
class Env:
    """f(j, j', k) = alpha_k + (j' - j) b_vertex + (pos[j'] - pos[j]) b_pin + d(j, j') b_net  (EnvelopeCosts.jl:20, :66-73)"""

    def __init__(self, A, mdl, tables=True):
        self.A, self.mdl = A, mdl
        self.dt = np.int64 if is_int_model(mdl) else np.float64
        self.pos = np.asarray(A.colptr, dtype=np.int64)
        self.lo, self.hi = leaves(A)
        self.D = span_table(A) if tables else None
        self._tab = {}

    def alpha(self, k):
        ak = getattr(self.mdl, "alpha_k", None)      # (a part number past the vector takes the scalar, as the library does)
        return self.dt(self.mdl.alpha if ak is None or k is None or k > len(ak) else ak[k - 1])

    def apply(self, k, nv, npins, d):
        """the model on count arrays, left to right in the element type (Int64 wraps)"""
        dt, m = self.dt, self.mdl
        with np.errstate(over="ignore"):
            return ((self.alpha(k) + np.asarray(nv).astype(dt) * dt(m.beta_vertex)) + np.asarray(npins).astype(dt) * dt(m.beta_pin)) \
                + np.asarray(d).astype(dt) * dt(m.beta_net)

    def table(self, k):
        """F[j - 1, j' - 1] = f(j, j', k); entries below the diagonal are not costs"""
        key = self.alpha(k).item()                   # (the part number enters through alpha only)
        if key not in self._tab:
            n = self.A.n
            idx = np.arange(n + 1, dtype=np.int64)
            self._tab[key] = self.apply(k, idx[None, :] - idx[:, None], self.pos[None, :] - self.pos[:, None], self.D)
        return self._tab[key]

    def f(self, j, jp, k):
        if self.D is not None:
            return self.table(k)[j - 1, jp - 1].item()
        return self.column(jp, k)[j - 1].item()

    def row(self, j, k):
        """f(j, j', k) for j' = j .. n + 1 (the prefix extrema of the leaves from j)"""
        n = self.A.n
        lo = np.concatenate([[self.A.m + 1], np.minimum.accumulate(self.lo[j - 1:])])
        hi = np.concatenate([[0], np.maximum.accumulate(self.hi[j - 1:])])
        jp = np.arange(j, n + 2, dtype=np.int64)
        return self.apply(k, jp - j, self.pos[jp - 1] - self.pos[j - 1], np.maximum(hi - lo, 0))

    def column(self, jp, k):
        """f(j, j', k) for j = 1 .. j' (needs no table: the suffix extrema of the leaves below j')"""
        lo = np.concatenate([np.minimum.accumulate(self.lo[:jp - 1][::-1])[::-1], [self.A.m + 1]])
        hi = np.concatenate([np.maximum.accumulate(self.hi[:jp - 1][::-1])[::-1], [0]])
        j = np.arange(1, jp + 1, dtype=np.int64)
        return self.apply(k, jp - j, self.pos[jp - 1] - self.pos[j - 1], np.maximum(hi - lo, 0))


# ---------------------------------------------------------------- compute_objective
def _reduce(E, vals, combine):
    if combine == "max":
        return max(vals)
    acc = np.zeros(1, dtype=E.dt)
    with np.errstate(over="ignore"):
        for v in vals:
            acc = acc + np.array([v], dtype=E.dt)
    return acc[0].item()


def _part_cost(E, cols, k):
    """the inner loop of EnvelopeCosts.jl:81-95 / :107-122 over the columns `cols` (1-based, any order)"""
    A = E.A
    n_pins, lo, hi = 0, A.m + 1, 0
    for j in cols:
        q, qp = int(A.colptr[j - 1]), int(A.colptr[j])
        n_pins += qp - q
        if qp > q:
            lo = min(lo, int(A.rowval[q - 1])); hi = max(hi, int(A.rowval[qp - 2]))
    return E.apply(k, len(cols), n_pins, max(hi - lo, 0)).item()


def objective_split(E, spl, combine):
    """compute_objective(g, A, Pi::SplitPartition, mdl)  EnvelopeCosts.jl:75-98"""
    return _reduce(E, [_part_cost(E, list(range(int(spl[k]), int(spl[k + 1]))), k + 1) for k in range(len(spl) - 1)], combine)


def objective_domain(E, prm, spl, combine):
    """compute_objective(g, A, K, Pi::DomainPartition, mdl)  :100-125 (a MapPartition converts to one, :127-129)"""
    return _reduce(E, [_part_cost(E, [int(prm[s - 1]) for s in range(int(spl[k]), int(spl[k + 1]))], k + 1) for k in range(len(spl) - 1)], combine)


# ---------------------------------------------------------------- bound_stripe, the model form
def bound_stripe(A, K, mdl):
    """EnvelopeCosts.jl:43-53; a pattern without nonzeros has no extrema"""
    assert mdl.beta_vertex >= 0 and mdl.beta_pin >= 0 and mdl.beta_net >= 0
    assert A.nnz > 0
    r = np.asarray(A.rowval)[:A.nnz]
    d = int(r.max()) - int(r.min())
    c_hi = mdl.alpha + mdl.beta_vertex * A.n + mdl.beta_pin * A.nnz + mdl.beta_net * d
    s = mdl.beta_vertex * A.n + mdl.beta_pin * A.nnz + mdl.beta_net * d
    c_lo = mdl.alpha + (s // K if is_int_model(mdl) else math.floor(s / K))
    return c_lo, c_hi


# ---------------------------------------------------------------- the K-part DP
def _typemax(E):
    return I64_MAX if E.dt == np.int64 else np.inf


def _combine(combine, W, F):
    with np.errstate(over="ignore"):
        return W + F if combine == "sum" else np.maximum(W, F)


def dp_literal(E, K, combine):
    """DynamicSplitter.jl:15-50: cst[j', k] = min over j <= j' of g(cst[j, k - 1], f(j, j', k)), the largest j among equals (`<=`
    while j grows); layer K holds row n + 1 only.  -> (spl, cst[(n + 1), K], ptr[(n + 1), K]) with ptr 1-based, 0 / typemax where
    the reference leaves zeros(Ti) / fill(typemax)"""
    n = E.A.n
    cst = np.full((n + 1, K), _typemax(E), dtype=E.dt)
    ptr = np.zeros((n + 1, K), dtype=np.int64)
    cst[:, 0] = E.table(1)[0, :]
    ptr[:, 0] = 1
    for k in range(2, K + 1):
        F, W = E.table(k), cst[:, k - 2]
        for r in range(n if k == K else 0, n + 1):
            v = _combine(combine, W[:r + 1], F[:r + 1, r])
            i = v.size - 1 - int(np.argmin(v[::-1]))
            cst[r, k - 1] = v[i]; ptr[r, k - 1] = i + 1
    return unravel(K, n, ptr), cst, ptr


def dp_valley(E, K):
    """the bottleneck DP as the device searches it: per row the first j with cst[j, k - 1] >= f(j, j', k) (none: j' + 1), the
    minimum at that j or the one before, then the largest j of that value by a second search over the previous layer"""
    n = E.A.n
    cst = np.full((n + 1, K), _typemax(E), dtype=E.dt)
    ptr = np.zeros((n + 1, K), dtype=np.int64)
    cst[:, 0] = E.table(1)[0, :]
    ptr[:, 0] = 1
    for k in range(2, K + 1):
        F, W = E.table(k), cst[:, k - 2]
        for r in range(n if k == K else 0, n + 1):
            lo, hi = 0, r + 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if W[mid] >= F[mid, r]:
                    hi = mid
                else:
                    lo = mid + 1
            ps = lo
            has_r, has_l = ps <= r, ps > 0
            if has_r and (not has_l or W[ps] <= F[ps - 1, r]):
                vr = W[ps]
                lo, hi = ps, r
                while lo < hi:
                    mid = (lo + hi + 1) >> 1
                    if W[mid] <= vr:
                        lo = mid
                    else:
                        hi = mid - 1
                cst[r, k - 1] = vr; ptr[r, k - 1] = lo + 1
            else:
                cst[r, k - 1] = F[ps - 1, r]; ptr[r, k - 1] = ps
    return unravel(K, n, ptr), cst, ptr


def unravel(K, n, ptr):
    """unravel_splits  DynamicSplitter.jl:89-99"""
    spl = np.zeros(K + 1, dtype=np.int64)
    spl[K] = n + 1
    for k in range(K, 0, -1):
        spl[k - 1] = ptr[spl[k] - 1, k - 1]
    return spl


# ---------------------------------------------------------------- the Bisect loops over f(j, j', k)
def _search(f, j, lo, hi, k, c):
    """the largest j' in [max(j, lo), hi] with f(j, j', k) <= c as the binary search finds it; max(j, lo) - 1 if none"""
    lo = max(j, lo)
    while lo <= hi:
        mid = (lo + hi) >> 1
        if f(j, mid, k) <= c:
            lo = mid + 1
        else:
            hi = mid - 1
    return hi


def _chain(f, n, K, spl, spl_lo, spl_hi, k0, c):
    for k in range(k0, K):
        j = spl[k - 1]
        rr = _search(f, j, spl_lo[k], spl_hi[k], k, c)
        spl[k] = rr
        if rr < j:
            for t in range(k, K):
                spl[t] = j
            return False
    return f(spl[K - 1], spl[K], K) <= c


def bisect_cost(f, n, K, eps, c_lo, c_hi):
    """BisectCostBottleneckSplitter.jl:6-63"""
    c_lo, c_hi = c_lo / 1, c_hi / 1
    spl_lo = [1] * (K + 1); spl_hi = [n + 1] * (K + 1); spl = [0] * (K + 1)
    spl_lo[K] = n + 1; spl_hi[0] = 1; spl[0] = 1; spl[K] = n + 1
    probes = 0
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        assert probes <= 4096, "the bisection does not terminate on these bounds"
        spl[0] = 1
        if _chain(f, n, K, spl, spl_lo, spl_hi, 1, c):
            c_hi = c; spl_hi = list(spl)
        else:
            c_lo = c; spl_lo = list(spl)
    return np.array(spl_hi, dtype=np.int64)


def bisect_index(f, n, K, c_lo, c_hi):
    """BisectIndexBottleneckSplitter.jl:5-83"""
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
                if _chain(f, n, K, spl, spl_lo, spl_hi, k + 1, c):
                    c_hi = c; jhi = jp - 1; spl_hi = list(spl)
                else:
                    c_lo = c; jlo = jp + 1; spl_lo = list(spl)
            elif c >= c_hi:
                jhi = jp - 1
            else:
                jlo = jp + 1
        if jhi < spl[k - 1]:
            break
        spl[k] = jhi
    return np.array(spl_hi, dtype=np.int64)
