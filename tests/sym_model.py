"""Pure-Python statement of the symmetric cost family, written from the definitions and from the reference's loops; it shares no
code with the device kernels or with the host mirror's marshalling.

  dianet(j, j') = |rows(A[:, j:j'-1]) united with {j .. j'-1}|          (test_SparseColorArrays.jl:11)
  selfpin(j, j') = nnz(A[j:j'-1, j:j'-1])                                (test_SparseColorArrays.jl:10)
  the three cost formulas, left to right in Int64 (wrapping) / float64    (SymmetricConnectivityCosts.jl:19, :47-55,
                                                                          MonotonizedSymmetricConnectivityCosts.jl:33, :107-113,
                                                                          SymmetricEdgeCutCosts.jl:18, :37-43)
  the literal K-layer DP (through tests/brute.py's layer), the literal BisectCost chain (BisectCostBottleneckSplitter.jl:6-63),
  the lazy probe_init / probe loop (LazyBisectCostBottleneckSplitter.jl:260-388), both bound_stripe forms (:35-66).

Tables are indexed by 0-based boundaries: T[p, r] is the count of the columns [p, r), p = j - 1, r = j' - 1."""
import math

import numpy as np

import brute


def _dense(A):
    D = np.zeros((A.m, A.n), dtype=bool)
    for j in range(A.n):
        D[A.rowval[A.colptr[j] - 1:A.colptr[j + 1] - 1] - 1, j] = True
    return D


def dianet_table(A):
    n = A.n
    D = _dense(A) | np.eye(n, dtype=bool)            # the diagonal added: a row j is a net of every range that holds column j
    T = np.zeros((n + 1, n + 1), dtype=np.int64)
    for p in range(n + 1):
        seen = np.zeros(n, bool)
        for r in range(p + 1, n + 1):
            seen |= D[:, r - 1]
            T[p, r] = seen.sum()
    return T


def selfpin_table(A):
    n = A.n
    D = _dense(A).astype(np.int64)
    S = np.zeros((n + 1, n + 1), dtype=np.int64)     # 2-d prefix sums
    S[1:, 1:] = D.cumsum(0).cumsum(1)
    T = np.zeros((n + 1, n + 1), dtype=np.int64)
    for p in range(n + 1):
        for r in range(p, n + 1):
            T[p, r] = S[r, r] - S[p, r] - S[r, p] + S[p, p]
    return T


def net_table(A):
    return brute.net_table(A)


def overpos(A, delta):
    deg = np.diff(A.colptr).astype(np.int64)
    return np.concatenate([[0], np.cumsum(np.maximum(deg - int(delta), 0))]).astype(np.int64)


class Tables:
    """the count tables of one pattern, computed once and shared"""

    def __init__(self, A):
        self.A = A
        self.pos = (A.colptr - 1).astype(np.int64)
        self._t = {}

    def get(self, name):
        if name not in self._t:
            self._t[name] = {"net": net_table, "dianet": dianet_table, "selfpin": selfpin_table}[name](self.A)
        return self._t[name]


def _is_int_model(mdl):
    return all(isinstance(v, (int, np.integer)) for v in mdl._params()) and \
        (getattr(mdl, "alpha_k", None) is None or all(isinstance(v, (int, np.integer)) for v in mdl.alpha_k))


def _acc(dt, alpha, terms):
    """alpha + c1*b1 + c2*b2 + ... left to right; Int64 wraps, float64 converts every count once"""
    if dt is np.int64:
        with np.errstate(over="ignore"):
            F = np.full(terms[0][0].shape, np.int64(alpha), dtype=np.int64)
            for c, b in terms:
                F = F + c.astype(np.int64) * np.int64(b)
        return F
    F = np.full(terms[0][0].shape, float(alpha), dtype=np.float64)
    for c, b in terms:
        F = F + c.astype(np.float64) * float(b)
    return F


def cost_table(T, mdl, k=None):
    """F[p, r] = f(j, j', k) of the model for all p <= r (the lower triangle is zeroed)"""
    A = T.A
    n = A.n
    P, R = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    nv = (R - P).astype(np.int64)
    w = T.pos[R] - T.pos[P]
    dt = np.int64 if _is_int_model(mdl) else np.float64
    name = type(mdl).__name__
    ak = getattr(mdl, "alpha_k", None)
    alpha = mdl.alpha if ak is None or k is None else ak[k - 1]
    if name == "AffineSymmetricConnectivityModel":
        d = T.get("net")
        rem = T.get("dianet") - nv
        loc = d - rem
        F = _acc(dt, alpha, [(nv, mdl.beta_vertex), (w, mdl.beta_pin), (loc, mdl.beta_local_net), (rem, mdl.beta_remote_net)])
    elif name == "AffineMonotonizedSymmetricConnectivityModel":
        op = overpos(A, mdl.delta_pins)
        F = _acc(dt, alpha, [(nv, mdl.beta_vertex), (op[R] - op[P], mdl.beta_over_pin), (T.get("dianet"), mdl.beta_dia_net)])
    elif name == "AffineSymmetricEdgeCutModel":
        l = T.get("selfpin")
        F = _acc(dt, alpha, [(nv, mdl.beta_vertex), (l, mdl.beta_self_pin), (w - l, mdl.beta_cut_pin)])
    else:
        raise TypeError(name)
    return np.triu(F)


def dp_partition(T, mdl, K, combine, order="splitter"):
    """the literal DP of DynamicSplitter.jl:15-50 (ties: the largest j); combine "sum" | "max"; the chunker order calls the cost
    without the part index (DynamicSplitter.jl:64).  -> (spl 1-based, objective)"""
    n = T.A.n
    Fk = lambda k: cost_table(T, mdl, k if order == "splitter" else None)
    F1 = Fk(1)
    cst = F1[0, :].copy()
    ptrs = [np.zeros(n + 1, dtype=np.int64)]
    same_F = getattr(mdl, "alpha_k", None) is None or order != "splitter"
    for k in range(2, K + 1):
        F = F1 if same_F else Fk(k)
        if combine == "sum":
            with np.errstate(over="ignore"):
                cst, ptr = brute.layer(cst, F)
        else:
            new = np.zeros_like(cst); ptr = np.zeros(n + 1, dtype=np.int64)
            for r in range(n + 1):
                v = np.maximum(cst[:r + 1], F[:r + 1, r])
                i = v.size - 1 - int(np.argmin(v[::-1]))
                new[r] = v[i]; ptr[r] = i
            cst = new
        ptrs.append(ptr)
    spl = [0] * (K + 1)
    at = n
    spl[K] = n + 1
    for k in range(K, 0, -1):
        at = int(ptrs[k - 1][at])
        spl[k - 1] = at + 1
    return np.array(spl, dtype=np.int64), cst[n]


def objective(T, mdl, spl, combine):
    vals = [cost_table(T, mdl, k + 1)[spl[k] - 1, spl[k + 1] - 1] for k in range(len(spl) - 1)]
    if combine == "sum":
        with np.errstate(over="ignore"):
            return np.sum(np.array(vals))
    return max(vals)


# ---------------------------------------------------------------- bound_stripe, both forms
def bound_stripe_model(A, K, mdl):
    """MonotonizedSymmetricConnectivityCosts.jl:50-66"""
    assert mdl.beta_vertex >= 0 and mdl.beta_over_pin >= 0 and mdl.beta_dia_net >= 0 and A.m == A.n
    nop = int(overpos(A, mdl.delta_pins)[-1])
    c_hi = mdl.alpha + mdl.beta_vertex * A.n + mdl.beta_over_pin * nop + mdl.beta_dia_net * A.m
    c_lo = mdl.alpha + math.floor((c_hi - mdl.alpha) / K) if not _is_int_model(mdl) else mdl.alpha + (c_hi - mdl.alpha) // K
    return c_lo, c_hi


def bound_stripe_oracle(T, K, mdl):
    """:35-46: c_hi = ocl(1, n + 1)"""
    c_hi = cost_table(T, mdl)[0, T.A.n].item()
    c_lo = mdl.alpha + math.floor((c_hi - mdl.alpha) / K) if not _is_int_model(mdl) else mdl.alpha + (c_hi - mdl.alpha) // K
    return c_lo, c_hi


def bound_stripe_funky(T, K, mdl):
    """test_Partitioners.jl:36-41 (per-part alpha)"""
    fmax = max(cost_table(T, mdl, k)[0, T.A.n].item() for k in range(1, K + 1))
    args = (min(mdl.alpha_k[:K]), max(mdl.alpha_k[:K]), fmax)
    return min(args), max(args)


def bounds(T, K, mdl):
    return bound_stripe_funky(T, K, mdl) if getattr(mdl, "alpha_k", None) is not None else bound_stripe_model(T.A, K, mdl)


# ---------------------------------------------------------------- BisectCostBottleneckSplitter.jl:6-63 (no flip)
def bisect_cost(T, K, mdl, eps, c_lo=None, c_hi=None):
    n = T.A.n
    Fs = {}

    def f(j, jp, k):
        kk = k if getattr(mdl, "alpha_k", None) is not None else None
        if kk not in Fs:
            Fs[kk] = cost_table(T, mdl, kk)
        return Fs[kk][j - 1, jp - 1]

    def search(j, lo, hi, k, c):                       # the largest j' in [lo, hi] found by bisection with f(j, j', k) <= c
        lo = max(j, lo)
        while lo <= hi:
            mid = (lo + hi) >> 1
            if f(j, mid, k) <= c:
                lo = mid + 1
            else:
                hi = mid - 1
        return hi
    if c_lo is None:
        c_lo, c_hi = bounds(T, K, mdl)
    c_lo, c_hi = c_lo / 1, c_hi / 1
    spl_lo = [1] * (K + 1); spl_hi = [n + 1] * (K + 1); spl = [0] * (K + 1)
    spl_lo[K] = n + 1; spl_hi[0] = 1; spl[0] = 1; spl[K] = n + 1
    probes = 0
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        spl[0] = 1
        chk = True
        for k in range(1, K):
            j = spl[k - 1]
            rr = search(j, spl_lo[k], spl_hi[k], k, c)
            spl[k] = rr
            if rr < j:
                chk = False
                for t in range(k + 1, K + 1):
                    spl[t - 1] = j
                break
        feas = chk and f(spl[K - 1], spl[K], K) <= c
        if feas:
            c_hi = c; spl_hi = list(spl)
        else:
            c_lo = c; spl_lo = list(spl)
    return np.array(spl_hi, dtype=np.int64), probes


# ---------------------------------------------------------------- BisectIndexBottleneckSplitter.jl:5-83 (no flip)
def bisect_index(T, K, mdl):
    """-> (spl_hi 1-based, number of probes).  c_lo / c_hi start as the bounds ./ 1 and become cost values (:60, :64); the
    comparisons are exact (Python compares ints with floats exactly, as Julia does)."""
    n = T.A.n
    Fs = {}

    def f(j, jp, k):
        kk = k if getattr(mdl, "alpha_k", None) is not None else None
        if kk not in Fs:
            Fs[kk] = cost_table(T, mdl, kk)
        return Fs[kk][j - 1, jp - 1].item()

    def search(j, lo, hi, k, c):
        lo = max(j, lo)
        while lo <= hi:
            mid = (lo + hi) >> 1
            if f(j, mid, k) <= c:
                lo = mid + 1
            else:
                hi = mid - 1
        return hi
    c_lo, c_hi = bounds(T, K, mdl)
    c_lo, c_hi = c_lo / 1, c_hi / 1
    spl_lo = [1] * (K + 1); spl_hi = [n + 1] * (K + 1); spl = [0] * (K + 1)
    spl_lo[K] = n + 1; spl_hi[0] = 1; spl[0] = 1; spl[K] = n + 1
    probes = 0
    for k in range(1, K + 1):
        jhi = spl_hi[k]
        jlo = max(spl[k - 1], spl_lo[k])
        while jlo <= jhi:
            jp = (jlo + jhi) >> 1
            c = f(spl[k - 1], jp, k)
            if c_lo <= c < c_hi:
                probes += 1
                chk = True
                spl[k] = jp
                for kk in range(k + 1, K):
                    j = spl[kk - 1]
                    rr = search(j, spl_lo[kk], spl_hi[kk], kk, c)
                    spl[kk] = rr
                    if rr < j:
                        chk = False
                        for t in range(kk + 1, K + 1):
                            spl[t - 1] = j
                        break
                if chk and f(spl[K - 1], spl[K], K) <= c:
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
    return np.array(spl_hi, dtype=np.int64), probes


# ---------------------------------------------------------------- LazyBisectCostBottleneckSplitter.jl:260-388
def lazy_bisect(A, K, mdl, eps):
    """-> (spl_hi 1-based, number of probes).  The loop is the reference's, statement for statement."""
    n = A.n
    colptr, rowval = A.colptr, A.rowval
    ak = getattr(mdl, "alpha_k", None)

    def f(nv, npins, nd, k):
        a = mdl.alpha if ak is None else ak[k - 1]
        return a + nv * mdl.beta_vertex + npins * mdl.beta_over_pin + nd * mdl.beta_dia_net
    delta = int(mdl.delta_pins)
    deg = [int(colptr[j + 1] - colptr[j]) for j in range(n)]
    spl = [0] * (K + 1); spl[0] = 1
    spl_hi = [n + 1] * (K + 1); spl_hi[0] = 1
    hst = [0] * (n + 1); dia = [0] * (n + 1); cch = [0] * (A.nnz + 1)

    def probe_init(c):
        spl[0] = 1
        j = 1; k = 1
        nv = npins = nd = 0
        for jp in range(1, n + 1):
            nv += 1
            npins += max(deg[jp - 1] - delta, 0)
            for q in range(int(colptr[jp - 1]), int(colptr[jp])):
                i = int(rowval[q - 1])
                if hst[i] < j:
                    nd += 1
                cch[q] = hst[i]
                hst[i] = jp
            if hst[jp] < j:
                nd += 1
            dia[jp] = hst[jp]
            hst[jp] = jp
            while k < K and f(nv, npins, nd, k) > c:
                spl[k] = jp
                j = jp
                k += 1
                nv = 1
                npins = max(deg[jp - 1] - delta, 0)
                nd = deg[jp - 1] + (1 if dia[jp] < jp else 0)
        res = k < K or f(nv, npins, nd, K) <= c
        while k <= K:
            spl[k] = n + 1
            k += 1
        return res

    def probe(c):
        spl[0] = 1
        j = 1; k = 1
        nv = npins = nd = 0
        for jp in range(1, n + 1):
            nv += 1
            npins += max(deg[jp - 1] - delta, 0)
            for q in range(int(colptr[jp - 1]), int(colptr[jp])):
                if cch[q] < j:
                    nd += 1
            if dia[jp] < j:
                nd += 1
            while f(nv, npins, nd, k) > c:
                if k == K:
                    return False
                spl[k] = jp
                j = jp
                k += 1
                nv = 1
                npins = max(deg[jp - 1] - delta, 0)
                nd = deg[jp - 1] + (1 if dia[jp] < jp else 0)
        while k <= K:
            spl[k] = n + 1
            k += 1
        return True
    T = None
    if ak is not None:
        T = Tables(A)
        c_lo, c_hi = bound_stripe_funky(T, K, mdl)
    else:
        c_lo, c_hi = bound_stripe_model(A, K, mdl)
    c_lo, c_hi = c_lo / 1, c_hi / 1
    for k in range(1, K + 1):
        c_lo = max(c_lo, f(0, 0, 0, k))
    probes = 0
    if c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        if probe_init(c):
            c_hi = c; spl_hi[:] = spl
        else:
            c_lo = c
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        if probe(c):
            c_hi = c; spl_hi[:] = spl
        else:
            c_lo = c
    return np.array(spl_hi, dtype=np.int64), probes


# ---------------------------------------------------------------- rows and columns of the tables without a dense table
class Sym:
    """f(j, j', k) of one symmetric model along a row (j fixed) or a column (j' fixed) of its cost table, and the three counts in
    the same two forms, from the entry list alone: any n.  One stable sort of the entries by row gives every entry the previous
    and the next column that holds its row; a call then reads the entries of its window's columns once, O(nnz of the window +
    its width).  0-based boundaries inside: p = j - 1, r = j' - 1, the part is the columns [p, r).

      net(p, r)      row i counts iff its last column below r is >= p (fixed r), iff its first column >= p is < r (fixed p)
      dianet(p, r)   row i counts iff max(last column < r that holds i, i if i < r) >= p: the diagonal joins the last column.
                     For a fixed p: iff min(first column >= p that holds i, i if i >= p) < r
      selfpin(p, r)  the entries (i, c) with min(i, c) >= p and max(i, c) < r

    so for a fixed end every count is one bincount of a key per row (or entry) and one cumulative sum, reversed where the fixed
    end is r.  The element type, the operand order and the alpha_k rule are cost_table's."""

    def __init__(self, A, mdl=None):
        assert A.m == A.n
        self.A, self.mdl, self.n = A, mdl, A.n
        self.pos = (np.asarray(A.colptr, dtype=np.int64) - 1)
        self.rows = np.asarray(A.rowval, dtype=np.int64) - 1
        self.cols = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(self.pos))
        nnz, n = self.rows.size, A.n
        order = np.argsort(self.rows, kind="stable")               # by (row, column): columns ascend in storage order
        rs, cs = self.rows[order], self.cols[order]
        same = rs[1:] == rs[:-1]
        self.prev = np.full(nnz, -1, dtype=np.int64); self.prev[order[1:][same]] = cs[:-1][same]
        self.next = np.full(nnz, n, dtype=np.int64); self.next[order[:-1][same]] = cs[1:][same]
        self.op = None if mdl is None or not hasattr(mdl, "delta_pins") else overpos(A, mdl.delta_pins)

    # ---- counts, one fixed end.  *_col(r, p0): p = p0 .. r;  *_row(p, r1): r = p .. r1
    def _window(self, a, b):
        sl = slice(self.pos[a], self.pos[b])
        return self.rows[sl], self.cols[sl], self.prev[sl], self.next[sl]

    @staticmethod
    def _at_least(keys, lo, hi):
        """out[t - lo] = #{keys >= t} for t = lo .. hi, keys in [lo, hi)"""
        h = np.bincount(keys - lo, minlength=hi - lo + 1)
        return np.cumsum(h[::-1])[::-1].astype(np.int64)

    @staticmethod
    def _below(keys, lo, hi):
        """out[t - lo] = #{keys < t} for t = lo .. hi, keys in [lo, hi)"""
        return np.concatenate([[0], np.cumsum(np.bincount(keys - lo, minlength=hi - lo))]).astype(np.int64)

    def net_col(self, r, p0=0):
        i, c, _, nx = self._window(p0, r)
        return self._at_least(c[nx >= r], p0, r)

    def net_row(self, p, r1=None):
        r1 = self.n if r1 is None else r1
        i, c, pv, _ = self._window(p, r1)
        return self._below(c[pv < p], p, r1)

    def dianet_col(self, r, p0=0):
        i, c, _, nx = self._window(p0, r)
        last = nx >= r                                             # the last entry of its row below column r: one per row
        i, c = i[last], c[last]
        key = np.arange(p0, r, dtype=np.int64)                     # rows p0 .. r - 1: at least their own diagonal position
        inside = (i >= p0) & (i < r)
        key[i[inside] - p0] = np.maximum(i[inside], c[inside])
        return self._at_least(np.concatenate([key, c[~inside]]), p0, r)

    def dianet_row(self, p, r1=None):
        r1 = self.n if r1 is None else r1
        i, c, pv, _ = self._window(p, r1)
        first = pv < p
        i, c = i[first], c[first]
        key = np.arange(p, r1, dtype=np.int64)
        inside = (i >= p) & (i < r1)
        key[i[inside] - p] = np.minimum(i[inside], c[inside])
        return self._below(np.concatenate([key, c[~inside]]), p, r1)

    def selfpin_col(self, r, p0=0):
        i, c, _, _ = self._window(p0, r)
        ok = (i >= p0) & (i < r)
        return self._at_least(np.minimum(i[ok], c[ok]), p0, r)

    def selfpin_row(self, p, r1=None):
        r1 = self.n if r1 is None else r1
        i, c, _, _ = self._window(p, r1)
        ok = (i >= p) & (i < r1)
        return self._below(np.maximum(i[ok], c[ok]), p, r1)

    # ---- 1-based forms of the library's counters: one fixed end, all other ends
    def count_column(self, name, jp, frm=1):
        """count(j, jp) for j = frm .. jp"""
        return getattr(self, name + "_col")(jp - 1, frm - 1)

    def count_row(self, name, j, upto=None):
        """count(j, j') for j' = j .. upto"""
        return getattr(self, name + "_row")(j - 1, None if upto is None else upto - 1)

    # ---- costs
    def _cost(self, k, nv, lo, hi, count):
        mdl = self.mdl
        dt = np.int64 if _is_int_model(mdl) else np.float64
        name = type(mdl).__name__
        ak = getattr(mdl, "alpha_k", None)
        alpha = mdl.alpha if ak is None or k is None else ak[k - 1]
        w = self.pos[hi] - self.pos[lo]
        if name == "AffineSymmetricConnectivityModel":
            rem = count("dianet") - nv
            loc = count("net") - rem
            return _acc(dt, alpha, [(nv, mdl.beta_vertex), (w, mdl.beta_pin), (loc, mdl.beta_local_net), (rem, mdl.beta_remote_net)])
        if name == "AffineMonotonizedSymmetricConnectivityModel":
            return _acc(dt, alpha, [(nv, mdl.beta_vertex), (self.op[hi] - self.op[lo], mdl.beta_over_pin), (count("dianet"), mdl.beta_dia_net)])
        if name == "AffineSymmetricEdgeCutModel":
            l = count("selfpin")
            return _acc(dt, alpha, [(nv, mdl.beta_vertex), (l, mdl.beta_self_pin), (w - l, mdl.beta_cut_pin)])
        raise TypeError(name)

    def row(self, j, k=None, upto=None):
        """f(j, j', k) for j' = j .. upto (n + 1 by default)"""
        p, r1 = j - 1, (self.n if upto is None else upto - 1)
        t = np.arange(p, r1 + 1, dtype=np.int64)
        return self._cost(k, t - p, p, t, lambda name: getattr(self, name + "_row")(p, r1))

    def column(self, jp, k=None, frm=1):
        """f(j, j', k) for j = frm .. j'"""
        r, p0 = jp - 1, frm - 1
        t = np.arange(p0, r + 1, dtype=np.int64)
        return self._cost(k, r - t, t, r, lambda name: getattr(self, name + "_col")(r, p0))
