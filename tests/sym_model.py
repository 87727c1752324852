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
