"""Pure-Python statement of partition_stripe(A, K, LazyBisectCostBottleneckSplitter(f::AbstractPrimaryConnectivityModel, eps), Pi)
(LazyBisectCostBottleneckSplitter.jl:390-483), written from the reference's text: the hst / lcl / drt arrays, the probe with its
split loop, the two bound_stripe forms and the plain bisection.  It shares no code with the device kernel, which counts from the
link array instead.

  bound_stripe_model   PrimaryConnectivityCosts.jl:43-51 over ConnectivityCosts.jl:25-35 (bound_stripe(A, K, Pi, f) drops Pi,
                       Costs.jl:17-19)
  bound_stripe_funky   test_Partitioners.jl:43-48 (the per-part alpha model of the reference's tests)
  lazy_bisect          :390-483 -> (spl_hi 1-based, number of probes)
  cost_tables / bottleneck_optimum   the primary cost of every column range from the definition (PrimaryConnectivityCosts.jl:94-125)
                       and the brute-force K-part bottleneck optimum over them
"""
import math

import numpy as np

import brute


def _is_int_model(mdl):
    return all(isinstance(v, (int, np.integer)) for v in mdl._params()) and \
        (getattr(mdl, "alpha_k", None) is None or all(isinstance(v, (int, np.integer)) for v in mdl.alpha_k))


def _asg(Pi, m):
    """convert(MapPartition, Pi).asg (1-based part of every row)"""
    if hasattr(Pi, "asg"):
        asg = [int(v) for v in Pi.asg]
    else:
        asg = [0] * m
        for k in range(1, Pi.K + 1):
            for i in range(int(Pi.spl[k - 1]), int(Pi.spl[k])):
                asg[i - 1] = k
    assert len(asg) == m
    return asg


def _f(mdl):
    ak = getattr(mdl, "alpha_k", None)
    flt = not _is_int_model(mdl)

    def f(nv, npins, nl, nr, k):                    # left to right, one Int -> Float conversion per product
        a = mdl.alpha if ak is None else ak[k - 1]
        if flt:
            return float(a) + float(nv) * float(mdl.beta_vertex) + float(npins) * float(mdl.beta_pin) + \
                float(nl) * float(mdl.beta_local_net) + float(nr) * float(mdl.beta_remote_net)
        return int(a) + nv * int(mdl.beta_vertex) + npins * int(mdl.beta_pin) + nl * int(mdl.beta_local_net) + nr * int(mdl.beta_remote_net)
    return f


def _nets(A):
    return len(set(int(i) for i in A.rowval))       # net(1, n + 1): the rows that hold a nonzero


def _fld(x, K, flt):
    return math.floor(x / K) if flt else x // K


def bound_stripe_model(A, K, mdl):
    """PrimaryConnectivityCosts.jl:43-51: c_hi of the connectivity model with max(b_local, b_remote), c_lo of the one with the min"""
    assert mdl.beta_vertex >= 0 and mdl.beta_pin >= 0 and mdl.beta_local_net >= 0 and mdl.beta_remote_net >= 0
    flt = not _is_int_model(mdl)
    cv = float if flt else int
    d = _nets(A)

    def conn(beta_net):                               # ConnectivityCosts.jl:25-35
        c_hi = cv(mdl.alpha) + cv(A.n) * cv(mdl.beta_vertex) + cv(A.nnz) * cv(mdl.beta_pin) + cv(d) * cv(beta_net)
        return cv(mdl.alpha) + _fld(c_hi - cv(mdl.alpha), K, flt), c_hi
    _, c_hi = conn(max(mdl.beta_local_net, mdl.beta_remote_net))
    c_lo, _ = conn(min(mdl.beta_local_net, mdl.beta_remote_net))
    return c_lo, c_hi


def bound_stripe_funky(A, K, mdl, Pi):
    """test_Partitioners.jl:43-48: (minimum, maximum) of (minimum(alpha), maximum(alpha), maximum_k ocl(1, n + 1, k))"""
    f = _f(mdl)
    asg = _asg(Pi, A.m)
    rows = sorted(set(int(i) for i in A.rowval))
    fmax = None
    for k in range(1, K + 1):
        l = sum(1 for i in rows if asg[i - 1] == k)
        v = f(A.n, A.nnz, l, len(rows) - l, k)
        fmax = v if fmax is None else max(fmax, v)
    args = (min(mdl.alpha_k), max(mdl.alpha_k), fmax)
    return min(args), max(args)


def lazy_bisect(A, K, mdl, Pi, eps, trace=None):
    """-> (spl_hi 1-based, number of probes).  The loop is the reference's, statement for statement.  trace: a list that receives
    ("again", j', pass) for every further pass of the split loop (:440) at one column and ("fail", j', pass) where it ends the probe."""
    m, n = A.m, A.n
    colptr, rowval = [int(v) for v in A.colptr], [int(v) for v in A.rowval]
    f = _f(mdl)
    asg = _asg(Pi, m)                                 # Pi_map = convert(MapPartition, Pi)
    assert Pi.K <= K                                  # lcl / drt have K slots

    spl = [0] * (K + 1); spl[0] = 1
    spl_hi = [n + 1] * (K + 1); spl_hi[0] = 1
    hst = [0] * (m + 1); lcl = [0] * (K + 1); drt = [0] * (K + 1)

    def probe(c):
        for i in range(m + 1):
            hst[i] = 0
        for k in range(K + 1):
            drt[k] = 0
        spl[0] = 1
        j = 1; k = 1
        nv = npins = nl = xc = 0
        for jp in range(1, n + 1):
            nv += 1
            npins += colptr[jp] - colptr[jp - 1]
            for q in range(colptr[jp - 1], colptr[jp]):
                i = rowval[q - 1]
                _k = asg[i - 1]
                if drt[_k] < jp:
                    lcl[_k] = 0
                lcl[_k] += 1
                drt[_k] = jp
                if hst[i] < j:
                    if _k == k:
                        nl += 1
                    else:
                        xc += 1
                hst[i] = jp
            passes = 0
            while f(nv, npins, nl, xc, k) > c:
                if trace is not None and (passes >= 1 or k == K):   # (no statement of the reference: what the split loop did, for tests)
                    trace.append(("fail" if k == K else "again", jp, passes + 1))
                if k == K:
                    return False
                passes += 1
                spl[k] = jp
                j = jp
                k += 1
                nv = 1
                npins = colptr[jp] - colptr[jp - 1]
                nl = 0
                xc = colptr[jp] - colptr[jp - 1]
                if drt[k] == jp:
                    nl += lcl[k]
                    xc -= lcl[k]
        while k <= K:
            spl[k] = n + 1
            k += 1
        return True

    if getattr(mdl, "alpha_k", None) is not None:
        c_lo, c_hi = bound_stripe_funky(A, K, mdl, Pi)
    else:
        c_lo, c_hi = bound_stripe_model(A, K, mdl)
    c_lo, c_hi = c_lo / 1, c_hi / 1
    for k in range(1, K + 1):
        c_lo = max(c_lo, float(f(0, 0, 0, 0, k)))
    probes = 0
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        chk = probe(c)
        if chk and spl[K] == n + 1:
            c_hi = c; spl_hi[:] = spl
        else:
            c_lo = c
    return np.array(spl_hi, dtype=np.int64), probes


# ---------------------------------------------------------------- the costs from the definition, and the optimum over them
def cost_tables(A, mdl, Pi, K):
    """[F_k[p, r] for k = 1 .. K]: the primary cost of the columns [p, r) as part k (0-based boundaries).  The nets are
    brute.net_table's; the local ones are the nets of the pattern restricted to the rows part k owns (the same definition)."""
    from util import cp
    n = A.n
    flt = not _is_int_model(mdl)
    dt = np.float64 if flt else np.int64
    ak = getattr(mdl, "alpha_k", None)
    asg = np.array(_asg(Pi, A.m), dtype=np.int64)
    pos = (A.colptr - 1).astype(np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.colptr))
    P, R = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    nv = (R - P).astype(dt)
    npins = (pos[R] - pos[P]).astype(dt)
    NT = brute.net_table(A)
    out = []
    for k in range(1, K + 1):
        own = asg[A.rowval - 1] == k if A.nnz else np.zeros(0, dtype=bool)
        colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols[own], minlength=n))]).astype(np.int64)
        LT = brute.net_table(cp.SparseMatrixCSC(A.m, n, colptr, A.rowval[own]))
        a = mdl.alpha if ak is None else ak[k - 1]
        F = np.full((n + 1, n + 1), a, dtype=dt)
        F = F + nv * dt(mdl.beta_vertex)
        F = F + npins * dt(mdl.beta_pin)
        F = F + LT.astype(dt) * dt(mdl.beta_local_net)
        F = F + (NT - LT).astype(dt) * dt(mdl.beta_remote_net)
        out.append(F)
    return out


def bottleneck_value(Fs, spl):
    return max(Fs[k][int(spl[k]) - 1, int(spl[k + 1]) - 1] for k in range(len(spl) - 1))


def bottleneck_optimum(Fs, K):
    """min over K consecutive (possibly empty) parts of the largest part cost, part k costed by Fs[k - 1]"""
    n1 = Fs[0].shape[0]
    cst = Fs[0][0, :].copy()
    for k in range(2, K + 1):
        F = Fs[k - 1]
        cst = np.array([np.min(np.maximum(cst[:r + 1], F[:r + 1, r])) for r in range(n1)])
    return cst[n1 - 1].item()
