"""Pure-Python statement of partition_stripe(A, K, LazyFlipBisectCostBottleneckSplitter(f, eps), [Pi])
(LazyBisectCostBottleneckSplitter.jl:72-138), written from the reference's text: the probe with its leading loop and its split
loop, the plain bisection between bound_stripe's bounds, and stepwise cost oracles that cost O(nnz) a probe.  It shares no code
with the device kernels, which count from the link array instead.

  oracles   connectivity (ConnectivityCosts.jl:20) and primary (PrimaryConnectivityCosts.jl:20): an hst array, the last column that
            held every row; secondary (SecondaryConnectivityCosts.jl:82-89): per part of Pi the last column that held one of its rows
  bounds    ConnectivityCosts.jl:25-35, PrimaryConnectivityCosts.jl:43-51, SecondaryConnectivityCosts.jl:42-61 and the per-part alpha
            ("Funky") forms of test_Partitioners.jl:36-48
  lazy_flip_bisect   :79-137 -> (spl_hi 1-based, number of probes)
  cost_tables        the cost of every column range as part k from the definitions, for the brute-force optimum
"""
import math

import numpy as np

import brute

CONNECTIVITY, PRIMARY, SECONDARY = 2, 8, 9
MAX_PROBES = 4096                                     # past this the device entry gives up as well (the reference would go on)


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


def _affine(mdl):
    """mdl(counts..., k): alpha[k] + sum of count * beta, left to right, one Int -> Float conversion per product"""
    ak = getattr(mdl, "alpha_k", None)
    cv = int if _is_int_model(mdl) else float
    betas = [cv(b) for b in mdl._params()[1:]]

    def f(counts, k):
        v = cv(mdl.alpha if ak is None else ak[k - 1])
        for cnt, b in zip(counts, betas):
            v = v + cv(cnt) * b
        return v
    return f


class _Stepper:
    """f(j, j', k) of the open part while j' grows by one column at a time; restart(j) opens an empty range [j, j)"""

    def __init__(self, A, mdl, Pi):
        self.A, self.kind = A, mdl.kind
        self.colptr, self.rowval = [int(v) for v in A.colptr], [int(v) for v in A.rowval]
        self.f = _affine(mdl)
        if self.kind != CONNECTIVITY:
            self.asg = _asg(Pi, A.m)
        if self.kind == SECONDARY:                    # w, d of :84-85 and |Pi_k| for every part
            spl = [int(v) for v in Pi.spl]
            rowdeg = np.bincount(np.asarray(A.rowval, dtype=np.int64) - 1, minlength=A.m)
            rpos = np.concatenate([[0], np.cumsum(rowdeg)])
            self.nvk = [0] + [spl[k] - spl[k - 1] for k in range(1, Pi.K + 1)]
            self.npk = [0] + [int(rpos[spl[k] - 1] - rpos[spl[k - 1] - 1]) for k in range(1, Pi.K + 1)]
            self.dk = [0] * (Pi.K + 1)
            seen = [0] * (Pi.K + 1)
            for jp in range(1, A.n + 1):
                for q in range(self.colptr[jp - 1], self.colptr[jp]):
                    p = self.asg[self.rowval[q - 1] - 1]
                    if seen[p] != jp:
                        seen[p] = jp
                        self.dk[p] += 1

    def reset(self):
        self.hst = [0] * (self.A.m + 1)               # last column of every row (connectivity, primary)
        self.seen = [0] * (len(getattr(self, "dk", [0])))   # last column of every part of Pi (secondary)
        self.restart(1)

    def restart(self, j):
        self.j = j
        self.nv = self.np = self.a = self.b = 0       # a: nets / local nets / l, b: remote nets

    def add_column(self, c, k):
        """extend [j, c) to [j, c + 1)"""
        self.nv += 1
        self.np += self.colptr[c] - self.colptr[c - 1]
        for q in range(self.colptr[c - 1], self.colptr[c]):
            i = self.rowval[q - 1]
            if self.kind == SECONDARY:
                p = self.asg[i - 1]
                if self.seen[p] != c:
                    self.seen[p] = c
                    if p == k:
                        self.a += 1
                continue
            if self.hst[i] < self.j:
                if self.kind == CONNECTIVITY or self.asg[i - 1] == k:
                    self.a += 1
                else:
                    self.b += 1
            self.hst[i] = c

    def cost(self, k):
        if self.kind == CONNECTIVITY:
            return self.f((self.nv, self.np, self.a), k)
        if self.kind == PRIMARY:
            return self.f((self.nv, self.np, self.a, self.b), k)
        return self.f((self.nvk[k], self.npk[k], self.a, self.dk[k] - self.a), k)


# ---------------------------------------------------------------- bounds
def _fld(x, K, flt):
    return math.floor(x / K) if flt else x // K


def _nets(A):
    return len(set(int(i) for i in A.rowval))


def bound_stripe(A, K, mdl, Pi=None):
    """bound_stripe(A, K, [Pi], ocl) as the call at :125 dispatches it"""
    flt = not _is_int_model(mdl)
    cv = float if flt else int
    f = _affine(mdl)
    if mdl.kind == SECONDARY:                         # SecondaryConnectivityCosts.jl:42-61
        assert mdl.beta_vertex >= 0 and mdl.beta_pin >= 0 and mdl.beta_local_net >= 0 and mdl.beta_remote_net >= 0
        st = _Stepper(A, mdl, Pi)
        c_lo = c_hi = 0
        for k in range(1, K + 1):
            work = cv(mdl.alpha) + cv(st.nvk[k]) * cv(mdl.beta_vertex) + cv(st.npk[k]) * cv(mdl.beta_pin)
            c_lo = max(c_lo, work)
            c_hi = max(c_hi, work + cv(st.dk[k]) * cv(mdl.beta_remote_net))
        return c_lo, c_hi
    if getattr(mdl, "alpha_k", None) is not None:     # test_Partitioners.jl:36-41, :43-48
        rows = sorted(set(int(i) for i in A.rowval))
        if mdl.kind == PRIMARY:
            asg = _asg(Pi, A.m)
            loc = [sum(1 for i in rows if asg[i - 1] == k) for k in range(1, K + 1)]
            fmax = max(f((A.n, A.nnz, loc[k - 1], len(rows) - loc[k - 1]), k) for k in range(1, K + 1))
        else:
            fmax = max(f((A.n, A.nnz, len(rows)), k) for k in range(1, K + 1))
        args = (min(mdl.alpha_k), max(mdl.alpha_k), fmax)
        return min(args), max(args)
    assert all(b >= 0 for b in mdl._params()[1:])

    def conn(beta_net):                               # ConnectivityCosts.jl:25-35
        c_hi = cv(mdl.alpha) + cv(A.n) * cv(mdl.beta_vertex) + cv(A.nnz) * cv(mdl.beta_pin) + cv(_nets(A)) * cv(beta_net)
        return cv(mdl.alpha) + _fld(c_hi - cv(mdl.alpha), K, flt), c_hi
    if mdl.kind == PRIMARY:                           # PrimaryConnectivityCosts.jl:43-51 (Pi is dropped, Costs.jl:17-19)
        return conn(min(mdl.beta_local_net, mdl.beta_remote_net))[0], conn(max(mdl.beta_local_net, mdl.beta_remote_net))[1]
    return conn(mdl.beta_net)


# ---------------------------------------------------------------- the method
def lazy_flip_bisect(A, K, mdl, Pi=None, eps=0.1, trace=None):
    """-> (spl_hi 1-based, number of probes).  The loop is the reference's, statement for statement.  trace: a list that receives,
    per probe, ("lead", number of leading empty parts), ("run", j', number of parts closed at j') for every j' that closed more
    than one part, and the exit taken: ("exit", "lead" | "split" | "fail")."""
    n = A.n
    if mdl.kind == SECONDARY:
        assert hasattr(Pi, "spl") and Pi.K == K       # the oracle indexes Pi.spl[k + 1] for k up to K
    if mdl.kind == PRIMARY:
        assert Pi.K <= K
    st = _Stepper(A, mdl, Pi)
    spl = [0] * (K + 1); spl[0] = 1
    spl_hi = [n + 1] * (K + 1); spl_hi[0] = 1
    note = (lambda *t: trace.append(t)) if trace is not None else (lambda *t: None)

    def probe(c):
        spl[0] = 1
        j = 1; k = 1
        st.reset()
        lead = 0
        while st.cost(k) <= c:                        # f(1, 1, k)
            if k == K:
                spl[K] = n + 1
                note("lead", lead); note("exit", "lead")
                return True
            spl[k] = 1
            k += 1
            lead += 1
        note("lead", lead)
        for jp in range(2, n + 2):
            st.add_column(jp - 1, k)                  # Step(f)(Same(j), Next(j'), Same(k))
            if st.cost(k) <= c:
                closed = 0
                while st.cost(k) <= c:                # f(j, j', k), then f(j', j', k) for the following k
                    if k == K:
                        spl[K] = n + 1
                        if closed > 1:
                            note("run", jp, closed)
                        note("exit", "split")
                        return True
                    spl[k] = jp
                    j = jp
                    k += 1
                    closed += 1
                    st.restart(j)
                if closed > 1:
                    note("run", jp, closed)
        note("exit", "fail")
        return False

    c_lo, c_hi = bound_stripe(A, K, mdl, Pi)
    c_lo, c_hi = c_lo / 1, c_hi / 1
    probes = 0
    while c_lo * (1 + eps) < c_hi:
        c = (c_lo + c_hi) / 2
        probes += 1
        if probes > MAX_PROBES:
            raise RuntimeError("the bisection does not terminate on these bounds")
        if probe(c):
            c_hi = c; spl_hi[:] = spl
        else:
            c_lo = c
    return np.array(spl_hi, dtype=np.int64), probes


# ---------------------------------------------------------------- the costs from the definition, and the optimum over them
def cost_tables(A, mdl, Pi, K):
    """[F_k[p, r] for k = 1 .. K]: the cost of the columns [p, r) as part k (0-based boundaries, p <= r), from tests/brute.py's net
    table (connectivity) and, for the secondary model, the number of columns of [p, r) that hold a row of part k."""
    n = A.n
    dt = np.int64 if _is_int_model(mdl) else np.float64
    ak = getattr(mdl, "alpha_k", None)
    pos = (A.colptr - 1).astype(np.int64)
    P, R = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.colptr))
    out = []
    if mdl.kind == CONNECTIVITY:
        NT = brute.net_table(A)
        for k in range(1, K + 1):
            F = np.full((n + 1, n + 1), mdl.alpha if ak is None else ak[k - 1], dtype=dt)
            F = F + (R - P).astype(dt) * dt(mdl.beta_vertex)
            F = F + (pos[R] - pos[P]).astype(dt) * dt(mdl.beta_pin)
            out.append(F + NT.astype(dt) * dt(mdl.beta_net))
        return out
    assert mdl.kind == SECONDARY
    asg = np.array(_asg(Pi, A.m), dtype=np.int64)
    rowdeg = np.bincount(A.rowval - 1, minlength=A.m)
    for k in range(1, K + 1):
        has = np.zeros(n, dtype=np.int64)
        has[np.unique(cols[asg[A.rowval - 1] == k])] = 1          # columns holding a row of part k
        cum = np.concatenate([[0], np.cumsum(has)])
        l = cum[R] - cum[P]
        F = np.full((n + 1, n + 1), mdl.alpha if ak is None else ak[k - 1], dtype=dt)
        F = F + dt(int((asg == k).sum())) * dt(mdl.beta_vertex)
        F = F + dt(int(rowdeg[asg == k].sum())) * dt(mdl.beta_pin)
        F = F + l.astype(dt) * dt(mdl.beta_local_net)
        out.append(F + (int(has.sum()) - l).astype(dt) * dt(mdl.beta_remote_net))
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
