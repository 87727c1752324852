"""Literal Python restatement of the reference's two map partitioners (src/MagneticPartitioner.jl), loop for loop; it shares no
code with the device kernels.  Where the reference calls Julia's global RNG the draws are arguments:

  magnetic(A, K, Pi, draws)                      :3-20    rand(1:k) -> 1 + u_j % k, rand(colptr[j]:colptr[j+1]-1) -> colptr[j] + u_j % d
  greedy_setup_split(A, adj_A, K, Pi, mdl)       :108-135 the counts of the parts of a SplitPartition of the rows (adj_net === nothing)
  greedy_setup_domain(A, adj_A, K, Pi, mdl)      :42-68   the same for any partition, through its DomainPartition
  greedy_walk(A, K, Pi, mdl, order, state)       :70-90 / :153-173   randperm(n) -> order; update=False: the same loop with the cost
                                                 update removed (what a kernel that forgets it would compute)
  greedy(A, K, Pi, mdl, order)                   the method as dispatch picks it

Arrays are used 1-based as the reference uses them (index 0 is padding).  Also here, from the definitions and a dense mask: the counts
the setup must produce, and the cost of every part of a column partition given as arbitrary column sets."""
import numpy as np

import cpamd
from greedy_model import transpose
from util import dense_mask

cp = cpamd.load()


def _one_based(A):
    return [0] + [int(x) for x in A.colptr], [0] + [int(x) for x in A.rowval]


def _asg(Pi):
    return [0] + [int(x) for x in cp.to_map(Pi).asg]


def magnetic(A, K, Pi, draws):
    n = A.n
    colptr, rowval = _one_based(A)
    pasg = _asg(Pi)
    asg = [0] * (n + 1)
    for j in range(1, n + 1):
        u = int(draws[j - 1])
        if colptr[j] == colptr[j + 1]:
            asg[j] = 1 + u % K
        else:
            i = rowval[colptr[j] + u % (colptr[j + 1] - colptr[j])]
            asg[j] = pasg[i]
    return np.array(asg[1:], dtype=np.int64)


def _mdl(mdl, nv, np_, nl, nr, k):
    """method.mdl(n_vertices, n_pins, n_local_nets, n_remote_nets, k): SecondaryConnectivityCosts.jl:19, left to right"""
    a = mdl.alpha if mdl.alpha_k is None else mdl.alpha_k[k - 1]
    return a + nv * mdl.beta_vertex + np_ * mdl.beta_pin + nl * mdl.beta_local_net + nr * mdl.beta_remote_net


def greedy_setup_split(A, adj_A, K, Pi, mdl):
    """-> state = [n_vertices, n_pins, n_local_nets, n_remote_nets, cst], each 1-based of K entries"""
    n = A.n
    tpos, tidx = _one_based(adj_A)
    spl = [0] + [int(x) for x in Pi.spl]
    nv, npins, nl, nr, cst = ([0] * (K + 1) for _ in range(5))
    hst = [0] * (n + 1)
    for k in range(1, K + 1):
        i, ip = spl[k], spl[k + 1]
        nv_k = ip - i
        np_k = tpos[ip] - tpos[i]
        nl_k = 0
        nr_k = 0
        for _i in range(i, ip):
            for _q in range(tpos[_i], tpos[_i + 1]):
                j = tidx[_q]
                if hst[j] < i:
                    nr_k += 1
                hst[j] = i
        nv[k], npins[k], nl[k], nr[k] = nv_k, np_k, nl_k, nr_k
        cst[k] = _mdl(mdl, nv_k, np_k, nl_k, nr_k, k)
    return [nv, npins, nl, nr, cst]


def greedy_setup_domain(A, adj_A, K, Pi, mdl):
    n = A.n
    tpos, tidx = _one_based(adj_A)
    dmn = cp.to_domain(Pi)
    spl = [0] + [int(x) for x in dmn.spl]
    prm = [0] + [int(x) for x in dmn.prm]
    nv, npins, nl, nr, cst = ([0] * (K + 1) for _ in range(5))
    hst = [0] * (n + 1)
    for k in range(1, K + 1):
        s, sp = spl[k], spl[k + 1]
        nv_k = sp - s
        np_k = 0
        nl_k = 0
        nr_k = 0
        for _s in range(s, sp):
            _i = prm[_s]
            q, qp = tpos[_i], tpos[_i + 1]
            np_k += qp - q
            for _q in range(q, qp):
                j = tidx[_q]
                if hst[j] < s:
                    nr_k += 1
                hst[j] = s
        nv[k], npins[k], nl[k], nr[k] = nv_k, np_k, nl_k, nr_k
        cst[k] = _mdl(mdl, nv_k, np_k, nl_k, nr_k, k)
    return [nv, npins, nl, nr, cst]


def greedy_walk(A, K, Pi, mdl, order, state, update=True):
    """-> (asg, cst): the MapPartition's asg (n entries) and the final part costs (K entries)"""
    n = A.n
    colptr, rowval = _one_based(A)
    pasg = _asg(Pi)
    nv, npins, nl, nr, cst = ([*x] for x in state)
    asg = [1] * (n + 1)
    for j in (int(x) for x in order):
        best_c = -float("inf")
        best_k = 0
        for q in range(colptr[j], colptr[j + 1]):
            i = rowval[q]
            k = pasg[i]
            c = cst[k]
            if c > best_c:
                best_c = c
                best_k = k
        if best_k != 0:
            asg[j] = best_k
            if update:
                nl[best_k] += 1
                nr[best_k] -= 1
                cst[best_k] = _mdl(mdl, nv[best_k], npins[best_k], nl[best_k], nr[best_k], best_k)
    return np.array(asg[1:], dtype=np.int64), np.array(cst[1:], dtype=mdl.cost_dtype())


def greedy(A, K, Pi, mdl, order, update=True, adj_A=None):
    adj_A = adj_A if adj_A is not None else transpose(A)
    setup = greedy_setup_split if isinstance(Pi, cp.SplitPartition) else greedy_setup_domain
    return greedy_walk(A, K, Pi, mdl, order, setup(A, adj_A, K, Pi, mdl), update)


# ---------------------------------------------------------------- the inputs the tests of the two partitioners share
SHAPES = ((12, 0.3), (300, 0.5), (2000, 0.01))       # (m, density): short columns; columns across 64 and 256 entries; many empty ones
NS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)
KS = (1, 2, 5, 64, 300)
_matrices = {}


def matrix(m, density, n):
    """greedy_model.copy_columns(m, n, density, 7000 + 13 n + m) and its transpose, built once"""
    from greedy_model import copy_columns
    if (m, n) not in _matrices:
        A = copy_columns(m, n, density, 7000 + 13 * n + m)
        _matrices[(m, n)] = (A, transpose(A))
    return _matrices[(m, n)]


def models(K):
    S = cp.AffineSecondaryConnectivityModel
    return (S(0, 10, 1, 0, 100), S(0, 0, 0, 0, 1), S(0.5, 0.1, 1.3, 0.7, 2.9), S(0, 10, 1, 0, 100, alpha_k=[(37 * k * k) % 101 for k in range(1, K + 1)]))


def row_partition(kind, m, K):
    """the split i K div m, the map i mod K (i = 0 .. m - 1, parts from 1), or the map told as a DomainPartition"""
    i = np.arange(m, dtype=np.int64)
    if kind == "split":
        return cp.SplitPartition(K, 1 + np.searchsorted(i * K // m, np.arange(K + 1), side="left"))
    P = cp.MapPartition(K, i % K + 1)
    return cp.to_domain(P) if kind == "domain" else P


def family():
    """(m, n, K, index of the model, kind of Pi): every shape, size, K and model, Pi alternately a split and a map"""
    for m, density in SHAPES:
        for a, n in enumerate(NS):
            for b, K in enumerate(KS):
                for c in range(4):
                    yield m, density, n, K, c, ("split", "map")[(a + b) % 2]


# ---------------------------------------------------------------- from the definitions, on a dense mask
def setup_counts(A, K, Pi):
    """(n_vertices, n_pins, n_remote_nets), K entries each: the rows of part k, the entries in those rows, the columns that hold one"""
    D = dense_mask(A)
    pasg = cp.to_map(Pi).asg
    rows = [pasg == k for k in range(1, K + 1)]
    return (np.array([r.sum() for r in rows], dtype=np.int64), np.array([D[r].sum() for r in rows], dtype=np.int64),
            np.array([D[r].any(axis=0).sum() for r in rows], dtype=np.int64))


def secondary_costs(A, K, Pi, Phi, mdl):
    """the cost of every part k of Pi (rows) when part k of Phi (columns, any sets) is given to it: a column that holds a row of
    the part is a local net if the part owns it, else a remote one"""
    D = dense_mask(A)
    pasg, casg = cp.to_map(Pi).asg, cp.to_map(Phi).asg
    out = []
    for k in range(1, K + 1):
        r = pasg == k
        touched = D[r].any(axis=0)
        local = int((touched & (casg == k)).sum())
        out.append(_mdl(mdl, int(r.sum()), int(D[r].sum()), local, int(touched.sum()) - local, k))
    return np.array(out, dtype=mdl.cost_dtype())


def part_costs(A, Phi, mdl, Pi=None):
    """the cost of every part of the column partition Phi (any sets) under a Work, Connectivity, HyperedgeCut or primary
    connectivity model, from the definitions: vertices, pins, the rows the part touches, those it touches alone, and -- primary --
    the touched rows the part's own number owns"""
    D = dense_mask(A)
    casg = cp.to_map(Phi).asg
    pasg = None if Pi is None else cp.to_map(Pi).asg
    out = []
    for k in range(1, Phi.K + 1):
        S = casg == k
        nv, npins = int(S.sum()), int(D[:, S].sum())
        nets = D[:, S].any(axis=1)
        if isinstance(mdl, cp.AffinePrimaryConnectivityModel):
            local = int((nets & (pasg == k)).sum())
            out.append(mdl(nv, npins, local, int(nets.sum()) - local, k))
        elif isinstance(mdl, cp.AffineHyperedgeCutModel):
            selfn = int((nets & ~D[:, ~S].any(axis=1)).sum())
            out.append(mdl(nv, npins, selfn, int(nets.sum()) - selfn, k))
        elif isinstance(mdl, cp.AffineConnectivityModel):
            out.append(mdl(nv, npins, int(nets.sum()), k))
        else:
            out.append(mdl(nv, npins, k))
    return out
