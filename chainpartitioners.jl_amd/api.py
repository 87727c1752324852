"""partition_stripe / pack_stripe / oracle_stripe / bound_stripe / total_value /
bottleneck_value -- the reference's dispatch API for the hot path, host side.

Each function marshals its Julia-shaped arguments into the flat C structs of
include/chainpart_types.h and calls a backend.  The product backend is the HIP C-ABI
library (`_lib.HipBackend`, libchainpart.so); there is no CPU fallback in this package --
if the library or a GPU is missing the call raises.  Tests inject the CPU oracle through
the same `backend=` hook to compare the two on identical marshalled inputs.

Reference entry points mirrored (under /root/reference/src):
  partition_stripe  EquiPartitioner.jl:5, DynamicSplitter.jl:15,52,206,260,
                    BisectCostBottleneckSplitter.jl:6,70, ConvexTotalChunker.jl:26,170, MagneticPartitioner.jl:3,26,96
  pack_stripe       EquiPartitioner.jl:15, DynamicChunker.jl:15,20, ConvexTotalChunker.jl:9,141, StrictChunker.jl:5, OverlapChunker.jl:6
  pack_plaid        AlternatingPacker.jl:18,40
  permute_stripe / permute_plaid   Permutations.jl:33-41, CuthillMcKeePermuter.jl:209-265; PermutingPartitioner.jl:6-64
  oracle_stripe / bound_stripe / total_value / bottleneck_value   Costs.jl:3-66
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import models as M
from .types import (SparseMatrixCSC, SplitPartition, MapPartition, DomainPartition, StepHint, NoHint, to_map, to_domain, DomainPermutation, perm)

_default_backend = None


def set_default_backend(b):
    global _default_backend
    _default_backend = b


def get_backend(backend=None):
    if backend is not None:
        return backend
    global _default_backend
    if _default_backend is None:
        from ._lib import HipBackend
        _default_backend = HipBackend()          # raises loudly if the HIP library / GPU is absent
    return _default_backend


class CPError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"chainpart status {code}: {msg}")
        self.code = code


def _check(rc, what, backend):
    if rc == M.CP_OK or rc == M.CP_INFEASIBLE:
        return rc
    msg = backend.last_error() if hasattr(backend, "last_error") else ""
    if rc == M.CP_EINVAL:
        raise AssertionError(f"{what}: violated precondition ({msg})")   # Julia: AssertionError
    if rc == M.CP_EUNSUPPORTED:
        raise NotImplementedError(f"{what}: no method for this (method, model) pair ({msg})")
    raise CPError(rc, f"{what}: {msg}")


def _rowpart(Pi, need_spl=False):
    """Marshal an optional row partition -> (cp_rowpart_t | None, keepalive)."""
    if Pi is None:
        return None, []
    rp = M.cp_rowpart_t()
    keep = []
    rp.K = Pi.K
    if isinstance(Pi, SplitPartition):
        spl = np.ascontiguousarray(Pi.spl, dtype=np.int64)
        asg = to_map(Pi).asg
        keep += [spl, asg]
        rp.spl = spl.ctypes.data
        rp.asg = asg.ctypes.data
    elif isinstance(Pi, (MapPartition, DomainPartition)):          # a DomainPartition goes as its map (Partitions.jl:62-84)
        asg = np.ascontiguousarray(to_map(Pi).asg, dtype=np.int64)
        keep += [asg]
        rp.asg = asg.ctypes.data
        rp.spl = None
    else:
        raise TypeError("row partition must be a SplitPartition, MapPartition or DomainPartition")
    return rp, keep


def _w_table_for(A, f, weight, w_max, stack_method=False):
    """Tabulation range (lo, hi) of closures over the part width.  DP methods only evaluate feasible pairs: 0 .. w_max under a
    VertexCount constraint, else 0 .. n.  The Convex/Concave chunkers (stack_method) also evaluate pairs outside the
    constraint and -- when the cost is not convex and their candidate stack goes stale -- pairs with j > j' inside one
    feasible window (ConvexTotalChunker.jl:76,99): widths -(w_max+1) .. 2(w_max+1) under VertexCount, -n .. n otherwise."""
    if weight is not None and isinstance(weight, M.VertexCount):
        w = int(w_max)
        return (-(2 * w + 2), 2 * w + 3) if stack_method else (0, w + 1)
    return (-(A.n + 1), A.n + 1) if stack_method else (0, A.n + 1)


def _need_hip(b, mdl):
    """The symmetric cost family and the plaid edge-cut pair exist on the HIP backend only (the CPU test oracle does not know
    these kinds)."""
    if (getattr(mdl, "symmetric", False) or getattr(mdl, "hip_only", False)) and getattr(b, "name", "") != "hip":
        raise NotImplementedError(f"{type(mdl).__name__} is implemented by the HIP backend only, not by backend "
                                  f"'{getattr(b, 'name', type(b).__name__)}'")


def _refuse_envelope(fn, method):
    """The envelope oracle has a 3-argument method only (EnvelopeCosts.jl:66-73): the splitter-order DP and the (non-flip) Bisect
    splitters can call it, the chunker loops and stack methods (ocl(j, j')) cannot, and the library has no constrained, lazy or
    flip form for it.  Raised before anything is marshalled, in the words the library's own refusals use (each entry of
    the library refuses the kind as well: tests/test_gpu_envelope.py calls them directly)."""
    if not hasattr(method, "f"):
        return
    mdl, weight, _ = M.split_constraint(method.f)
    if not isinstance(mdl, M.AffineEnvelopeModel) and not isinstance(weight, M.AffineEnvelopeModel):
        return
    name = type(method).__name__
    if weight is not None:
        raise NotImplementedError(f"{fn}({name}): ConstrainedCost with an AffineEnvelopeModel as cost or weight has no device path")
    served = (isinstance(method, (M.DynamicTotalSplitter, M.DynamicBottleneckSplitter, M.BisectCostBottleneckSplitter, M.BisectIndexBottleneckSplitter))
              and not getattr(method, "flip", 0) and fn == "partition_stripe")
    if not served:
        raise NotImplementedError(f"{fn}({name}): AffineEnvelopeModel has no device path in this method (served: Dynamic{{Total,Bottleneck}}Splitter, "
                                  f"BisectCostBottleneckSplitter and BisectIndexBottleneckSplitter; the chunker loops call ocl(j, j'), for which "
                                  f"the envelope oracle has no method)")


def _lazy_primary_needs_hip(b, mdl):
    """LazyBisectCost on a primary connectivity model (LazyBisectCostBottleneckSplitter.jl:390-483) is a kernel of the HIP backend;
    the CPU test oracle does not know the pair."""
    if getattr(mdl, "kind", None) == M.CP_MODEL_PRIMARY and getattr(b, "name", "") != "hip":
        raise NotImplementedError(f"LazyBisectCostBottleneckSplitter({type(mdl).__name__}) is implemented by the HIP backend only, not by "
                                  f"backend '{getattr(b, 'name', type(b).__name__)}'")


def _marshal(A, f, Pi, stack_method=False):
    mdl, weight, w_max = M.split_constraint(f)
    wlo, wt = _w_table_for(A, mdl, weight, w_max, stack_method)
    if not isinstance(mdl, (M.BlockComponentCostModel, M.ColumnBlockComponentCostModel)):
        wlo = 0
    # the block model's row tables run to m + 1 unless the model presets u_table (a preset w_table does not win)
    ut = A.m + 1 if isinstance(mdl, M.BlockComponentCostModel) and mdl.u_table is None else None
    mm = mdl.marshal(w_table=wt, w_lo=wlo, u_table=ut)
    wm = weight.marshal() if weight is not None else None
    wmax_i = int(w_max) if weight is not None and (weight.dtype == M.CP_I64) else 0
    wmax_f = float(w_max) if weight is not None else 0.0
    rp, keep = _rowpart(Pi)
    return mdl, mm, wm, wmax_i, wmax_f, rp, keep


# ---------------------------------------------------------------- partition_stripe / pack_stripe
# How a method reaches the backend: the backend method, the name _check reports, stack_method of _w_table_for, when Pi is
# passed, the refusal of a ConstrainedCost (None: constraints are served) and the method's own scalars.  A row that serves
# constraints calls b.<call>(A, [K,] *scalars, mm, rp, wm, wi, wf, *outs), one that refuses them b.<call>(A, K, mm, *scalars,
# spl[, rp]).  Rows are found along the MRO, so the Reference* and Flip* classes follow their bases.
_Row = namedtuple("_Row", "call what stack pi refuse scalars")
_PI_ALWAYS, _PI_IF_NEEDED, _PI_NEVER = "always", "if the model needs_rowpart", "never"
# The backend method of LazyBisectCost has no argument for Pi (its call is pinned as (A, K, mm, eps, spl)), and only its primary
# specialisation reads one: for a model with needs_rowpart Pi travels on the marshalled model, as mm.rowpart.
_PI_ON_MODEL = "on the marshalled model, if the model needs_rowpart"
_DYNAMIC = _Row("partition_dynamic", "Dynamic*", False, _PI_ALWAYS, None, lambda m: (m.combine, m.order))
_PARTITION = {
    M.DynamicTotalSplitter: _DYNAMIC, M.DynamicBottleneckSplitter: _DYNAMIC,
    M.DynamicTotalChunker: _DYNAMIC, M.DynamicBottleneckChunker: _DYNAMIC,
    M.BisectCostBottleneckSplitter: _Row("partition_bisect_cost", "BisectCost", False, _PI_IF_NEEDED,
                                         "BisectCost on a ConstrainedCost errors in the reference (Costs.jl:150)", lambda m: (m.eps, m.flip)),
    M.BisectIndexBottleneckSplitter: _Row("partition_bisect_index", "BisectIndex", False, _PI_IF_NEEDED,
                                          "BisectIndex on a ConstrainedCost errors in the reference (Costs.jl:150)", lambda m: (m.flip,)),
    M.LazyBisectCostBottleneckSplitter: _Row("partition_lazy_bisect_cost", "LazyBisectCost", False, _PI_ON_MODEL,
                                             "LazyBisectCost on a ConstrainedCost has no method in the reference", lambda m: (m.eps,)),
    M.LazyFlipBisectCostBottleneckSplitter: _Row("partition_lazy_flip_bisect_cost", "LazyFlipBisectCost", False, _PI_IF_NEEDED,
                                                 "LazyFlipBisectCost on a ConstrainedCost has no method in the reference", lambda m: (m.eps,)),
    M.ConvexTotalSplitter: _Row("partition_convex", "ConvexTotalSplitter", True, _PI_ALWAYS, None, lambda m: ()),
    M.ConcaveTotalSplitter: _Row("partition_concave", "ConcaveTotalSplitter", True, _PI_ALWAYS, None, lambda m: ()),
}
_PACK = {
    M.DynamicTotalChunker: _Row("pack_dynamic", "DynamicTotalChunker", False, _PI_ALWAYS, None, lambda m: ()),
    M.ConvexTotalChunker: _Row("pack_convex", "ConvexTotalChunker", True, _PI_ALWAYS, None, lambda m: ()),
    M.ConcaveTotalChunker: _Row("pack_concave", "ConcaveTotalChunker", True, _PI_ALWAYS, None, lambda m: ()),
}


def _dispatch(fn, table, head, method, Pi, backend, alloc):
    """The body partition_stripe (head = (A, K)) and pack_stripe (head = (A,)) share: marshal, allocate the outputs, one backend
    call, _check.  -> the outputs"""
    b = get_backend(backend)
    if hasattr(method, "f"):
        _need_hip(b, M.split_constraint(method.f)[0])
    _refuse_envelope(fn, method)
    row = next((table[c] for c in type(method).__mro__ if c in table), None)
    if row is None:
        raise NotImplementedError(f"{fn}: method {type(method).__name__} is outside the hot path")
    if isinstance(method, M.LazyFlipBisectCostBottleneckSplitter) and not hasattr(b, row.call):      # a kernel of the HIP backend
        raise NotImplementedError(f"{type(method).__name__}: backend '{getattr(b, 'name', type(b).__name__)}' has no method {row.call}")
    needs = hasattr(method, "f") and getattr(M.split_constraint(method.f)[0], "needs_rowpart", False)
    rides = None
    if row.pi == _PI_ON_MODEL:
        _lazy_primary_needs_hip(b, M.split_constraint(method.f)[0])
        rides, Pi = (Pi if needs else None), None
    if row.pi == _PI_NEVER or (row.pi == _PI_IF_NEEDED and not needs):
        Pi = None
    mdl, mm, wm, wi, wf, rp, keep = _marshal(head[0], method.f, Pi, row.stack)
    if rides is not None:
        mm.rowpart, mm.rowpart_keep = _rowpart(rides)
    if row.refuse is not None and wm is not None:
        raise NotImplementedError(row.refuse)
    outs = alloc()
    if row.refuse is None:
        args = (*row.scalars(method), mm, rp, wm, wi, wf, *outs)
    else:
        args = (mm, *row.scalars(method), *outs) + ((rp,) if row.pi == _PI_IF_NEEDED else ())
    rc = getattr(b, row.call)(*head, *args)
    _check(rc, f"{fn}({row.what})", b)
    return outs


def _partition_map(A, K, method, Pi, backend):
    """MagneticPartitioner / GreedyBottleneckPartitioner (MagneticPartitioner.jl:3-20, :26-177): the two methods that return a
    MapPartition.  Both need the row partition Pi (any kind, of the m rows); the draws are the method's own fields."""
    b = get_backend(backend)
    name = type(method).__name__
    greedy = isinstance(method, M.GreedyBottleneckPartitioner)
    if greedy and not isinstance(method.mdl, M.AffineSecondaryConnectivityModel):
        raise NotImplementedError(f"{name}({type(method.mdl).__name__}): the reference has a method for an AffineSecondaryConnectivityModel only")
    if Pi is None:
        raise NotImplementedError(f"partition_stripe(A, K, {name}) without a row partition Pi has no method in the reference")
    call = "partition_greedy_bottleneck" if greedy else "partition_magnetic"
    if not hasattr(b, call):
        raise NotImplementedError(f"{name} is implemented by the HIP backend only, not by backend '{getattr(b, 'name', type(b).__name__)}'")
    rp, keep = _rowpart(Pi)
    if keep[-1].shape != (A.m,):                                # (keep[-1]: the map form of Pi)
        raise AssertionError(f"partition_stripe({name}): Pi must assign the {A.m} rows of A, it has {keep[-1].size} entries")
    given = method.order if greedy else method.draws
    if given is not None and given.shape != (A.n,):
        raise AssertionError(f"partition_stripe({name}): {'order' if greedy else 'draws'} must have one entry per column")
    asg = np.zeros(A.n, dtype=np.int64)
    if greedy:
        rc, order, cst = b.partition_greedy_bottleneck(A, K, method.mdl.marshal(), rp, method.seed, given, asg)
        b.last_greedy = {"order": order, "cst": cst}             # the order that was walked and the K final part costs
    else:
        rc = b.partition_magnetic(A, K, rp, method.seed, given, asg)
    _check(rc, f"partition_stripe({name})", b)
    return MapPartition(K, asg)


def partition_stripe(A: SparseMatrixCSC, K, method, Pi=None, *, backend=None, adj_A=None, adj_net=None):
    """-> SplitPartition, or MapPartition from the map partitioners (DomainPartition through a PermutingPartitioner).  adj_A /
    adj_net: the reference's keywords of GreedyBottleneckPartitioner (MagneticPartitioner.jl:26, :96), accepted and ignored -- the
    device setup counts the parts of Pi from A's own columns and needs neither the adjoint nor its net counter."""
    K = int(K)
    if isinstance(method, M.PermutingPartitioner):              # PermutingPartitioner.jl:18-34: Pi, a row partition, passes through
        tau, B = _permuted_stripe(A, method, backend)
        return tau[partition_stripe(B, K, method.prt, Pi, backend=backend)]
    if isinstance(method, (M.MagneticPartitioner, M.GreedyBottleneckPartitioner)):
        return _partition_map(A, K, method, Pi, backend)
    if isinstance(method, M.EquiSplitter):
        # closed form, O(K) host arithmetic (EquiPartitioner.jl:7)
        n = A.n
        k = np.arange(0, K + 1, dtype=np.int64)
        return SplitPartition(K, k * (n // K) + np.minimum(n % K, k) + 1)
    spl, = _dispatch("partition_stripe", _PARTITION, (A, K), method, Pi, backend, lambda: (np.zeros(K + 1, dtype=np.int64),))
    return SplitPartition(K, spl)


def partition_stripe_batch(A: SparseMatrixCSC, requests, *, backend=None):
    """[partition_stripe(A, K, method) for (K, method) in requests] in ONE device launch, for the methods whose single partition is a
    sequential chain on one wave: BisectCostBottleneckSplitter(f, eps) with Work / Connectivity costs (a sweep over K, eps and the
    model constants; BisectCostBottleneckSplitter.jl:6-63 per request).  The reference has no batch call -- it would loop; the
    results are those of the loop."""
    b = get_backend(backend)
    if not requests:
        return []
    for _, m in requests:
        if hasattr(m, "f"):
            _need_hip(b, M.split_constraint(m.f)[0])
        _refuse_envelope("partition_stripe_batch", m)
    if not all(isinstance(m, M.BisectCostBottleneckSplitter) for _, m in requests):
        raise NotImplementedError("partition_stripe_batch takes BisectCostBottleneckSplitter requests")
    if not hasattr(b, "partition_bisect_cost_batch"):
        return [partition_stripe(A, K, m, backend=b) for K, m in requests]
    mms = []
    for K, m in requests:
        mdl, mm, wm, wi, wf, rp, keep = _marshal(A, m.f, None)
        if wm is not None:
            raise NotImplementedError("BisectCost on a ConstrainedCost errors in the reference (Costs.jl:150)")
        mms.append(mm)
    rc, spls = b.partition_bisect_cost_batch(A, [int(K) for K, _ in requests], mms, [m.eps for _, m in requests], [int(m.flip) for _, m in requests])
    _check(rc, "partition_stripe_batch(BisectCost)", b)
    return [SplitPartition(int(K), s) for (K, _), s in zip(requests, spls)]


def pack_stripe_batch(A: SparseMatrixCSC, methods, *, backend=None):
    """[pack_stripe(A, method) for method in methods] in ONE device launch for ConvexTotalChunker(ConstrainedCost(f, VertexCount(), w))
    requests with 1 <= w <= 15 and ColumnBlock / Connectivity / Work costs (ConvexTotalChunker.jl:141-168, 211-265 per request): a sweep
    over the cost constants and width limits.  The results are those of the loop."""
    b = get_backend(backend)
    if not methods:
        return []
    for m in methods:
        if hasattr(m, "f"):
            _need_hip(b, M.split_constraint(m.f)[0])
        _refuse_envelope("pack_stripe_batch", m)
    ok = all(isinstance(m, M.ConvexTotalChunker) and isinstance(M.split_constraint(m.f)[1], M.VertexCount) for m in methods)
    if not ok:
        raise NotImplementedError("pack_stripe_batch takes ConvexTotalChunker(ConstrainedCost(f, VertexCount(), w)) requests")
    if not hasattr(b, "pack_convex_batch"):
        return [pack_stripe(A, m, backend=b) for m in methods]
    mms, ws = [], []
    for m in methods:
        mdl, mm, wm, wi, wf, rp, keep = _marshal(A, m.f, None, stack_method=True)
        mms.append(mm); ws.append(int(wi))
    rc, spls = b.pack_convex_batch(A, mms, ws, A.n)
    _check(rc, "pack_stripe_batch(ConvexTotalChunker)", b)
    return [SplitPartition(len(s) - 1, s) for s in spls]


# ---------------------------------------------------------------- pack_stripe
def _pack_greedy(A, method, n_nets, backend):
    """StrictChunker / OverlapChunker (StrictChunker.jl:5, OverlapChunker.jl:6): no cost model to marshal, Pi is not looked at."""
    b = get_backend(backend)
    call = "pack_strict" if isinstance(method, M.StrictChunker) else "pack_overlap"
    if not hasattr(b, call):
        raise NotImplementedError(f"{type(method).__name__} is implemented by the HIP backend only, not by backend "
                                  f"'{getattr(b, 'name', type(b).__name__)}'")
    spl, Kout = np.zeros(A.n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    if isinstance(method, M.StrictChunker):
        rc = b.pack_strict(A, method.w_max, spl, Kout)
    else:
        nn = None if n_nets is None else np.zeros(max(A.n, 1), dtype=np.int64)
        rc = b.pack_overlap(A, method.rho, method.w_max, spl, Kout, nn)
    _check(rc, f"pack_stripe({type(method).__name__})", b)
    K = int(Kout[0])
    if n_nets is not None and isinstance(method, M.OverlapChunker):
        n_nets[0] = nn[:K].copy()
    return SplitPartition(K, spl[:K + 1].copy())


def pack_stripe(A: SparseMatrixCSC, method, Pi=None, *, n_nets=None, backend=None) -> SplitPartition:
    """n_nets: a one-element list standing for the reference's Ref (OverlapChunker.jl:6, :24-29); OverlapChunker leaves the int64
    array of the K parts' distinct-row counts in its element 0.  The other methods ignore it, as the reference's kwargs... do."""
    if isinstance(method, M.PermutingPartitioner):              # PermutingPartitioner.jl:48-64
        tau, B = _permuted_stripe(A, method, backend)
        return tau[pack_stripe(B, method.prt, Pi, n_nets=n_nets, backend=backend)]
    if isinstance(method, M.EquiChunker):
        n, w = A.n, method.w
        spl = np.concatenate([np.arange(1, n + 1, w, dtype=np.int64), [n + 1]])   # [1:w:n; n+1]
        return SplitPartition(len(spl) - 1, spl)
    if isinstance(method, (M.StrictChunker, M.OverlapChunker)):
        return _pack_greedy(A, method, n_nets, backend)
    spl, Kout = _dispatch("pack_stripe", _PACK, (A,), method, Pi, backend,
                          lambda: (np.zeros(A.n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)))
    return SplitPartition(int(Kout[0]), spl[:int(Kout[0]) + 1].copy())


def pack_stripe_tables(A: SparseMatrixCSC, method, Pi=None, *, backend=None):
    """(cst, spl) of pack_stripe(A, DynamicTotalChunker(f)): the per-column tables DynamicChunker.jl:20-56 builds before
    unravel_chunks!, indexed by j' - 1 -- cst[j' - 1] is the least total cost of columns 1 : j' - 1, spl[j' - 1] the smallest
    minimising start of its last chunk (spl[0] = 0)."""
    if not isinstance(method, M.DynamicTotalChunker):
        raise NotImplementedError(f"pack_stripe_tables: method {type(method).__name__} is not a DynamicTotalChunker")
    b = get_backend(backend)
    _need_hip(b, M.split_constraint(method.f)[0])
    _refuse_envelope("pack_stripe_tables", method)
    if not hasattr(b, "pack_dynamic_tables"):
        raise NotImplementedError(f"pack_stripe_tables: backend {b.name} has no tables")
    mdl, mm, wm, wi, wf, rp, keep = _marshal(A, method.f, Pi)
    rc, cst, spl = b.pack_dynamic_tables(A, mm, rp, wm, wi, wf)
    _check(rc, "pack_stripe_tables(DynamicTotalChunker)", b)
    return cst, spl


# ---------------------------------------------------------------- oracles / scoring
class Oracle:
    """Callable cost oracle ocl(j, j', k...) (vectorised over arrays of queries)."""

    def __init__(self, hint, mdl, A, Pi, backend):
        _need_hip(backend, mdl)
        self.hint, self.mdl, self.A, self.Pi, self.backend = hint, mdl, A, Pi, backend

    def __call__(self, j, jp, k=None):
        scalar = np.isscalar(j)
        jj = np.atleast_1d(np.asarray(j, dtype=np.int64))
        jjp = np.atleast_1d(np.asarray(jp, dtype=np.int64))
        kk = None if k is None else np.broadcast_to(np.asarray(k, dtype=np.int64), jj.shape).copy()
        _, mm, _, _, _, rp, keep = _marshal(self.A, self.mdl, self.Pi)
        out = np.zeros(jj.shape, dtype=self.mdl.cost_dtype())
        rc = self.backend.oracle_eval(self.A, mm, rp, self.hint.code, jj, jjp, kk, out)
        _check(rc, "oracle", self.backend)
        return out[0].item() if scalar else out


class _Move:
    code = None

    def __init__(self, arg):
        self.arg = int(arg)


class Same(_Move):
    code = 0


class Next(_Move):
    code = 1


class Prev(_Move):
    code = 2


class Jump(_Move):
    code = 3


class Step:
    """Step(ocl)(Same(j) | Next(j) | Prev(j) | Jump(j), <same for j'>, [Same(k)])  (Costs.jl:174-195).  Single calls keep the
    walk's previous position (the moves are promises about it, checked by the backend); `walk` takes a whole sequence."""

    def __init__(self, ocl):
        self.ocl = ocl
        self._last = None

    def __call__(self, mj, mjp, mk=None):
        k = None if mk is None else (mk.arg if isinstance(mk, _Move) else int(mk))
        if self._last is None:
            vals = self.walk([(mj, mjp, k)])
        else:                                       # replay the previous position so that the promise is checked
            vals = self.walk([(Jump(self._last[0]), Jump(self._last[1]), self._last[2]), (mj, mjp, k)])
        self._last = (mj.arg, mjp.arg, k)
        return vals[-1].item()

    def walk(self, moves):
        o = self.ocl
        mj = np.array([m[0].code for m in moves], dtype=np.int32); j = np.array([m[0].arg for m in moves], dtype=np.int64)
        mjp = np.array([m[1].code for m in moves], dtype=np.int32); jp = np.array([m[1].arg for m in moves], dtype=np.int64)
        ks = [m[2] if len(m) > 2 else None for m in moves]
        kk = None if all(x is None for x in ks) else np.array([0 if x is None else (x.arg if isinstance(x, _Move) else int(x)) for x in ks], dtype=np.int64)
        _, mm, _, _, _, rp, keep = _marshal(o.A, o.mdl, o.Pi)
        out = np.zeros(j.shape, dtype=o.mdl.cost_dtype())
        rc = o.backend.oracle_step(o.A, mm, rp, mj, j, mjp, jp, kk, out)
        _check(rc, "Step(oracle)", o.backend)
        return out


def oracle_stripe(hint, mdl, A, Pi=None, *, backend=None) -> Oracle:
    return Oracle(hint, mdl, A, Pi, get_backend(backend))


def bound_stripe(A, K, mdl, Pi=None, *, backend=None):
    """bound_stripe(A, K, [Pi], mdl): Pi only matters to the secondary models (Costs.jl:17-19; SecondaryConnectivityCosts.jl:21-31,
    SecondaryEdgeCutCosts.jl:20-28)."""
    b = get_backend(backend)
    _need_hip(b, mdl)
    mm = mdl.marshal(w_table=A.n + 1)
    if Pi is not None and isinstance(mdl, (M.AffineSecondaryConnectivityModel, M.AffineSecondaryEdgeCutModel)):
        rp, keep = _rowpart(Pi)
        rc, lo, hi = b.bound_stripe_pi(A, int(K), rp, mm)
    else:
        rc, lo, hi = b.bound_stripe(A, int(K), mm)
    _check(rc, "bound_stripe", b)
    return lo, hi


def _objective(g, A, Phi, mdl, Pi, backend):
    b = get_backend(backend)
    if isinstance(Phi, (MapPartition, DomainPartition)):
        # compute_objective for any Phi (Costs.jl:34-39, :52-57): gather the parts' columns together on the device and score the
        # split of the gathered matrix; Pi, a partition of the rows, passes through.  The symmetric family has one partition for
        # rows and columns, so both sides are permuted (the reference would permute the columns only: DESIGN.md section 5f).
        dom = to_domain(Phi)
        prm = DomainPermutation(dom.prm)
        A_prm = permute(A, prm if getattr(mdl, "symmetric", False) else None, prm, backend=b)
        return _objective(g, A_prm, SplitPartition(dom.K, dom.spl), mdl, Pi, b)
    if not isinstance(Phi, SplitPartition):
        raise TypeError("Phi must be a SplitPartition, MapPartition or DomainPartition")
    _need_hip(b, mdl)
    _, mm, _, _, _, rp, keep = _marshal(A, mdl, Pi)
    rc, v = b.objective(A, Phi.K, np.ascontiguousarray(Phi.spl, dtype=np.int64), mm, rp, g)
    _check(rc, "objective", b)
    return v


def total_value(A, Phi, mdl, Pi=None, *, backend=None):
    """total_value(A, [Pi], Phi, mdl)  Costs.jl:28-29"""
    return _objective(M.CP_COMBINE_SUM, A, Phi, M.split_constraint(mdl)[0], Pi, backend)


def bottleneck_value(A, Phi, mdl, Pi=None, *, backend=None):
    """bottleneck_value(A, [Pi], Phi, mdl)  Costs.jl:26-27"""
    return _objective(M.CP_COMBINE_MAX, A, Phi, M.split_constraint(mdl)[0], Pi, backend)


def partition_plaid(A: SparseMatrixCSC, K, method, *, adj_A=None, backend=None):
    """partition_plaid(A, K, method) -> (Pi, Phi)  (AlternatingPartitioner.jl:6-87): the 2-D callers of partition_stripe.
    A and its adjoint both stay resident on the device between the sweeps."""
    K = int(K)
    if isinstance(method, M.PermutingPartitioner):              # PermutingPartitioner.jl:6-16
        sigma, tau, B = _permuted_plaid(A, method, adj_A, backend)
        Pi, Phi = partition_plaid(B, K, method.prt, backend=backend)
        return sigma[Pi], tau[Phi]
    if isinstance(method, M.DisjointPartitioner):
        Phi = partition_stripe(A, K, method.mtd, backend=backend)
        T = adj_A if adj_A is not None else adjointpattern(A, backend=backend)
        Pi = partition_stripe(T, K, method.mtd2, Phi, backend=backend)
        return Pi, Phi
    if isinstance(method, M.AlternatingPartitioner):            # also AlternatingNetPartitioner
        T = adj_A if adj_A is not None else adjointpattern(A, backend=backend)
        Phi = partition_stripe(A, K, method.mtds[0], backend=backend)
        Pi = partition_stripe(T, K, method.mtds[1], Phi, backend=backend)
        for i, mtd in enumerate(method.mtds[2:], start=1):
            if i % 2 == 1:
                Phi = partition_stripe(A, K, mtd, Pi, backend=backend)
            else:
                Pi = partition_stripe(T, K, mtd, Phi, backend=backend)
        return Pi, Phi
    if isinstance(method, M.SymmetricPartitioner):
        if len(method.mtds) > 1:
            T = adj_A if adj_A is not None else adjointpattern(A, backend=backend)
            Pi = partition_stripe(A, K, method.mtds[0], backend=backend)
            for i, mtd in enumerate(method.mtds[1:], start=1):
                Pi = partition_stripe(A if i % 2 == 1 else T, K, mtd, Pi, backend=backend)
        else:
            Pi = partition_stripe(A, K, method.mtds[0], backend=backend)
        return Pi, Pi
    raise NotImplementedError(f"partition_plaid: method {type(method).__name__} is outside the hot path")


def pack_plaid(A: SparseMatrixCSC, method, *, adj_A=None, backend=None):
    """pack_plaid(A, method) -> (Pi, Phi)  (AlternatingPacker.jl:18-32, :40-53): the 2-D callers of pack_stripe, host orchestration
    over adjointpattern and pack_stripe -- any pack_stripe method, on any backend that has it.  DisjointPacker goes through a
    PermutedDimsArray, for which the reference has no chunker method: not served."""
    if isinstance(method, M.PermutingPartitioner):              # PermutingPartitioner.jl:36-46
        sigma, tau, B = _permuted_plaid(A, method, adj_A, backend)
        Pi, Phi = pack_plaid(B, method.prt, backend=backend)
        return sigma[Pi], tau[Phi]
    if isinstance(method, M.AlternatingPacker):
        T = adj_A if adj_A is not None else adjointpattern(A, backend=backend)
        Phi = pack_stripe(A, method.mtds[0], backend=backend)
        Pi = pack_stripe(T, method.mtds[1], Phi, backend=backend)
        for i, mtd in enumerate(method.mtds[2:], start=1):
            if i % 2 == 1:
                Phi = pack_stripe(A, mtd, Pi, backend=backend)
            else:
                Pi = pack_stripe(T, mtd, Phi, backend=backend)
        return Pi, Phi
    if isinstance(method, M.SymmetricPacker):
        T = adj_A if adj_A is not None else adjointpattern(A, backend=backend)
        Pi = pack_stripe(A, method.mtds[0], backend=backend)
        for i, mtd in enumerate(method.mtds[1:], start=1):
            Pi = pack_stripe(A if i % 2 == 1 else T, mtd, Pi, backend=backend)
        return Pi, Pi
    raise NotImplementedError(f"pack_plaid: method {type(method).__name__} is outside the hot path")


def adjointpattern(A: SparseMatrixCSC, *, backend=None) -> SparseMatrixCSC:
    """adjointpattern(A) (util.jl:67-95): transposed pattern, computed on the device (cp_adjoint); the returned matrix
    keeps its device handle, so partitioning it needs no upload."""
    return get_backend(backend).adjoint(A)


# ---------------------------------------------------------------- reordering
def permute_plaid(A: SparseMatrixCSC, method, adj_A=None, *, backend=None):
    """permute_plaid(A, method; adj_A) -> (sigma, tau), the row and the column permutation.  IdentityPermuter (Permutations.jl:38-41)
    is host arithmetic; CuthillMcKeePermuter (CuthillMcKeePermuter.jl:221-265) is the device walk of csrc/rcm.hip.  On its symmetric
    path sigma and tau are ONE object, as the reference returns one vector twice (test_CuthillMcKee.jl:28).  The counters of the
    call (cp_rcm's stats_out, by name) are left in backend.last_rcm_stats."""
    if isinstance(method, M.IdentityPermuter):
        return (DomainPermutation(np.arange(1, A.m + 1, dtype=np.int64)), DomainPermutation(np.arange(1, A.n + 1, dtype=np.int64)))
    if not isinstance(method, M.CuthillMcKeePermuter):
        raise NotImplementedError(f"permute_plaid: method {type(method).__name__} is outside the hot path")
    b = get_backend(backend)
    if not hasattr(b, "rcm"):
        raise NotImplementedError(f"CuthillMcKeePermuter is implemented by the HIP backend only, not by backend "
                                  f"'{getattr(b, 'name', type(b).__name__)}'")
    mode = 1 if method.assumesymmetry else 0 if method.checksymmetry else 2
    rc, rowprm, colprm, stats = b.rcm(A, adj_A, mode, method.reverse)
    _check(rc, "permute_plaid(CuthillMcKeePermuter)", b)
    b.last_rcm_stats = stats
    if stats["path"] == 1:
        sigma = DomainPermutation(colprm)
        return sigma, sigma
    return DomainPermutation(rowprm), DomainPermutation(colprm)


def permute_stripe(A: SparseMatrixCSC, method, *, backend=None):
    """permute_stripe(A, method) (Permutations.jl:33-36, CuthillMcKeePermuter.jl:209-211): the column half of permute_plaid"""
    return permute_plaid(A, method, backend=backend)[-1]


def permute(A: SparseMatrixCSC, sigma=None, tau=None, *, backend=None) -> SparseMatrixCSC:
    """A[perm(sigma), perm(tau)] on the device (cp_csr_permute; None: that side stays); the returned matrix keeps its device handle,
    like adjointpattern's."""
    b = get_backend(backend)
    if not hasattr(b, "csr_permute"):
        raise NotImplementedError(f"permute is implemented by the HIP backend only, not by backend '{getattr(b, 'name', type(b).__name__)}'")
    rc, B = b.csr_permute(A, None if sigma is None else perm(sigma), None if tau is None else perm(tau))
    _check(rc, "permute", b)
    return B


def quotientpattern(A: SparseMatrixCSC, Pi, *, backend=None) -> SparseMatrixCSC:
    """A with the rows of every part of the SplitPartition Pi merged (cp_csr_quotient): Pi.K x n, entry (k, c) where part k has a nonzero
    in column c -- the pattern BlockComponentCostModel is a weighted net count on.  Empty parts give empty rows.  The returned matrix
    keeps its device handle, like adjointpattern's."""
    b = get_backend(backend)
    if not hasattr(b, "csr_quotient"):
        raise NotImplementedError(f"quotientpattern is implemented by the HIP backend only, not by backend '{getattr(b, 'name', type(b).__name__)}'")
    rp, keep = _rowpart(Pi)
    rc, Q = b.csr_quotient(A, rp)
    _check(rc, "quotientpattern", b)
    return Q


def _permuted_stripe(A, method, backend):
    tau = permute_stripe(A, method.prm, backend=backend)
    return tau, permute(A, None, tau, backend=backend)


def _permuted_plaid(A, method, adj_A, backend):
    """The reference hands the UNPERMUTED adj_A on to the inner call on B (PermutingPartitioner.jl:13, :43); here the inner call
    takes the adjoint of B."""
    sigma, tau = permute_plaid(A, method.prm, adj_A, backend=backend)
    return sigma, tau, permute(A, sigma, tau, backend=backend)


# ---------------------------------------------------------------- counting structures
class CountMatrix:
    """netcount / selfnetcount / dominancecount object: obj[j, j'] (or obj(i, j)), vectorised."""

    def __init__(self, kind, A, hint, backend):
        self.kind, self.A, self.hint, self.backend = kind, A, hint, backend
        self.handle = backend.count_build(kind, A, hint.code)

    def __call__(self, a, b):
        scalar = np.isscalar(a)
        aa = np.atleast_1d(np.asarray(a, dtype=np.int64))
        bb = np.atleast_1d(np.asarray(b, dtype=np.int64))
        out = np.zeros(aa.shape, dtype=np.int64)
        rc = self.backend.count_query(self.kind, self.handle, aa, bb, out)
        _check(rc, "count query", self.backend)
        return int(out[0]) if scalar else out

    def __getitem__(self, ij):
        return self(*ij)

    def __del__(self):
        try:
            self.backend.count_free(self.kind, self.handle)
        except Exception:
            pass


def netcount(A, hint=None, *, backend=None):
    """netcount(hint, A)  SparseColorArrays.jl:57-58"""
    return CountMatrix("net", A, hint or NoHint(), get_backend(backend))


def selfnetcount(A, hint=None, *, backend=None):
    """selfnetcount(hint, A)  SparseColorArrays.jl:165-166"""
    return CountMatrix("selfnet", A, hint or NoHint(), get_backend(backend))


def dominancecount(A, hint=None, *, backend=None):
    """dominancecount(hint, A)  SparsePrefixMatrices.jl:438-446 : C[i, j] = #{nonzeros row < i, col < j}"""
    return CountMatrix("dom", A, hint or NoHint(), get_backend(backend))


class EnvelopeMatrix:
    """rowenvelope(A) (EnvelopeMatrices.jl:1-57): env[j, j'] -> (lo, hi), the least first row and the greatest last row of the
    columns j : j'-1, (m + 1, 0) for a range without entries.  The reference's implicit tree, built and walked on the device;
    .query(j, jp) is the batched getindex, .tree the (2^(H+1) - 1, 2) int64 nodes in the reference's order."""

    def __init__(self, A, backend):
        self.A, self.backend = A, backend                       # (the matrix keeps the device handle the tree is cached on alive)
        self.handle = backend.envelope_build(A)
        self.H, self.m, self.n = backend.envelope_dims(self.handle)

    @property
    def shape(self):
        return (self.n + 1, self.n + 1)

    @property
    def tree(self):
        return self.backend.envelope_tree(self.handle)

    def query(self, j, jp):
        """(lo, hi) arrays of env[j[i], jp[i]]"""
        jj = np.ascontiguousarray(np.atleast_1d(j), dtype=np.int64)
        jjp = np.ascontiguousarray(np.atleast_1d(jp), dtype=np.int64)
        if jj.shape != jjp.shape:
            raise ValueError("query: j and jp must have one shape")
        lo, hi = np.zeros(jj.shape, dtype=np.int64), np.zeros(jj.shape, dtype=np.int64)
        rc = self.backend.envelope_query(self.handle, jj, jjp, lo, hi)
        _check(rc, "envelope query", self.backend)
        return lo, hi

    def __getitem__(self, jjp):
        lo, hi = self.query(*jjp)
        return (int(lo[0]), int(hi[0])) if np.isscalar(jjp[0]) else (lo, hi)

    def __del__(self):
        try:
            self.backend.envelope_free(self.handle)
        except Exception:
            pass


def rowenvelope(A, backend=None):
    """rowenvelope(A)  EnvelopeMatrices.jl:10-33 (HIP backend only)"""
    b = get_backend(backend)
    if not hasattr(b, "envelope_build") or getattr(b, "name", "") != "hip":
        raise NotImplementedError(f"rowenvelope is implemented by the HIP backend only, not by backend '{getattr(b, 'name', type(b).__name__)}'")
    return EnvelopeMatrix(A, b)


def _sym_count(kind, A, hint, backend):
    b = get_backend(backend)
    if getattr(b, "name", "") != "hip":
        raise NotImplementedError(f"{kind}count is implemented by the HIP backend only")
    return CountMatrix(kind, A, hint or NoHint(), b)


def dianetcount(A, hint=None, *, backend=None):
    """dianetcount(hint, A)  SparseColorArrays.jl:65-99 : D[j, j'] = #(rows of A[:, j:j'-1] united with j:j'-1); square A"""
    return _sym_count("dianet", A, hint, backend)


def selfpincount(A, hint=None, *, backend=None):
    """selfpincount(hint, A)  SparseColorArrays.jl:268-318 : S[j, j'] = nnz(A[j:j'-1, j:j'-1]); square A"""
    return _sym_count("selfpin", A, hint, backend)
