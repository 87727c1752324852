"""Cost models, weights and partitioning methods of the hot path, plus their marshalling
into the flat C structs of include/chainpart_types.h.

Mirrors (file:line under /root/reference/src):
  AffineWorkModel                WorkCosts.jl:5-17
  AffineConnectivityModel        ConnectivityCosts.jl:7-20
  AffineHyperedgeCutModel        HyperedgeCutCosts.jl:7-21
  ColumnBlockComponentCostModel  BlockCosts.jl:1-17
  BlockComponentCostModel        BlockCosts.jl:19-44
  VertexCount                    SparseColorArrays.jl:1-6
  ConstrainedCost                Costs.jl:105-116
  EquiSplitter / EquiChunker     EquiPartitioner.jl:3-22
  Dynamic{Total,Bottleneck}{Splitter,Chunker}   DynamicSplitter.jl:1-13, DynamicChunker.jl:1-13
  Reference*                     ReferenceSplitter.jl:1-21
  [Flip]BisectCostBottleneckSplitter            BisectCostBottleneckSplitter.jl:1-4, 65-68
  ConvexTotalChunker / ConvexTotalSplitter      ConvexTotalChunker.jl:1-7
  AffineSymmetricConnectivityModel              SymmetricConnectivityCosts.jl:5-19
  AffineMonotonizedSymmetricConnectivityModel   MonotonizedSymmetricConnectivityCosts.jl:5-33
  AffineSymmetricEdgeCutModel                   SymmetricEdgeCutCosts.jl:5-18
  AffinePrimaryEdgeCutModel                     PrimaryEdgeCutCosts.jl:5-18
  AffineSecondaryEdgeCutModel                   SecondaryEdgeCutCosts.jl:5-18
  AffineEnvelopeModel                           EnvelopeCosts.jl:5-20

Julia's constructors `promote` all parameters to one element type (ConnectivityCosts.jl:14-16):
all-int arguments give an Int64 model, any float gives Float64.  Closures (e.g.
`w -> 1 + w`) cannot cross a C ABI, so callables are tabulated host-side for w = 0..w_table.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

CP_I64, CP_F64 = 0, 1
(CP_MODEL_FEASIBLE, CP_MODEL_WORK, CP_MODEL_CONNECTIVITY, CP_MODEL_HYPEREDGE_CUT,
 CP_MODEL_COLBLOCK, CP_MODEL_BLOCK, CP_MODEL_VERTEX_COUNT, CP_MODEL_POWER_WORK, CP_MODEL_PRIMARY,
 CP_MODEL_SECONDARY) = range(10)
CP_MODEL_SYM_CONNECTIVITY, CP_MODEL_MONO_SYM_CONNECTIVITY, CP_MODEL_SYM_EDGE_CUT = 10, 11, 12
CP_MODEL_PRIMARY_EDGE_CUT, CP_MODEL_SECONDARY_EDGE_CUT = 13, 14
CP_MODEL_ENVELOPE = 15
CP_COMBINE_SUM, CP_COMBINE_MAX = 0, 1
CP_ORDER_SPLITTER, CP_ORDER_CHUNKER = 0, 1
CP_MAX_R = 4
CP_OK, CP_EINVAL, CP_INFEASIBLE, CP_EHIP, CP_EUNSUPPORTED, CP_EINTERNAL = range(6)


class cp_component_t(C.Structure):
    _fields_ = [("is_const", C.c_int32), ("_pad", C.c_int32), ("c_i64", C.c_int64), ("c_f64", C.c_double),
                ("table", C.c_void_p), ("len", C.c_int64), ("lo", C.c_int64)]


class cp_model_t(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dtype", C.c_int32), ("p_i64", C.c_int64 * 5), ("p_f64", C.c_double * 5),
                ("alpha_k", C.c_void_p), ("n_alpha_k", C.c_int64), ("R", C.c_int32), ("_pad", C.c_int32),
                ("alpha_row", cp_component_t), ("alpha_col", cp_component_t),
                ("beta_row", cp_component_t * CP_MAX_R), ("beta_col", cp_component_t * CP_MAX_R)]


class cp_rowpart_t(C.Structure):
    _fields_ = [("K", C.c_int64), ("asg", C.c_void_p), ("spl", C.c_void_p)]


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) or isinstance(x, bool)


def _promote(*xs):
    """Julia promote(): Int64 iff every argument is an integer/bool."""
    flat = []
    for x in xs:
        if isinstance(x, (list, tuple, np.ndarray)):
            flat.extend(np.asarray(x).ravel().tolist())
        else:
            flat.append(x)
    return CP_I64 if all(_is_int(v) for v in flat) else CP_F64


class Marshalled:
    """A cp_model_t plus the numpy buffers it points into (kept alive together).  `rowpart`: the row partition of a call whose
    backend method has no argument for one (LazyBisectCost on a primary model), as (cp_rowpart_t, its buffers) in rowpart /
    rowpart_keep; None everywhere else.  The struct bytes do not know about it."""
    rowpart = None
    rowpart_keep = ()

    def __init__(self, struct, keep):
        self.struct = struct
        self.keep = keep

    @property
    def ptr(self):
        return C.byref(self.struct)

    _as_parameter_ = ptr     # what a `const cp_model_t *` parameter of the binding takes


class _Model:
    kind = None
    dtype = CP_I64
    fields = ()             # the attributes that fill cp_model_t.p_i64 / p_f64, in that order
    alpha_k = None          # per-part alpha[k], where the constructor takes it
    w_table = None          # tabulation length for callables; set via with_table()

    def cost_dtype(self):
        return np.int64 if self.dtype == CP_I64 else np.float64

    def _set(self, *values, alpha_k=None):
        """the constructor of an affine model: stores `values` under `fields` and promotes them all to one element type"""
        for name, v in zip(self.fields, values):
            setattr(self, name, v)
        self.alpha_k = alpha_k
        self.dtype = _promote(*values, *([alpha_k] if alpha_k is not None else []))

    def _params(self):
        return [getattr(self, name) for name in self.fields]

    def _alpha_k(self):
        return self.alpha_k

    def marshal(self, w_table=None, w_lo=0, u_table=None):
        """-> Marshalled.  w_lo .. w_table (u_table: the same for the row tables of the block model) is the range closures over
        the part width are tabulated for; nothing is written to the model."""
        s = cp_model_t()
        keep = []
        s.kind = self.kind
        s.dtype = self.dtype
        for i, v in enumerate(self._params()):
            if self.dtype == CP_I64:
                s.p_i64[i] = int(v)
            else:
                s.p_f64[i] = float(v)
        ak = self._alpha_k()
        if ak is not None:
            arr = np.ascontiguousarray(ak, dtype=self.cost_dtype())
            keep.append(arr)
            s.alpha_k = arr.ctypes.data
            s.n_alpha_k = arr.size
        self._marshal_extra(s, keep, w_table, w_lo, u_table)
        return Marshalled(s, keep)

    def _marshal_extra(self, s, keep, w_table, w_lo, u_table):
        pass


class AffineWorkModel(_Model):
    kind = CP_MODEL_WORK
    fields = ("alpha", "beta_vertex", "beta_pin")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_pins * self.beta_pin


class PowerWorkModel(_Model):
    """alpha + (n_vertices*beta_vertex + n_pins*beta_pin)^gamma, Float64: the ConvexWorkModel (gamma 0.8) and
    ConcaveWorkModel (gamma 2) of the reference's tests (test/test_Partitioners.jl:54-74)."""
    kind = CP_MODEL_POWER_WORK
    fields = ("alpha", "beta_vertex", "beta_pin", "gamma")

    def __init__(self, alpha, beta_vertex, beta_pin, gamma):
        self.alpha, self.beta_vertex, self.beta_pin, self.gamma = float(alpha), float(beta_vertex), float(beta_pin), float(gamma)
        self.alpha_k = None
        self.dtype = CP_F64

    def __call__(self, n_vertices, n_pins, k=None):
        x = n_vertices * self.beta_vertex + n_pins * self.beta_pin
        return self.alpha + (x * x if self.gamma == 2.0 else x ** self.gamma)


def ConvexWorkModel(alpha, beta_vertex, beta_pin):
    return PowerWorkModel(alpha, beta_vertex, beta_pin, 0.8)


def ConcaveWorkModel(alpha, beta_vertex, beta_pin):
    return PowerWorkModel(alpha, beta_vertex, beta_pin, 2.0)


class AffineConnectivityModel(_Model):
    """alpha + nv*beta_vertex + np*beta_pin + nets*beta_net.  `alpha_k` gives the per-part
    alpha[k] of the reference tests' FunkyConnectivityModel (test_Partitioners.jl:1-8)."""
    kind = CP_MODEL_CONNECTIVITY
    fields = ("alpha", "beta_vertex", "beta_pin", "beta_net")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, beta_net=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, beta_net, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, n_nets, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_pins * self.beta_pin + n_nets * self.beta_net


class AffineHyperedgeCutModel(_Model):
    kind = CP_MODEL_HYPEREDGE_CUT
    fields = ("alpha", "beta_vertex", "beta_pin", "beta_self_net", "beta_cut_net")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, beta_self_net=0, beta_cut_net=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, beta_self_net, beta_cut_net, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, n_self, n_cut, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return (a + n_vertices * self.beta_vertex + n_pins * self.beta_pin
                + n_self * self.beta_self_net + n_cut * self.beta_cut_net)


class AffinePrimaryConnectivityModel(_Model):
    """PrimaryConnectivityCosts.jl:5-20: nets of a column part split by the row partition Pi into local (owned by the same
    part number) and remote ones.  Needs Pi (any partition of the rows)."""
    kind = CP_MODEL_PRIMARY
    needs_rowpart = True
    fields = ("alpha", "beta_vertex", "beta_pin", "beta_local_net", "beta_remote_net")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, beta_local_net=0, beta_remote_net=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, beta_local_net, beta_remote_net, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, n_local, n_remote, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_pins * self.beta_pin + n_local * self.beta_local_net + n_remote * self.beta_remote_net


class AffineSecondaryConnectivityModel(AffinePrimaryConnectivityModel):
    """SecondaryConnectivityCosts.jl:5-20: the cost of giving a range of columns to part k of the SplitPartition Pi of the
    rows -- the alternating partitioners call it on the adjoint, with Pi the column split found in the previous sweep."""
    kind = CP_MODEL_SECONDARY


# ---------------------------------------------------------------- the symmetric family (square patterns, one partition for
# rows and columns; HIP backend only)
class AffineSymmetricConnectivityModel(_Model):
    """SymmetricConnectivityCosts.jl:5-19: alpha + nv*beta_vertex + np*beta_pin + local*beta_local_net + remote*beta_remote_net with
    remote = dianet(j, j') - nv (the nets of the part that reach outside its own rows) and local = net(j, j') - remote.
    `alpha_k` gives a per-part alpha[k], as for the monotonized model."""
    kind = CP_MODEL_SYM_CONNECTIVITY
    symmetric = True
    fields = ("alpha", "beta_vertex", "beta_pin", "beta_local_net", "beta_remote_net")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, beta_local_net=0, beta_remote_net=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, beta_local_net, beta_remote_net, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, n_local, n_remote, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return (a + n_vertices * self.beta_vertex + n_pins * self.beta_pin + n_local * self.beta_local_net
                + n_remote * self.beta_remote_net)


def _cld(a, b):
    """Julia cld: Int for Ints (exact), ceil(a / b) for floats"""
    if _is_int(a) and _is_int(b):
        return -((-int(a)) // int(b))
    return float(np.ceil(a / b))


class AffineMonotonizedSymmetricConnectivityModel(_Model):
    """MonotonizedSymmetricConnectivityCosts.jl:5-33: alpha + nv*beta_vertex + overpins*beta_over_pin + dianet(j, j')*beta_dia_net,
    overpins = sum of max(deg - delta_pins, 0) over the part's columns; every term grows with the part.  Positional, keyword
    (:13-15) and converting (from an AffineSymmetricConnectivityModel, :17-29) constructors.  `alpha_k` gives the per-part alpha[k]
    of the reference tests' FunkyMonotonizedSymmetricConnectivityModel (test_Partitioners.jl:12-22).  delta_pins must be
    integer-valued (the reference keeps the over-pin prefix in an integer vector)."""
    kind = CP_MODEL_MONO_SYM_CONNECTIVITY
    symmetric = True
    fields = ("alpha", "beta_vertex", "beta_over_pin", "beta_dia_net", "delta_pins")

    def __init__(self, alpha=0, beta_vertex=0, beta_over_pin=0, beta_dia_net=0, delta_pins=0, *, alpha_k=None):
        if isinstance(alpha, AffineSymmetricConnectivityModel):
            if (beta_vertex, beta_over_pin, beta_dia_net, delta_pins) != (0, 0, 0, 0):
                raise TypeError("the converting constructor takes the symmetric model alone")
            s = alpha
            zero = 0 if s.dtype == CP_I64 else 0.0
            alpha, beta_dia_net, beta_over_pin = s.alpha, s.beta_remote_net, s.beta_pin
            if s.beta_vertex < s.beta_remote_net:
                delta_pins, beta_vertex = _cld(s.beta_remote_net - s.beta_vertex, s.beta_pin), zero
            else:
                delta_pins, beta_vertex = 0, s.beta_vertex - s.beta_remote_net
            if s.dtype == CP_F64:                    # the struct is {Tv}: every field converts to the model's element type
                alpha, beta_vertex, beta_over_pin, beta_dia_net, delta_pins = (float(v) for v in (alpha, beta_vertex, beta_over_pin, beta_dia_net, delta_pins))
        self._set(alpha, beta_vertex, beta_over_pin, beta_dia_net, delta_pins, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_over_pins, n_dia_nets, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_over_pins * self.beta_over_pin + n_dia_nets * self.beta_dia_net


class AffineSymmetricEdgeCutModel(_Model):
    """SymmetricEdgeCutCosts.jl:5-18: alpha + nv*beta_vertex + selfpin(j, j')*beta_self_pin + (np - selfpin)*beta_cut_pin,
    selfpin = nonzeros of the part's diagonal block.  `alpha_k` gives a per-part alpha[k]."""
    kind = CP_MODEL_SYM_EDGE_CUT
    symmetric = True
    fields = ("alpha", "beta_vertex", "beta_self_pin", "beta_cut_pin")

    def __init__(self, alpha=0, beta_vertex=0, beta_self_pin=0, beta_cut_pin=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_self_pin, beta_cut_pin, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_self_pins, n_cut_pins, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_self_pins * self.beta_self_pin + n_cut_pins * self.beta_cut_pin


# ---------------------------------------------------------------- the plaid edge-cut pair (HIP backend only)
class AffinePrimaryEdgeCutModel(_Model):
    """PrimaryEdgeCutCosts.jl:5-18: alpha + nv*beta_vertex + self*beta_self_pin + cut*beta_cut_pin, the pins of a column part split
    by the row partition Pi into self pins (row owned by the same part number) and cut pins.  Needs Pi (any partition of the
    rows).  `alpha_k` gives a per-part alpha[k]."""
    kind = CP_MODEL_PRIMARY_EDGE_CUT
    needs_rowpart = True
    hip_only = True
    fields = ("alpha", "beta_vertex", "beta_self_pin", "beta_cut_pin")

    def __init__(self, alpha=0, beta_vertex=0, beta_self_pin=0, beta_cut_pin=0, *, alpha_k=None):
        self._set(alpha, beta_vertex, beta_self_pin, beta_cut_pin, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_self_pins, n_cut_pins, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_self_pins * self.beta_self_pin + n_cut_pins * self.beta_cut_pin


class AffineSecondaryEdgeCutModel(AffinePrimaryEdgeCutModel):
    """SecondaryEdgeCutCosts.jl:5-18: the cost of giving a range of columns to part k of the SplitPartition Pi of the rows; the
    vertices and pins are those of the part of Pi, the self pins the entries of the range in its rows."""
    kind = CP_MODEL_SECONDARY_EDGE_CUT


# ---------------------------------------------------------------- the envelope cost (HIP backend only)
class AffineEnvelopeModel(_Model):
    """EnvelopeCosts.jl:5-20: alpha + nv*beta_vertex + np*beta_pin + d*beta_net, d = max(hi - lo, 0) the span between the least
    first row and the greatest last row of the part's columns (rowenvelope, EnvelopeMatrices.jl:10-57).  Positional or keyword
    form with zero defaults (:12-14).  `alpha_k` gives a per-part alpha[k]: the reference's 4-argument fallback (:3) makes the
    part number meaningful.  A row partition passed along is accepted and ignored (Costs.jl:5-7, :17-19)."""
    kind = CP_MODEL_ENVELOPE
    hip_only = True
    fields = ("alpha", "beta_vertex", "beta_pin", "beta_net")

    def __init__(self, alpha=0, beta_vertex=0, beta_pin=0, beta_net=0, alpha_k=None):
        self._set(alpha, beta_vertex, beta_pin, beta_net, alpha_k=alpha_k)

    def __call__(self, n_vertices, n_pins, n_nets, k=None):
        a = self.alpha if self.alpha_k is None or k is None else self.alpha_k[k - 1]
        return a + n_vertices * self.beta_vertex + n_pins * self.beta_pin + n_nets * self.beta_net


def _tabulate(f, lo, hi, npdt):
    """f(w) for w = lo .. hi; vectorised when the callable allows it, checked against three scalar calls."""
    ws = np.arange(lo, hi + 1, dtype=np.int64)
    try:
        tab = np.asarray(f(ws))
        if tab.shape == ws.shape and all(tab[i] == f(int(ws[i])) for i in (0, len(ws) // 2, len(ws) - 1)):
            return tab.astype(npdt)
    except Exception:
        pass
    return np.array([f(int(w)) for w in ws], dtype=npdt)


def _component(f, dtype, w_table, keep, w_lo=0):
    """block_component(f, w) (BlockCosts.jl:41-44): number | callable | tuple/array (1-based).
    Callables are tabulated for w = w_lo .. w_table (w_lo < 0: see cp_component_t in include/chainpart_types.h)."""
    c = cp_component_t()
    npdt = np.int64 if dtype == CP_I64 else np.float64
    if callable(f):
        if w_table is None:
            raise ValueError("a callable block component needs w_table (tabulation length)")
        tab = _tabulate(f, w_lo, w_table, npdt)
        c.lo = int(w_lo)
    elif isinstance(f, (list, tuple, np.ndarray)):
        arr = np.asarray(f)
        tab = np.concatenate([[0], arr]).astype(npdt)   # Julia f[w], w >= 1
    else:
        c.is_const = 1
        if dtype == CP_I64:
            c.c_i64 = int(f)
        else:
            c.c_f64 = float(f)
        return c
    tab = np.ascontiguousarray(tab)
    keep.append(tab)
    c.is_const = 0
    c.table = tab.ctypes.data
    c.len = tab.size
    return c


class ColumnBlockComponentCostModel(_Model):
    """1-D VBR cost alpha_col(w) + nets * beta_col(w); an AbstractConnectivityModel (BlockCosts.jl:1-17)."""
    kind = CP_MODEL_COLBLOCK

    def __init__(self, alpha_col=0, beta_col=0, dtype=int, w_table=None):
        self.alpha_col, self.beta_col = alpha_col, beta_col
        self.dtype = CP_I64 if dtype in (int, np.int64, "int", CP_I64) else CP_F64
        self.w_table = w_table

    def _marshal_extra(self, s, keep, w_table, w_lo, u_table):
        wt = w_table if w_table is not None else self.w_table
        s.R = 1
        s.alpha_col = _component(self.alpha_col, self.dtype, wt, keep, w_lo)
        s.beta_col[0] = _component(self.beta_col, self.dtype, wt, keep, w_lo)

    def __call__(self, n_vertices, n_pins, n_nets, k=None):
        bc = lambda f, w: f(w) if callable(f) else (f[w - 1] if isinstance(f, (list, tuple, np.ndarray)) else f)
        return bc(self.alpha_col, n_vertices) + n_nets * bc(self.beta_col, n_vertices)


class BlockComponentCostModel(_Model):
    """Rank-R separable 2-D VBR cost (BlockCosts.jl:19-44); needs a row partition Pi."""
    kind = CP_MODEL_BLOCK

    def __init__(self, alpha_row=0, alpha_col=0, beta_row=(), beta_col=(), dtype=int, w_table=None, u_table=None):
        assert len(beta_row) == len(beta_col) <= CP_MAX_R
        self.alpha_row, self.alpha_col = alpha_row, alpha_col
        self.beta_row, self.beta_col = tuple(beta_row), tuple(beta_col)
        self.dtype = CP_I64 if dtype in (int, np.int64, "int", CP_I64) else CP_F64
        self.w_table, self.u_table = w_table, u_table

    def _marshal_extra(self, s, keep, w_table, w_lo, u_table):
        wt = w_table if w_table is not None else self.w_table
        ut = u_table if u_table is not None else self.u_table if self.u_table is not None else wt
        s.R = len(self.beta_row)
        s.alpha_row = _component(self.alpha_row, self.dtype, ut, keep)
        s.alpha_col = _component(self.alpha_col, self.dtype, wt, keep, w_lo)
        for r in range(s.R):
            s.beta_row[r] = _component(self.beta_row[r], self.dtype, ut, keep)
            s.beta_col[r] = _component(self.beta_col[r], self.dtype, wt, keep, w_lo)


class VertexCount(_Model):
    """w(j, j') = j' - j, always Int (SparseColorArrays.jl:1-6)."""
    kind = CP_MODEL_VERTEX_COUNT
    dtype = CP_I64


class FeasibleCost(_Model):
    kind = CP_MODEL_FEASIBLE
    dtype = CP_I64


class ConstrainedCost:
    """ConstrainedCost(f, w, w_max): f where w(j, j') <= w_max, infinity elsewhere (Costs.jl:105-147)."""

    def __init__(self, f, w, w_max):
        self.f, self.w, self.w_max = f, w, w_max


def split_constraint(f):
    """-> (model, weight | None, w_max)"""
    if isinstance(f, ConstrainedCost):
        if isinstance(f.w, FeasibleCost):
            return f.f, None, 0
        return f.f, f.w, f.w_max
    return f, None, 0


# ---------------------------------------------------------------- methods
class EquiSplitter:
    pass


class EquiChunker:
    def __init__(self, w):
        self.w = int(w)


class StrictChunker:
    """StrictChunker.jl:1-3: greedy parts of identical columns, at most w_max wide (w_max < 1: no limit)."""

    def __init__(self, w_max):
        self.w_max = int(w_max)


class OverlapChunker:
    """OverlapChunker.jl:1-4: greedy parts whose columns overlap the part's first column by the fraction rho, at most w_max wide."""

    def __init__(self, rho, w_max):
        self.rho, self.w_max = float(rho), int(w_max)


class _FMethod:
    def __init__(self, f):
        self.f = f


class DynamicTotalSplitter(_FMethod):
    combine, order = CP_COMBINE_SUM, CP_ORDER_SPLITTER


class DynamicBottleneckSplitter(_FMethod):
    combine, order = CP_COMBINE_MAX, CP_ORDER_SPLITTER


class DynamicTotalChunker(_FMethod):
    combine, order = CP_COMBINE_SUM, CP_ORDER_CHUNKER


class DynamicBottleneckChunker(_FMethod):
    combine, order = CP_COMBINE_MAX, CP_ORDER_CHUNKER


class ReferenceTotalSplitter(DynamicTotalSplitter):
    """ReferenceSplitter.jl:1-6: invokes the generic DynamicTotalSplitter method."""


class ReferenceBottleneckSplitter(DynamicBottleneckSplitter):
    """ReferenceSplitter.jl:8-13"""


class ReferenceTotalChunker(DynamicTotalChunker):
    """ReferenceSplitter.jl:16-21"""


class BisectCostBottleneckSplitter:
    flip = 0

    def __init__(self, f, eps):
        self.f, self.eps = f, float(eps)


class FlipBisectCostBottleneckSplitter(BisectCostBottleneckSplitter):
    flip = 1


class BisectIndexBottleneckSplitter:
    """BisectIndexBottleneckSplitter.jl:1-83 (exact bottleneck by bisection over split indices)"""
    flip = 0

    def __init__(self, f):
        self.f = f


class FlipBisectIndexBottleneckSplitter(BisectIndexBottleneckSplitter):
    """BisectIndexBottleneckSplitter.jl:85-166"""
    flip = 1


class LazyBisectCostBottleneckSplitter:
    """LazyBisectCostBottleneckSplitter.jl:1-4, connectivity specialisation :140-258, monotonized symmetric one :260-388, and the
    one for an AffinePrimaryConnectivityModel under a row partition, partition_stripe(A, K, method, Pi), :390-483 (HIP backend
    only; Pi is any partition of the rows with at most K parts)"""

    def __init__(self, f, eps):
        self.f, self.eps = f, float(eps)


class LazyFlipBisectCostBottleneckSplitter:
    """LazyBisectCostBottleneckSplitter.jl:72-138, for decreasing costs: partition_stripe(A, K, method, [Pi]) with a connectivity
    model (per-part alpha included), an AffinePrimaryConnectivityModel under a row partition with at most K parts, or an
    AffineSecondaryConnectivityModel under a SplitPartition of the rows with exactly K parts (HIP backend only)"""

    def __init__(self, f, eps):
        self.f, self.eps = f, float(eps)


class MagneticPartitioner:
    """MagneticPartitioner.jl:1-20: partition_stripe(A, K, method, Pi) -> MapPartition; column j with d entries takes the part of
    the row of its entry number u_j mod d, a column without entries the part 1 + u_j mod K.  draws: the n values u_j >= 0 that
    stand for the reference's rand calls; None: u_j = draws.draw(seed, 1, j), computed on the device."""

    def __init__(self, seed=0, draws=None):
        self.seed = int(seed)
        self.draws = None if draws is None else np.ascontiguousarray(draws, dtype=np.int64)


class GreedyBottleneckPartitioner:
    """MagneticPartitioner.jl:22-177: partition_stripe(A, K, method, Pi) -> MapPartition; the columns are visited in `order` and
    each takes the part of largest current cost among its rows' parts, whose cost then falls.  mdl: an
    AffineSecondaryConnectivityModel (the reference has no method for another model).  order: a permutation of 1 .. n (an int64
    array or a DomainPermutation) that stands for the reference's randperm(n); None: the columns ascending by
    (draws.draw(seed, 2, j), j), sorted on the device."""

    def __init__(self, mdl, seed=0, order=None):
        self.mdl, self.seed = mdl, int(seed)
        if order is not None and hasattr(order, "prm"):
            order = order.prm
        self.order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)


class DisjointPartitioner:
    """AlternatingPartitioner.jl:1-10: columns first, then the rows of the adjoint given the column split."""

    def __init__(self, mtd, mtd2):
        self.mtd, self.mtd2 = mtd, mtd2


class AlternatingPartitioner:
    """AlternatingPartitioner.jl:12-32: Phi on A, Pi on the adjoint given Phi, then alternately again."""

    def __init__(self, *mtds):
        assert len(mtds) >= 2
        self.mtds = tuple(mtds)


class AlternatingNetPartitioner(AlternatingPartitioner):
    """AlternatingPartitioner.jl:34-58: same sweeps, sharing one net counter of A (the device keeps A's link arrays anyway)."""

    def __init__(self, *mtds, hint=None):
        super().__init__(*mtds)
        self.hint = hint


class SymmetricPartitioner:
    """AlternatingPartitioner.jl:60-87: one partition for rows and columns of a square matrix."""

    def __init__(self, *mtds):
        assert len(mtds) >= 1
        self.mtds = tuple(mtds)


class AlternatingPacker:
    """AlternatingPacker.jl:12-32: pack_stripe for Phi on A, for Pi on the adjoint given Phi, then alternately again."""

    def __init__(self, *mtds):
        assert len(mtds) >= 2
        self.mtds = tuple(mtds)


class SymmetricPacker:
    """AlternatingPacker.jl:34-53: one packing for rows and columns, refined on A and its adjoint in turn."""

    def __init__(self, *mtds):
        assert len(mtds) >= 1
        self.mtds = tuple(mtds)


class ConvexTotalChunker(_FMethod):
    pass


class ConvexTotalSplitter(_FMethod):
    pass


class ConcaveTotalChunker(_FMethod):
    """ConcaveTotalChunker.jl:1-24"""


class ConcaveTotalSplitter(_FMethod):
    """ConcaveTotalChunker.jl:5-55, :140-180"""


# ---------------------------------------------------------------- reordering (Permutations.jl:31, CuthillMcKeePermuter.jl:1-5,199, PermutingPartitioner.jl:1-4)
class IdentityPermuter:
    pass


class CuthillMcKeePermuter:
    """reverse: the queue backwards; assumesymmetry: walk the columns of a square pattern as they are; checksymmetry: walk them if
    the pattern equals its adjoint, else the bipartite graph of rows and columns"""

    def __init__(self, reverse=False, assumesymmetry=False, checksymmetry=True):
        self.reverse, self.assumesymmetry, self.checksymmetry = bool(reverse), bool(assumesymmetry), bool(checksymmetry)


class PermutingPartitioner:
    """order with prm, permute, partition with prt, map the partition back"""

    def __init__(self, prm, prt):
        self.prm, self.prt = prm, prt
