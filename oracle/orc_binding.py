"""ctypes binding of the TEST ORACLE (oracle/liborc.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py -- never by the product package.  It implements the same
`backend` interface as chainpartitioners.jl_amd._lib.HipBackend so the host-side API
(api.partition_stripe etc.) can drive either on identical marshalled inputs.

SIGNATURES declares the prototypes of oracle/orc.h that are called from here; lib() applies them.  The two argument classes
are a copy of the product binding's idea on purpose: this file loads without the package, and the package never loads this.
"""
import ctypes as C
import os
import subprocess
from functools import partial

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, "liborc.so")
    srcs = [os.path.join(_HERE, f) for f in ("orc_counts.c", "orc_i64.c", "orc_f64.c", "orc_api.c",
                                             "orc_algos.inc", "orc.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", _HERE, "liborc.so"], stdout=subprocess.DEVNULL)
    return so


class _Array:
    """`T *name`: None (NULL) or a C-contiguous numpy array of exactly this element type"""

    def __init__(self, dtype, name):
        self.dtype, self.name = np.dtype(dtype), name

    def from_param(self, a):
        if a is None:
            return None
        if not (isinstance(a, np.ndarray) and a.dtype == self.dtype and a.flags.c_contiguous):
            raise TypeError(f"{self.name}: expected None or a C-contiguous {self.dtype.name} array, got {getattr(a, 'dtype', type(a).__name__)}")
        return C.c_void_p(a.ctypes.data)


class _Struct:
    """`const cp_model_t *name` / `const cp_rowpart_t *name`: None, a ctypes struct, or what carries one as `.struct` (the
    package's Marshalled); the struct types themselves belong to the package"""

    def __init__(self, name):
        self.name = name

    def from_param(self, x):
        x = getattr(x, "struct", x)
        if x is not None and not isinstance(x, C.Structure):
            raise TypeError(f"{self.name}: expected None or a ctypes struct, got {type(x).__name__}")
        return None if x is None else C.byref(x)


_I64, _I32, _F64 = (partial(_Array, t) for t in (np.int64, np.int32, np.float64))
_i32, _i64, _f64, _vp = C.c_int32, C.c_int64, C.c_double, C.c_void_p
_pi64, _pf64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
_CSC = [_i64, _i64, _i64, _I64("pos"), _I64("idx")]                    # m, n, N, pos, idx: what every entry takes for A
_MDL, _PI, _WEIGHT = _Struct("mdl"), _Struct("Pi"), _Struct("weight")
_CONSTRAINT = [_WEIGHT, _i64, _f64]
_BOUNDS = [_pi64, _pi64, _pf64, _pf64]
_COSTS = [_I64("cst_i64"), _F64("cst_f64")]
_PACK = (_i32, [*_CSC, _MDL, _PI, *_CONSTRAINT, _I64("spl_out"), _I64("K_out")])
_SPLIT = (_i32, [*_CSC, _i64, _MDL, _PI, *_CONSTRAINT, _I64("spl_out")])

SIGNATURES = {
    "orc_dom_build": (_vp, [_i32, *_CSC, _i64, _i64, _i64]),
    "orc_dom_query": (_i64, [_vp, _i64, _i64]),
    "orc_dom_step": (_i64, [_vp, _i32, _i64, _i32, _i64]),
    "orc_dom_free": (None, [_vp]),
    "orc_netcount_build": (_vp, [_i32, *_CSC]),
    "orc_selfnetcount_build": (_vp, [_i32, *_CSC]),
    "orc_net_query": (_i64, [_vp, _i64, _i64]),
    "orc_net_step": (_i64, [_vp, _i32, _i64, _i32, _i64]),
    "orc_net_free": (None, [_vp]),
    "orc_net_link_array": (None, [*_CSC, _I64("out")]),
    "orc_partwise": (_i64, [*_CSC, _i64, _I64("asg"), _I64("pios_out"), _I64("prm_out"), _I64("pos_out"), _I64("idx_out")]),
    "orc_oracle_eval": (_i32, [*_CSC, _MDL, _PI, _i32, _i64, _I64("j"), _I64("jp"), _I64("k"), _I64("out_i64"), _F64("out_f64")]),
    "orc_oracle_step": (_i32, [*_CSC, _MDL, _PI, _i64, _I32("move_j"), _I64("j"), _I32("move_jp"), _I64("jp"), _I64("k"),
                               _I64("out_i64"), _F64("out_f64")]),
    "orc_bound_stripe": (_i32, [*_CSC, _i64, _MDL, *_BOUNDS]),
    "orc_bound_stripe_pi": (_i32, [*_CSC, _i64, _PI, _MDL, *_BOUNDS]),
    "orc_objective": (_i32, [*_CSC, _i64, _I64("spl"), _MDL, _PI, _i32, _pi64, _pf64]),
    "orc_partition_dynamic": (_i32, [*_CSC, _i64, _i32, _i32, _MDL, _PI, *_CONSTRAINT, _I64("spl_out")]),
    "orc_pack_dynamic": _PACK,
    "orc_partition_bisect_cost": (_i32, [*_CSC, _i64, _MDL, _PI, _f64, _i32, _I64("spl_out"), _I64("n_probes_out")]),
    "orc_partition_bisect_index": (_i32, [*_CSC, _i64, _MDL, _PI, _i32, _I64("spl_out"), _I64("n_probes_out")]),
    "orc_partition_lazy_bisect_cost": (_i32, [*_CSC, _i64, _MDL, _f64, _I64("spl_out"), _I64("n_probes_out")]),
    "orc_pack_convex": _PACK,
    "orc_partition_convex": _SPLIT,
    "orc_pack_concave": _PACK,
    "orc_partition_concave": _SPLIT,
    "orc_partition_equi": (None, [_i64, _i64, _I64("spl_out")]),
    "orc_pack_equi": (_i64, [_i64, _i64, _I64("spl_out")]),
    "orc_dynamic_tables": (_i32, [*_CSC, _i64, _i32, _MDL, _PI, _I64("ptr_out"), *_COSTS]),
    "orc_dynamic_tables_constrained": (_i32, [*_CSC, _i64, _i32, _MDL, _PI, *_CONSTRAINT, _I64("win_lo"), _I64("win_hi"),
                                              _I64("ptr_out"), *_COSTS]),
}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(_LIB, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _LIB


def _cost_zeros(mm, shape):
    return np.zeros(shape, dtype=np.int64 if mm.struct.dtype == 0 else np.float64)


def _by_type(a):
    """the `int64_t *x_i64, double *x_f64` pair: a and NULL, by a's element type"""
    return (None, a) if a.dtype == np.float64 else (a, None)


class OracleBackend:
    name = "oracle"

    def last_error(self):
        return ""

    def _A(self, A):
        return (A.m, A.n, A.nnz, A.colptr, A.rowval)

    def partition_dynamic(self, A, K, combine, order, mm, rp, wm, wi, wf, spl):
        return lib().orc_partition_dynamic(*self._A(A), K, combine, order, mm, rp, wm, wi, wf, spl)

    def pack_dynamic(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return lib().orc_pack_dynamic(*self._A(A), mm, rp, wm, wi, wf, spl, Kout)

    def adjoint(self, A):
        """adjointpattern(A): CSC transpose of the pattern by a stable counting sort (util.jl:67-95)."""
        m, n = A.shape
        cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), np.diff(A.colptr))
        order = np.argsort(A.rowval, kind="stable")
        cnt = np.bincount(A.rowval - 1, minlength=m)
        pos = np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int64)
        return type(A)(n, m, pos, cols[order])

    def _probed(self, fn, *args):
        """the bisection entries also report how many probes they ran: kept in last_probes"""
        pr = np.zeros(1, dtype=np.int64)
        rc = fn(*args, pr)
        self.last_probes = int(pr[0])
        return rc

    def partition_bisect_index(self, A, K, mm, flip, spl, rp=None):
        return self._probed(lib().orc_partition_bisect_index, *self._A(A), K, mm, rp, flip, spl)

    def partition_lazy_bisect_cost(self, A, K, mm, eps, spl):
        return self._probed(lib().orc_partition_lazy_bisect_cost, *self._A(A), K, mm, eps, spl)

    def partition_bisect_cost(self, A, K, mm, eps, flip, spl, rp=None):
        return self._probed(lib().orc_partition_bisect_cost, *self._A(A), K, mm, rp, eps, flip, spl)

    def pack_convex(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return lib().orc_pack_convex(*self._A(A), mm, rp, wm, wi, wf, spl, Kout)

    def partition_convex(self, A, K, mm, rp, wm, wi, wf, spl):
        return lib().orc_partition_convex(*self._A(A), K, mm, rp, wm, wi, wf, spl)

    def pack_concave(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return lib().orc_pack_concave(*self._A(A), mm, rp, wm, wi, wf, spl, Kout)

    def partition_concave(self, A, K, mm, rp, wm, wi, wf, spl):
        return lib().orc_partition_concave(*self._A(A), K, mm, rp, wm, wi, wf, spl)

    def oracle_eval(self, A, mm, rp, hint, j, jp, k, out):
        return lib().orc_oracle_eval(*self._A(A), mm, rp, hint, j.size, j, jp, k, *_by_type(out))

    def oracle_step(self, A, mm, rp, mj, j, mjp, jp, k, out):
        return lib().orc_oracle_step(*self._A(A), mm, rp, j.size, mj, j, mjp, jp, k, *_by_type(out))

    def _bounds(self, fn, mm, *args):
        li, hi, lf, hf = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        rc = fn(*args, C.byref(li), C.byref(hi), C.byref(lf), C.byref(hf))
        if mm.struct.dtype == 0:
            return rc, li.value, hi.value
        return rc, lf.value, hf.value

    def bound_stripe(self, A, K, mm):
        return self._bounds(lib().orc_bound_stripe, mm, *self._A(A), K, mm)

    def bound_stripe_pi(self, A, K, rp, mm):
        return self._bounds(lib().orc_bound_stripe_pi, mm, *self._A(A), K, rp, mm)

    def objective(self, A, K, spl, mm, rp, g):
        oi, of = C.c_int64(), C.c_double()
        rc = lib().orc_objective(*self._A(A), K, spl, mm, rp, g, C.byref(oi), C.byref(of))
        return rc, (oi.value if mm.struct.dtype == 0 else of.value)

    def dynamic_tables(self, A, K, combine, mm, rp):
        ptr = np.zeros((K, A.n + 1), dtype=np.int64)       # column-major (n+1) x K
        cst = _cost_zeros(mm, (K, A.n + 1))
        rc = lib().orc_dynamic_tables(*self._A(A), K, combine, mm, rp, ptr, *_by_type(cst))
        return rc, ptr.T, cst.T                               # [j', k] views

    def dynamic_tables_constrained(self, A, K, combine, mm, rp, wm, wi, wf):
        """(rc, j'_lo[K], j'_hi[K], ptr[j', k], cst[j', k]) of the ConstrainedCost splitter, tables densified"""
        ptr = np.zeros((K, A.n + 1), dtype=np.int64)
        cst = _cost_zeros(mm, (K, A.n + 1))
        lo = np.zeros(K, dtype=np.int64); hi = np.zeros(K, dtype=np.int64)
        rc = lib().orc_dynamic_tables_constrained(*self._A(A), K, combine, mm, rp, wm, wi, wf, lo, hi, ptr, *_by_type(cst))
        return rc, lo, hi, ptr.T, cst.T

    # counting structures
    def count_build(self, kind, A, hint, b=0, H=0, bp=0):
        L = lib()
        if kind == "net":
            return C.c_void_p(L.orc_netcount_build(hint, *self._A(A)))
        if kind == "selfnet":
            return C.c_void_p(L.orc_selfnetcount_build(hint, *self._A(A)))
        return C.c_void_p(L.orc_dom_build(hint, *self._A(A), b, H, bp))

    def count_query(self, kind, h, a, b, out):
        L = lib()
        f = L.orc_dom_query if kind == "dom" else L.orc_net_query
        for t in range(a.size):
            out[t] = f(h, a[t], b[t])
        return 0

    def count_step(self, kind, h, ma, a, mb, b):
        L = lib()
        f = L.orc_dom_step if kind == "dom" else L.orc_net_step
        return f(h, ma, a, mb, b)

    def count_free(self, kind, h):
        L = lib()
        (L.orc_dom_free if kind == "dom" else L.orc_net_free)(h)

    def link_array(self, A):
        out = np.zeros(A.nnz, dtype=np.int64)
        lib().orc_net_link_array(*self._A(A), out)
        return out

    def partwise(self, A, K, asg):
        asg = np.ascontiguousarray(asg, dtype=np.int64)
        pios = np.zeros(K + 1, dtype=np.int64)
        prm = np.zeros(max(A.nnz, 1), dtype=np.int64)
        pos = np.zeros(A.nnz + 1, dtype=np.int64)
        idx = np.zeros(max(A.nnz, 1), dtype=np.int64)
        npr = lib().orc_partwise(*self._A(A), K, asg, pios, prm, pos, idx)
        return int(npr), pios, prm[:npr].copy(), pos[:npr + 1].copy(), idx[:A.nnz].copy()
