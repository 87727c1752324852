"""ctypes binding of the product C-ABI library libchainpart.so (HIP, gfx950).

No fallback of any kind lives here: if the shared object is missing, or no HIP device is
visible, construction raises.  The symbols bound are exactly those of include/chainpart.h:
SIGNATURES declares each prototype once, load_library() applies it, and the argument classes
below check at the boundary what C cannot (element type and contiguity of every host array).
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partial
import weakref

import numpy as np

from . import models as M

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CP_LIB_PATH") or os.path.join(_HERE, "libchainpart.so")   # CP_LIB_PATH: A/B builds only


class _Array:
    """`T *name` over caller-owned host memory: None (NULL) or a C-contiguous numpy array of exactly this element type."""

    def __init__(self, dtype, name):
        self.dtype, self.name, self.what = np.dtype(dtype), name, np.dtype(dtype).name

    def _accepts(self, a):
        return a.dtype == self.dtype

    def from_param(self, a):
        if a is None:
            return None
        if not (isinstance(a, np.ndarray) and self._accepts(a) and a.flags.c_contiguous):
            got = f"{'' if a.flags.c_contiguous else 'non-contiguous '}{a.dtype} array" if isinstance(a, np.ndarray) else type(a).__name__
            raise TypeError(f"{self.name}: expected None or a C-contiguous {self.what} array, got {got}")
        return C.c_void_p(a.ctypes.data)


class _Words(_Array):
    """`const void *name`: 8-byte elements whose type another argument gives (the weights of cp_domsum_build / cp_rook_build)."""

    def __init__(self, name):
        self.dtype, self.name, self.what = None, name, "8-byte-element"

    def _accepts(self, a):
        return a.dtype.itemsize == 8


_I64, _I32, _F64 = (partial(_Array, t) for t in (np.int64, np.int32, np.float64))
_i32, _i64, _f64, _vp, _str = C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_char_p   # handles and device pointers: c_void_p
_pi32, _pi64, _pf64, _pvp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_void_p)    # out scalars
_MODEL, _ROWPART = C.POINTER(M.cp_model_t), C.POINTER(M.cp_rowpart_t)     # take the struct, byref(struct), a Marshalled or None
_PACK = (_i32, [_vp, _MODEL, _ROWPART, _MODEL, _i64, _f64, _I64("spl_out"), _I64("K_out")])
_SPLIT = (_i32, [_vp, _i64, _MODEL, _ROWPART, _MODEL, _i64, _f64, _I64("spl_out")])

# every function of include/chainpart.h: name -> (restype, argtypes); tests/test_abi_and_host.py holds it against the header
SIGNATURES = {
    "cp_last_error": (_str, []),
    "cp_version": (_i32, []),
    "cp_device_count": (_i32, []),
    "cp_csr_create": (_i32, [_i64, _i64, _i64, _I64("colptr"), _I64("rowval"), _i32, _pvp]),
    "cp_csr_create_device": (_i32, [_i64, _i64, _i64, _vp, _vp, _i32, _pvp]),
    "cp_csr_destroy": (_i32, [_vp]),
    "cp_adjoint": (_i32, [_vp, _pvp]),
    "cp_csr_download": (_i32, [_vp, _I64("dims_out"), _I64("colptr_out"), _I64("rowval_out")]),
    "cp_csr_reset_cache": (_i32, [_vp]),
    "cp_rcm": (_i32, [_vp, _vp, _i32, _i32, _I64("rowprm_out"), _I64("colprm_out"), _I64("stats_out")]),
    "cp_csr_permute": (_i32, [_vp, _I64("rowprm"), _I64("colprm"), _pvp]),
    "cp_csr_quotient": (_i32, [_vp, _ROWPART, _pvp]),
    "cp_count_build": (_i32, [_vp, _i32, _i32, _pvp]),
    "cp_count_query": (_i32, [_vp, _i64, _I64("a"), _I64("b"), _I64("out")]),
    "cp_count_destroy": (_i32, [_vp]),
    "cp_link_array": (_i32, [_vp, _I64("out")]),
    "cp_envelope_build": (_i32, [_vp, _pvp]),
    "cp_envelope_query": (_i32, [_vp, _i64, _I64("j"), _I64("jp"), _I64("lo_out"), _I64("hi_out")]),
    "cp_envelope_tree": (_i32, [_vp, _I64("dims_out"), _I64("tree_out")]),
    "cp_envelope_destroy": (_i32, [_vp]),
    "cp_domsum_build": (_i32, [_vp, _i32, _Words("val"), _pvp]),
    "cp_rook_build": (_i32, [_i64, _I64("idx"), _i32, _Words("val"), _i32, _pvp]),
    "cp_wsum_query": (_i32, [_vp, _i64, _I64("i"), _I64("j"), _I64("count_out"), _I64("sum_i64"), _F64("sum_f64")]),
    "cp_wsum_destroy": (_i32, [_vp]),
    "cp_partwise": (_i32, [_vp, _i64, _I64("asg"), _pi64, _I64("pios_out"), _I64("prm_out"), _I64("pos_out"), _I64("idx_out")]),
    "cp_oracle_eval": (_i32, [_vp, _MODEL, _ROWPART, _i32, _i64, _I64("j"), _I64("jp"), _I64("k"), _I64("out_i64"), _F64("out_f64")]),
    "cp_oracle_step": (_i32, [_vp, _MODEL, _ROWPART, _i64, _I32("move_j"), _I64("j"), _I32("move_jp"), _I64("jp"), _I64("k"),
                              _I64("out_i64"), _F64("out_f64")]),
    "cp_bound_stripe": (_i32, [_vp, _i64, _MODEL, _pi64, _pi64, _pf64, _pf64]),
    "cp_bound_stripe_pi": (_i32, [_vp, _i64, _ROWPART, _MODEL, _pi64, _pi64, _pf64, _pf64]),
    "cp_objective": (_i32, [_vp, _i64, _I64("spl"), _MODEL, _ROWPART, _i32, _pi64, _pf64]),
    "cp_partition_dynamic": (_i32, [_vp, _i64, _i32, _i32, _MODEL, _ROWPART, _MODEL, _i64, _f64, _I64("spl_out")]),
    "cp_pack_dynamic": _PACK,
    "cp_pack_dynamic_tables": (_i32, [_vp, _MODEL, _ROWPART, _MODEL, _i64, _f64, _I64("spl_tab"), _I64("cst_i64"), _F64("cst_f64")]),
    "cp_partition_bisect_cost": (_i32, [_vp, _i64, _MODEL, _f64, _i32, _I64("spl_out")]),
    "cp_partition_bisect_cost_batch": (_i32, [_vp, _i64, _I64("K"), _MODEL, _F64("eps"), _I32("flip"), _i64, _I64("spl_out")]),
    "cp_partition_bisect_cost_pi": (_i32, [_vp, _i64, _MODEL, _ROWPART, _f64, _i32, _I64("spl_out")]),
    "cp_partition_bisect_index_pi": (_i32, [_vp, _i64, _MODEL, _ROWPART, _i32, _I64("spl_out")]),
    "cp_pack_concave": _PACK,
    "cp_partition_concave": _SPLIT,
    "cp_partition_bisect_index": (_i32, [_vp, _i64, _MODEL, _i32, _I64("spl_out")]),
    "cp_partition_lazy_bisect_cost": (_i32, [_vp, _i64, _MODEL, _f64, _I64("spl_out")]),
    "cp_partition_lazy_bisect_cost_probes": (_i32, [_vp, _i64, _MODEL, _f64, _I64("spl_out"), _pi64]),
    "cp_partition_lazy_bisect_cost_pi": (_i32, [_vp, _i64, _MODEL, _ROWPART, _f64, _I64("spl_out"), _I64("nprobes_out")]),
    "cp_partition_lazy_flip_bisect_cost": (_i32, [_vp, _i64, _MODEL, _ROWPART, _f64, _I64("spl_out"), _I64("nprobes_out")]),
    "cp_pack_convex": _PACK,
    "cp_pack_convex_batch": (_i32, [_vp, _i64, _MODEL, _I64("wmax"), _i64, _I64("spl_out"), _I64("K_out")]),
    "cp_partition_convex": _SPLIT,
    "cp_pack_strict": (_i32, [_vp, _i64, _I64("spl_out"), _I64("K_out")]),
    "cp_pack_overlap": (_i32, [_vp, _f64, _i64, _I64("spl_out"), _I64("K_out"), _I64("n_nets_out")]),
    "cp_partition_magnetic": (_i32, [_vp, _i64, _ROWPART, _i64, _I64("draws"), _I64("asg_out")]),
    "cp_partition_greedy_bottleneck": (_i32, [_vp, _i64, _MODEL, _ROWPART, _i64, _I64("order"), _I64("asg_out"), _I64("order_out"),
                                              _I64("cst_i64"), _F64("cst_f64")]),
    "cp_partition_equi": (_i32, [_i64, _i64, _I64("spl_out")]),
    "cp_pack_equi": (_i32, [_i64, _i64, _I64("spl_out"), _I64("K_out")]),
    "cp_dynamic_tables": (_i32, [_vp, _i64, _i32, _MODEL, _ROWPART, _I64("ptr_out"), _I64("cst_i64"), _F64("cst_f64")]),
    "cp_dynamic_tables_constrained": (_i32, [_vp, _i64, _MODEL, _i64, _I64("win_lo"), _I64("win_hi"), _I64("ptr_out"),
                                             _I64("cst_i64"), _F64("cst_f64")]),
    "cp_dynamic_tables_constrained_combine": (_i32, [_vp, _i64, _i32, _MODEL, _MODEL, _i64, _f64, _I64("win_lo"), _I64("win_hi"),
                                                     _I64("ptr_out"), _I64("cst_i64"), _F64("cst_f64")]),
    "cp_dp_begin": (_i32, [_vp, _i64, _i32, _i32, _MODEL, _i64, _i64, _pvp]),
    "cp_dp_layer": (_i32, [_vp, _i64, _vp, _vp]),
    "cp_dp_ptr_at": (_i32, [_vp, _i64, _i64, _pi64]),
    "cp_dp_ptr_row": (_i32, [_vp, _i64, _I64("out")]),
    "cp_dp_set_window": (_i32, [_vp, _i64]),
    "cp_dp_set_rows": (_i32, [_vp, _i64, _i64]),
    "cp_dp_block_tables": (_i32, [_vp, _pi32, _I64("opt_out"), _I64("nets_out"), _I64("selfnets_out")]),
    "cp_dp_destroy": (_i32, [_vp]),
    "cp_set_stream": (_i32, [_vp, _vp]),
    "cp_reset_stream": (_i32, [_vp]),
    "cp_get_stat": (_i32, [_str, _pi64]),
    "cp_test_round_scans": (_i32, [_I32("a"), _i64, _i64, _I32("b"), _i64, _i64, _i32, _i64, _i64, _i32, _i32,
                                   _I64("offs_out"), _I64("toffs_out"), _I64("res")]),
    "cp_test_list_alloc": (_i32, [_I32("a"), _i64, _I32("b"), _i64, _i32, _i64, _i64, _i64, _i32, _i32, _i64, _i64, _i64,
                                  _I64("offs_out"), _I32("slot_a"), _I64("toffs_out"), _I32("slot_b"), _I32("ioffs_out"), _I64("res")]),
    "cp_test_fix_merge": (_i32, [_MODEL, _i64, _I64("toffs"), _I64("part_v"), _I32("part_p"), _I32("part_nn"), _I32("part_nl"), _I32("tile_s"),
                                 _I32("tile_s2"), _I32("anchor"), _I32("anchor2"), _I32("row"), _I32("plane"), _i64, _i32, _I32("p_out"),
                                 _I32("nn_out"), _I32("nl_out"), _I64("res")]),
    "cp_test_own_split": (_i32, [_vp, _I32("vpos_out"), _I32("vsa_out"), _I32("vnext_out"), _I64("res")]),
    "cp_test_own_pair": (_i32, [_i64, _i64, _I64("res")]),
    "cp_test_own_pack": (_i32, [_vp, _I32("vpk_out"), _I32("vbase_out"), _I64("res")]),
    "cp_set_option": (_i32, [_str, _i64]),
    "cp_prof_enable": (_i32, [_i32]),
    "cp_prof_reset": (_i32, []),
    "cp_prof_get": (_i32, [_i32, C.POINTER(C.c_char_p), _pi64, _pf64, _pf64]),
}
SYMBOLS = list(SIGNATURES)
# test entries a library of an earlier build may lack when it is loaded through CP_LIB_PATH for an A/B run (tools/ab_libs.sh): the
# call, not the load, fails there
OPTIONAL = {"cp_test_own_pack", "cp_test_list_alloc"}

_lib = None


def _typed(name, fn, restype, argtypes):
    """fn with its prototype set.  ctypes reports an argument its argtype refused as ctypes.ArgumentError; callers get the
    TypeError it stands for."""
    fn.restype, fn.argtypes = restype, argtypes

    def call(*args):
        try:
            return fn(*args)
        except C.ArgumentError as e:
            raise TypeError(f"{name}: {e}") from None
    return call


def _missing(name):
    def call(*args):
        raise RuntimeError(f"{LIB_PATH} has no {name}: it is a library of an earlier build")
    return call


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(make -C chainpartitioners.jl_amd/csrc); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in OPTIONAL and not hasattr(lib, name):
                setattr(lib, name, _missing(name))
                continue
            setattr(lib, name, _typed(name, getattr(lib, name), restype, argtypes))
        _lib = lib
    return _lib


def _cost_zeros(mm, shape):
    return np.zeros(shape, dtype=np.int64 if mm.struct.dtype == M.CP_I64 else np.float64)


def _by_type(a):
    """the `int64_t *x_i64, double *x_f64` pair of an entry that writes values of the model's element type: a and NULL"""
    return (None, a) if a.dtype == np.float64 else (a, None)


_COUNT_KIND = {"dom": 0, "net": 1, "selfnet": 2, "dianet": 3, "selfpin": 4}


class HipBackend:
    """backend interface of api.py over libchainpart.so (one HIP device per process)."""
    name = "hip"

    def __init__(self, device=0):
        self.lib = load_library()
        if self.lib.cp_device_count() <= 0:
            raise RuntimeError("libchainpart: no HIP device visible (the product path has no CPU fallback)")
        self.device = int(device)
        self._handles = {}

    def last_error(self):
        return (self.lib.cp_last_error() or b"").decode()

    def _ok(self, rc, what, exc=RuntimeError):
        if rc != 0:
            raise exc(f"{what} -> {rc}: {self.last_error()}")

    # ---- CSR residency: one device handle per host matrix object, dropped with it
    def _register(self, obj, h):
        lib, handles, key = self.lib, self._handles, id(obj)

        def _drop(_ref):
            handles.pop(key, None)
            lib.cp_csr_destroy(h)
        handles[key] = (weakref.ref(obj, _drop), h)
        return h

    def csr(self, A):
        ent = self._handles.get(id(A))
        if ent is not None and ent[0]() is A:
            return ent[1]
        h = C.c_void_p()
        rc = self.lib.cp_csr_create(A.m, A.n, A.nnz, A.colptr, A.rowval, self.device, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"cp_csr_create failed ({rc}): {self.last_error()}")
        return self._register(A, h)

    def _h(self, A):
        return A if isinstance(A, C.c_void_p) else self.csr(A)

    def csr_from_device(self, m, n, N, colptr_dev_ptr, rowval_dev_ptr):
        """Handle over colptr/rowval already resident in HBM (1-based int64 device arrays)."""
        h = C.c_void_p()
        rc = self.lib.cp_csr_create_device(m, n, N, colptr_dev_ptr, rowval_dev_ptr, self.device, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"cp_csr_create_device failed ({rc}): {self.last_error()}")
        return h

    def csr_destroy(self, h):
        self.lib.cp_csr_destroy(h)

    def _adopt(self, t):
        """the host mirror of a device handle the library made; the handle stays registered with it"""
        from .types import SparseMatrixCSC
        dims = np.zeros(3, dtype=np.int64)
        self.lib.cp_csr_download(t, dims, None, None)
        m, n, N = (int(x) for x in dims)
        colptr = np.zeros(n + 1, dtype=np.int64); rowval = np.zeros(max(N, 1), dtype=np.int64)
        rc = self.lib.cp_csr_download(t, dims, colptr, rowval)
        if rc != 0:
            self.lib.cp_csr_destroy(t)
            raise RuntimeError(f"cp_csr_download failed ({rc}): {self.last_error()}")
        T = SparseMatrixCSC(m, n, colptr, rowval[:N])
        self._register(T, t)
        return T

    def adjoint(self, A):
        """adjointpattern(A) on the device; the result's device handle stays registered, so a following
        partition_stripe(adj_A, ...) needs no upload."""
        t = C.c_void_p()
        rc = self.lib.cp_adjoint(self._h(A), C.byref(t))
        if rc != 0:
            raise RuntimeError(f"cp_adjoint failed ({rc}): {self.last_error()}")
        return self._adopt(t)

    RCM_STATS = ("path", "trees", "levels", "wide_levels", "walker_launches", "readbacks")

    def rcm(self, A, adj_A, mode, reverse):
        """(rc, rowprm, colprm, stats) of cp_rcm: mode 0 check symmetry / 1 assume it / 2 bipartite; stats["path"]: 1 the symmetric
        walk (both vectors are the same), 2 the bipartite one"""
        rowprm, colprm = np.zeros(A.m, dtype=np.int64), np.zeros(A.n, dtype=np.int64)
        stats = np.zeros(6, dtype=np.int64)
        rc = self.lib.cp_rcm(self._h(A), None if adj_A is None else self._h(adj_A), mode, 1 if reverse else 0, rowprm, colprm, stats)
        return rc, rowprm, colprm, dict(zip(self.RCM_STATS, (int(v) for v in stats)))

    def csr_permute(self, A, rowprm, colprm):
        """A[rowprm, colprm] on the device (None: the identity) -> (rc, matrix that keeps its device handle | None)"""
        t = C.c_void_p()
        as64 = lambda p: None if p is None else np.ascontiguousarray(p, dtype=np.int64)
        rowprm, colprm = as64(rowprm), as64(colprm)
        if (rowprm is not None and rowprm.shape != (A.m,)) or (colprm is not None and colprm.shape != (A.n,)):
            raise ValueError("permute: a permutation must have one entry per row / column")
        rc = self.lib.cp_csr_permute(self._h(A), rowprm, colprm, C.byref(t))
        return rc, (self._adopt(t) if rc == 0 else None)

    def csr_quotient(self, A, rp):
        """the quotient pattern of A under the marshalled row split rp, on the device -> (rc, matrix that keeps its device handle | None)"""
        t = C.c_void_p()
        rc = self.lib.cp_csr_quotient(self._h(A), rp, C.byref(t))
        return rc, (self._adopt(t) if rc == 0 else None)

    def reset_cache(self, A_or_handle):
        return self.lib.cp_csr_reset_cache(self._h(A_or_handle))

    def set_stream(self, A_or_handle, stream_ptr):
        return self.lib.cp_set_stream(self._h(A_or_handle), stream_ptr)

    def reset_stream(self, A_or_handle):
        return self.lib.cp_reset_stream(self._h(A_or_handle))

    def get_stat(self, name):
        out = C.c_int64()
        rc = self.lib.cp_get_stat(name.encode(), C.byref(out))
        if rc != 0:
            raise KeyError(name)
        return out.value

    def test_round_scans(self, a, na_max, b, nb_max, two=True, cap_t=2**62, cap_nt=2**62, err_in=0, reps=1):
        """the two task scans + verdict of a DP round in one launch (test entry): (offs, toffs, {T, NT, nlong, nown, ntile, err})"""
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.ascontiguousarray(b, dtype=np.int32)
        offs = np.zeros(len(a) + 1, dtype=np.int64)
        toffs = np.zeros(len(b) + 1, dtype=np.int64)
        res = np.zeros(6, dtype=np.int64)
        rc = self.lib.cp_test_round_scans(a, len(a), na_max, b, len(b), nb_max, 1 if two else 0, cap_t, cap_nt, err_in, reps,
                                          offs, toffs, res)
        self._ok(rc, "cp_test_round_scans")
        return offs, toffs, dict(zip(("T", "NT", "nlong", "nown", "ntile", "err"), (int(v) for v in res)))

    def test_fix_merge(self, mm, toffs, part_v, part_p, part_nn, part_nl, tile_s, tile_s2, anchor, anchor2, row, plane, n, reps=1):
        """the own-tile merge of a DP round in one launch (test entry): (p, nn, nl or None, {items, trips, edges, tickets_left}); part_v
        holds the costs in the model's element type, part_nl / tile_s2 / anchor2 are None unless the model is HyperedgeCut"""
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        toffs = np.ascontiguousarray(toffs, dtype=np.int64)
        ntask = len(toffs) - 1
        part_v = np.ascontiguousarray(part_v, dtype=np.int64 if mm.struct.dtype == M.CP_I64 else np.float64).view(np.int64)
        p, nn, res = np.zeros(ntask, np.int32), np.zeros(ntask, np.int32), np.zeros(4, np.int64)
        nl = None if part_nl is None else np.zeros(ntask, np.int32)
        rc = self.lib.cp_test_fix_merge(mm, ntask, toffs, part_v, i32(part_p), i32(part_nn), i32(part_nl), i32(tile_s), i32(tile_s2), i32(anchor),
                                        i32(anchor2), i32(row), i32(plane), n, reps, p, nn, nl, res)
        self._ok(rc, "cp_test_fix_merge")
        return p, nn, nl, dict(zip(("items", "trips", "edges", "tickets_left"), (int(v) for v in res)))

    def test_own_split(self, A):
        """the link entries split by bit plane (test entry): (nb, vpos[nb, n + 1], vsa[nb, n + 1], vnext[total])"""
        nb = max(0, int(A.n).bit_length() - 8)
        vpos = np.zeros((max(nb, 1), A.n + 1), np.int32); vsa = np.zeros_like(vpos)
        vnext = np.zeros(max(A.nnz, 1), np.int32); res = np.zeros(2, np.int64)
        rc = self.lib.cp_test_own_split(self._h(A), vpos.reshape(-1), vsa.reshape(-1), vnext, res)
        self._ok(rc, "cp_test_own_split")
        assert int(res[0]) == nb
        return nb, vpos[:nb], vsa[:nb], vnext[:int(res[1])]

    def test_own_pair(self, nt, wave):
        """the two slots of the run order a wave of the paired own-tile stream takes (test entry, host only): (has work, s0, s1)"""
        res = np.zeros(3, np.int64)
        self._ok(self.lib.cp_test_own_pair(nt, wave, res), "cp_test_own_pair")
        return bool(res[0]), int(res[1]), int(res[2])

    def test_own_pack(self, A):
        """the packed words and block bases of the split link entries (test entry): (nb, vpk[nb, n + 1] uint32, vbase[nb, blocks + 1, 2],
        {"blocks", "packed", "max_start", "max_prefix"})"""
        nb = max(0, int(A.n).bit_length() - 8)
        nblk = (A.n + 1 + 255) // 256
        vpk = np.zeros((max(nb, 1), A.n + 1), np.int32); vbase = np.zeros((max(nb, 1), nblk + 1, 2), np.int32)
        res = np.zeros(5, np.int64)
        self._ok(self.lib.cp_test_own_pack(self._h(A), vpk.reshape(-1), vbase.reshape(-1), res), "cp_test_own_pack")
        assert int(res[0]) == nb and int(res[1]) == nblk
        return nb, vpk[:nb].view(np.uint32), vbase[:nb], dict(zip(("blocks", "packed", "max_start", "max_prefix"), (int(v) for v in res[1:])))

    def set_option(self, name, value):
        return self.lib.cp_set_option(name.encode(), value)

    # ---- partitioners
    def partition_dynamic(self, A, K, combine, order, mm, rp, wm, wi, wf, spl):
        return self.lib.cp_partition_dynamic(self._h(A), K, combine, order, mm, rp, wm, wi, wf, spl)

    def pack_dynamic(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return self.lib.cp_pack_dynamic(self._h(A), mm, rp, wm, wi, wf, spl, Kout)

    def pack_dynamic_tables(self, A, mm, rp, wm, wi, wf):
        """(rc, cst[n+1], spl[n+1]) of DynamicTotalChunker: the tables DynamicChunker.jl:20-56 builds before unravel_chunks!
        (index j' - 1; spl[0] = 0)"""
        spl = np.zeros(A.n + 1, dtype=np.int64)
        cst = _cost_zeros(mm, A.n + 1)
        rc = self.lib.cp_pack_dynamic_tables(self._h(A), mm, rp, wm, wi, wf, spl, *_by_type(cst))
        return rc, cst, spl

    def partition_bisect_cost(self, A, K, mm, eps, flip, spl, rp=None):
        return self.lib.cp_partition_bisect_cost_pi(self._h(A), K, mm, rp, eps, flip, spl)

    def partition_bisect_cost_batch(self, A, Ks, mms, epss, flips):
        """B requests on one pattern in one launch -> (rc, [split vector of request b])"""
        B = len(Ks)
        arr = (M.cp_model_t * B)(*[m.struct for m in mms])          # (struct copies; the buffers they point into live in `mms`)
        Kv = np.ascontiguousarray(Ks, dtype=np.int64)
        ev = np.ascontiguousarray(epss, dtype=np.float64)
        fv = np.ascontiguousarray(flips, dtype=np.int32)
        ld = int(Kv.max()) + 1
        out = np.zeros((B, ld), dtype=np.int64)
        rc = self.lib.cp_partition_bisect_cost_batch(self._h(A), B, Kv, arr, ev, fv, ld, out)
        return rc, [out[b, :int(Kv[b]) + 1].copy() for b in range(B)]

    def partition_bisect_index(self, A, K, mm, flip, spl, rp=None):
        return self.lib.cp_partition_bisect_index_pi(self._h(A), K, mm, rp, flip, spl)

    def partition_lazy_bisect_cost(self, A, K, mm, eps, spl):
        """the row partition of a primary model rides on the marshalled model (mm.rowpart, set by api._dispatch)"""
        if getattr(mm, "rowpart", None) is not None:
            return self.lib.cp_partition_lazy_bisect_cost_pi(self._h(A), K, mm, mm.rowpart, eps, spl, None)
        return self.lib.cp_partition_lazy_bisect_cost(self._h(A), K, mm, eps, spl)

    def partition_lazy_bisect_cost_probes(self, A, K, mm, eps, rp=None):
        """(rc, spl, number of probes the bisection ran); rp: the row partition a primary model needs"""
        spl = np.zeros(K + 1, dtype=np.int64)
        if rp is not None:
            npr = np.zeros(1, dtype=np.int64)
            rc = self.lib.cp_partition_lazy_bisect_cost_pi(self._h(A), K, mm, rp, eps, spl, npr)
            return rc, spl, int(npr[0])
        npr = C.c_int64()
        rc = self.lib.cp_partition_lazy_bisect_cost_probes(self._h(A), K, mm, eps, spl, C.byref(npr))
        return rc, spl, npr.value

    def partition_lazy_flip_bisect_cost(self, A, K, mm, eps, spl, rp=None):
        return self.lib.cp_partition_lazy_flip_bisect_cost(self._h(A), K, mm, rp, eps, spl, None)

    def partition_lazy_flip_bisect_cost_probes(self, A, K, mm, eps, rp=None):
        """(rc, spl, number of probes the bisection ran); rp: the row partition a primary or secondary model needs"""
        spl, npr = np.zeros(K + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        rc = self.lib.cp_partition_lazy_flip_bisect_cost(self._h(A), K, mm, rp, eps, spl, npr)
        return rc, spl, int(npr[0])

    def pack_convex(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return self.lib.cp_pack_convex(self._h(A), mm, rp, wm, wi, wf, spl, Kout)

    def pack_convex_batch(self, A, mms, wmaxs, n):
        """B requests (model, w_max) on one pattern in one launch -> (rc, [chunk boundaries of request b])"""
        B = len(mms)
        arr = (M.cp_model_t * B)(*[m.struct for m in mms])
        wv = np.ascontiguousarray(wmaxs, dtype=np.int64)
        ld = int(n) + 1
        out = np.zeros((B, ld), dtype=np.int64)
        Kout = np.zeros(B, dtype=np.int64)
        rc = self.lib.cp_pack_convex_batch(self._h(A), B, arr, wv, ld, out, Kout)
        return rc, [out[b, :int(Kout[b]) + 1].copy() for b in range(B)]

    def partition_convex(self, A, K, mm, rp, wm, wi, wf, spl):
        return self.lib.cp_partition_convex(self._h(A), K, mm, rp, wm, wi, wf, spl)

    def pack_concave(self, A, mm, rp, wm, wi, wf, spl, Kout):
        return self.lib.cp_pack_concave(self._h(A), mm, rp, wm, wi, wf, spl, Kout)

    def partition_concave(self, A, K, mm, rp, wm, wi, wf, spl):
        return self.lib.cp_partition_concave(self._h(A), K, mm, rp, wm, wi, wf, spl)

    def pack_strict(self, A, w_max, spl, Kout):
        return self.lib.cp_pack_strict(self._h(A), int(w_max), spl, Kout)

    def pack_overlap(self, A, rho, w_max, spl, Kout, n_nets=None):
        """n_nets: None or an int64 array of n slots; the first K receive the distinct-row count of every part"""
        return self.lib.cp_pack_overlap(self._h(A), float(rho), int(w_max), spl, Kout, n_nets)

    def partition_magnetic(self, A, K, rp, seed, draws, asg):
        """MagneticPartitioner: draws None (the device draws draw(seed, 1, j)) or n int64 values; asg: n slots"""
        return self.lib.cp_partition_magnetic(self._h(A), K, rp, seed, draws, asg)

    def partition_greedy_bottleneck(self, A, K, mm, rp, seed, order, asg):
        """GreedyBottleneckPartitioner: order None (the device sorts the keys draw(seed, 2, j)) or a permutation of 1 .. n;
        -> (rc, the order that was walked, the K final part costs in the model's element type)"""
        order_out, cst = np.zeros(A.n, dtype=np.int64), _cost_zeros(mm, K)
        rc = self.lib.cp_partition_greedy_bottleneck(self._h(A), K, mm, rp, seed, order, asg, order_out, *_by_type(cst))
        return rc, order_out, cst

    # ---- oracles / scoring
    def oracle_eval(self, A, mm, rp, hint, j, jp, k, out):
        return self.lib.cp_oracle_eval(self._h(A), mm, rp, hint, j.size, j, jp, k, *_by_type(out))

    def oracle_step(self, A, mm, rp, mj, j, mjp, jp, k, out):
        return self.lib.cp_oracle_step(self._h(A), mm, rp, j.size, mj, j, mjp, jp, k, *_by_type(out))

    def _bounds(self, fn, mm, *args):
        li, hi, lf, hf = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        rc = fn(*args, C.byref(li), C.byref(hi), C.byref(lf), C.byref(hf))
        if mm.struct.dtype == M.CP_I64:
            return rc, li.value, hi.value
        return rc, lf.value, hf.value

    def bound_stripe(self, A, K, mm):
        return self._bounds(self.lib.cp_bound_stripe, mm, self._h(A), K, mm)

    def bound_stripe_pi(self, A, K, rp, mm):
        return self._bounds(self.lib.cp_bound_stripe_pi, mm, self._h(A), K, rp, mm)

    def objective(self, A, K, spl, mm, rp, g):
        oi, of = C.c_int64(), C.c_double()
        rc = self.lib.cp_objective(self._h(A), K, spl, mm, rp, g, C.byref(oi), C.byref(of))
        return rc, (oi.value if mm.struct.dtype == M.CP_I64 else of.value)

    def dynamic_tables(self, A, K, combine, mm, rp):
        ptr = np.zeros((K, A.n + 1), dtype=np.int64)
        cst = _cost_zeros(mm, (K, A.n + 1))
        rc = self.lib.cp_dynamic_tables(self._h(A), K, combine, mm, rp, ptr, *_by_type(cst))
        return rc, ptr.T, cst.T

    def dynamic_tables_constrained(self, A, K, mm, wmax, combine=0, wm=None):
        """(rc, j'_lo[K], j'_hi[K], ptr[j', k], cst[j', k]) of Dynamic{Total,Bottleneck}Splitter(ConstrainedCost(f, w, wmax))
        (combine 0 = total, 1 = bottleneck; wm: the marshalled weight, None = VertexCount())"""
        ptr = np.zeros((K, A.n + 1), dtype=np.int64)
        cst = _cost_zeros(mm, (K, A.n + 1))
        lo = np.zeros(K, dtype=np.int64); hi = np.zeros(K, dtype=np.int64)
        rc = self.lib.cp_dynamic_tables_constrained_combine(self._h(A), K, combine, mm, wm, int(wmax), float(wmax), lo, hi, ptr,
                                                            *_by_type(cst))
        return rc, lo, hi, ptr.T, cst.T

    # ---- counting structures
    def count_build(self, kind, A, hint):
        h = C.c_void_p()
        rc = self.lib.cp_count_build(self._h(A), _COUNT_KIND[kind], hint, C.byref(h))
        if rc == M.CP_EINVAL and kind in ("dianet", "selfpin"):      # the reference asserts m == n
            raise AssertionError(f"cp_count_build({kind}): violated precondition ({self.last_error()})")
        self._ok(rc, f"cp_count_build({kind})", NotImplementedError)
        return h

    def count_query(self, kind, h, a, b, out):
        return self.lib.cp_count_query(h, a.size, a, b, out)

    def count_free(self, kind, h):
        self.lib.cp_count_destroy(h)

    # ---- rowenvelope (EnvelopeMatrices.jl)
    def envelope_build(self, A):
        h = C.c_void_p()
        rc = self.lib.cp_envelope_build(self._h(A), C.byref(h))
        if rc == M.CP_EINVAL:
            raise AssertionError(f"cp_envelope_build: violated precondition ({self.last_error()})")
        self._ok(rc, "cp_envelope_build")
        return h

    def envelope_dims(self, h):
        dims = np.zeros(3, dtype=np.int64)
        self._ok(self.lib.cp_envelope_tree(h, dims, None), "cp_envelope_tree")
        return tuple(int(v) for v in dims)

    def envelope_tree(self, h):
        H = self.envelope_dims(h)[0]
        dims, tree = np.zeros(3, dtype=np.int64), np.zeros(((2 << H) - 1, 2), dtype=np.int64)
        self._ok(self.lib.cp_envelope_tree(h, dims, tree.reshape(-1)), "cp_envelope_tree")
        return tree

    def envelope_query(self, h, j, jp, lo, hi):
        return self.lib.cp_envelope_query(h, j.size, j, jp, lo, hi)

    def envelope_free(self, h):
        self.lib.cp_envelope_destroy(h)

    # ---- weighted dominance (a13)
    def domsum_build(self, A, val):
        val = np.ascontiguousarray(val)
        dt = M.CP_F64 if val.dtype == np.float64 else M.CP_I64
        h = C.c_void_p()
        self._ok(self.lib.cp_domsum_build(self._h(A), dt, val, C.byref(h)), "cp_domsum_build")
        return h, dt

    def rook_build(self, N, idx, val=None):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dt = M.CP_I64
        if val is not None:
            val = np.ascontiguousarray(val)
            dt = M.CP_F64 if val.dtype == np.float64 else M.CP_I64
        h = C.c_void_p()
        self._ok(self.lib.cp_rook_build(N, idx, dt, val, self.device, C.byref(h)), "cp_rook_build")
        return h, dt

    def wsum_query(self, h, dt, i, j, unsigned=False):
        i = np.ascontiguousarray(i, dtype=np.int64); j = np.ascontiguousarray(j, dtype=np.int64)
        cnt = np.zeros(i.shape, dtype=np.int64)
        sm = np.zeros(i.shape, dtype=np.float64 if dt == M.CP_F64 else np.int64)
        self._ok(self.lib.cp_wsum_query(h, i.size, i, j, cnt, *_by_type(sm)), "cp_wsum_query")
        return cnt, (sm.view(np.uint64) if unsigned and dt == M.CP_I64 else sm)      # the same words, read as UInt

    def wsum_free(self, h):
        self.lib.cp_wsum_destroy(h)

    def link_array(self, A):
        out = np.zeros(max(A.nnz, 1), dtype=np.int64)
        rc = self.lib.cp_link_array(self._h(A), out)
        if rc != 0:
            raise RuntimeError(self.last_error())
        return out[:A.nnz]

    def partwise(self, A, K, asg):
        asg = np.ascontiguousarray(asg, dtype=np.int64)
        npr = C.c_int64()
        pios = np.zeros(K + 1, dtype=np.int64)
        prm = np.zeros(max(A.nnz, 1), dtype=np.int64)
        pos = np.zeros(A.nnz + 1, dtype=np.int64)
        idx = np.zeros(max(A.nnz, 1), dtype=np.int64)
        rc = self.lib.cp_partwise(self._h(A), K, asg, C.byref(npr), pios, prm, pos, idx)
        self._ok(rc, "cp_partwise", NotImplementedError)
        n = npr.value
        return n, pios, prm[:n].copy(), pos[:n + 1].copy(), idx[:A.nnz].copy()

    # ---- row-tiled DP (multi-GPU): see distributed.py
    def dp_begin(self, A, K, combine, order, mm, row_lo, row_hi):
        h = C.c_void_p()
        self._ok(self.lib.cp_dp_begin(self._h(A), K, combine, order, mm, row_lo, row_hi, C.byref(h)), "cp_dp_begin")
        return h

    def dp_layer(self, dp, k, prev_ptr, cur_ptr):
        self._ok(self.lib.cp_dp_layer(dp, k, prev_ptr, cur_ptr), "cp_dp_layer")

    def dp_ptr_at(self, dp, k, jp):
        out = C.c_int64()
        self._ok(self.lib.cp_dp_ptr_at(dp, k, jp, C.byref(out)), "cp_dp_ptr_at")
        return out.value

    def dp_ptr_row(self, dp, k, n):
        out = np.zeros(n + 1, dtype=np.int64)
        self._ok(self.lib.cp_dp_ptr_row(dp, k, out), "cp_dp_ptr_row")
        return out

    def dp_block_tables(self, dp, n, hyper=False):
        """(nplanes, opt[b, r], nets[b, r], selfnets[b, r] | None) of the last layer computed through `dp`."""
        nb = C.c_int32()
        opt = np.zeros((31, n + 1), dtype=np.int64); nn = np.zeros((31, n + 1), dtype=np.int64)
        nl = np.zeros((31, n + 1), dtype=np.int64) if hyper else None
        self._ok(self.lib.cp_dp_block_tables(dp, C.byref(nb), opt, nn, nl), "cp_dp_block_tables")
        # the library lays the planes out with stride n+1
        k = nb.value
        return k, opt.reshape(-1)[:k * (n + 1)].reshape(k, n + 1), nn.reshape(-1)[:k * (n + 1)].reshape(k, n + 1), \
            (nl.reshape(-1)[:k * (n + 1)].reshape(k, n + 1) if hyper else None)

    def dp_set_window(self, dp, wmax):
        rc = self.lib.cp_dp_set_window(dp, wmax)
        if rc != 0:
            raise RuntimeError(f"cp_dp_set_window -> {rc}")

    def dp_set_rows(self, dp, lo, hi):
        rc = self.lib.cp_dp_set_rows(dp, lo, hi)
        if rc != 0:
            raise RuntimeError(f"cp_dp_set_rows({lo}, {hi}) -> {rc}")

    def windowed_layer(self, A, mm, W, wmax, lo=None, hi=None):
        """one DP layer over injected previous costs W (numpy, n+1) with the width window wmax: (cst[r], ptr[r]) 0-based,
        rows [lo, hi) 1-based like cp_dp_begin (default: all)"""
        import torch
        n = A.n
        dev = torch.device("cuda", self.device)
        dp = self.dp_begin(A, 3, 0, 0, mm, lo or 1, hi or n + 2)
        try:
            self.dp_set_window(dp, wmax)
            prev = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
            cur = torch.zeros(n + 1, dtype=prev.dtype, device=dev)
            self.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
            return cur.cpu().numpy(), self.dp_ptr_row(dp, 2, n) - 1
        finally:
            self.dp_destroy(dp)

    def dp_destroy(self, dp):
        self.lib.cp_dp_destroy(dp)

    # ---- measurement
    def prof_enable(self, on=True):
        self.lib.cp_prof_enable(1 if on else 0)

    def prof_reset(self):
        self.lib.cp_prof_reset()

    def prof_get(self):
        out = {}
        name = C.c_char_p()
        n, ms, by = C.c_int64(), C.c_double(), C.c_double()
        args = (C.byref(name), C.byref(n), C.byref(ms), C.byref(by))
        for s in range(self.lib.cp_prof_get(0, *args)):
            self.lib.cp_prof_get(s, *args)
            out[name.value.decode()] = {"launches": n.value, "ms": ms.value, "units": by.value}
        return out
