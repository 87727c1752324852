"""CPU-only checks: the C-ABI library loads and exports every symbol include/chainpart.h declares
(no compute calls without a GPU), the product refuses to run without a device, host-side closed
forms, and the struct layouts the Python marshalling assumes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from util import cp, sprand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "chainpart.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cp_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from chainpartitioners_jl_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(_lib.LIB_PATH)
    decl = declared_symbols()
    assert len(decl) >= 25
    for name in decl:
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == decl       # the binding covers exactly the header (prototype by prototype: below)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from chainpartitioners_jl_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    assert lib.cp_device_count() == 0
    with pytest.raises(RuntimeError):
        _lib.HipBackend()
    A = sprand(4, 6, 0.5, np.random.default_rng(0))
    h = C.c_void_p()
    rc = lib.cp_csr_create(C.c_int64(A.m), C.c_int64(A.n), C.c_int64(A.nnz), A.colptr.ctypes.data_as(C.c_void_p),
                           A.rowval.ctypes.data_as(C.c_void_p), C.c_int32(0), C.byref(h))
    assert rc == 3 and not h.value                # CP_EHIP: refuses loudly, no handle
    lib.cp_last_error.restype = C.c_char_p
    assert b"no HIP device" in lib.cp_last_error()


def test_equi_closed_forms_match_library_and_oracle(orc):
    from chainpartitioners_jl_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    import orc_binding
    olib = orc_binding.lib()
    for n in (0, 1, 5, 17, 100):
        for K in (1, 2, 3, 8, 23):
            a = np.zeros(K + 1, dtype=np.int64); b = np.zeros(K + 1, dtype=np.int64)
            assert lib.cp_partition_equi(C.c_int64(n), C.c_int64(K), a.ctypes.data_as(C.c_void_p)) == 0
            olib.orc_partition_equi(C.c_int64(n), C.c_int64(K), b)
            A = cp.SparseMatrixCSC(1, n, np.ones(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64))
            assert a.tolist() == b.tolist() == cp.partition_stripe(A, K, cp.EquiSplitter()).spl.tolist()
        for w in (1, 2, 5):
            a = np.zeros(n + 2, dtype=np.int64); b = np.zeros(n + 2, dtype=np.int64); Ka = C.c_int64()
            assert lib.cp_pack_equi(C.c_int64(n), C.c_int64(w), a.ctypes.data_as(C.c_void_p), C.byref(Ka)) == 0
            Kb = olib.orc_pack_equi(C.c_int64(n), C.c_int64(w), b)
            assert Ka.value == Kb and a[:Kb + 1].tolist() == b[:Kb + 1].tolist()


def test_struct_layout_matches_header(tmp_path):
    """ctypes mirrors vs the C header itself: sizes and field offsets printed by a program compiled from
    include/chainpart_types.h."""
    import subprocess
    from chainpartitioners_jl_amd import models as M
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "chainpart_types.h"
int main(void) {
    printf("%zu %zu %zu ", sizeof(cp_component_t), sizeof(cp_model_t), sizeof(cp_rowpart_t));
    printf("%zu %zu %zu ", offsetof(cp_component_t, table), offsetof(cp_component_t, len), offsetof(cp_component_t, lo));
    printf("%zu %zu %zu %zu %zu\\n", offsetof(cp_model_t, p_f64), offsetof(cp_model_t, alpha_k), offsetof(cp_model_t, R),
           offsetof(cp_model_t, alpha_row), offsetof(cp_model_t, beta_col));
    return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(M.cp_component_t), C.sizeof(M.cp_model_t), C.sizeof(M.cp_rowpart_t),
            M.cp_component_t.table.offset, M.cp_component_t.len.offset, M.cp_component_t.lo.offset,
            M.cp_model_t.p_f64.offset, M.cp_model_t.alpha_k.offset, M.cp_model_t.R.offset,
            M.cp_model_t.alpha_row.offset, M.cp_model_t.beta_col.offset]
    assert got == want


def test_model_promotion_rules():
    assert cp.AffineConnectivityModel(0, 10, 1, 100).dtype == 0          # all Int -> Int64
    assert cp.AffineConnectivityModel(0.0, 0, 0, 1).dtype == 1           # promote -> Float64
    assert cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[1, 2]).dtype == 0
    assert cp.AffineWorkModel(0, 10, 1)(3, 7) == 37


def test_plain_c_client_builds_against_the_header():
    """examples/c_abi_demo.c uses nothing but include/chainpart.h and the shared library (no Python, no torch types)."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "clean", "c_abi_demo"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(ROOT, "examples", "c_abi_demo"))


# every option of cp_set_option with its default (csrc: the g_opt_* definitions): setting it again leaves the process as it was
OPTIONS = {"force_brute": 0, "brute_max_n": 200000, "dbg": 0, "short_t": 8, "short_e": 64, "rpass_ch": 256, "prof_only": -1, "gap_tau": 6,
           "gap_min": 64, "gap_nr": 2, "pool": 1, "ra_cache": 1, "leaf": 1, "poison": 0, "block_tables": 0, "rpass_small_tau": 4,
           "force_max": 1024, "setup_bs": 1024, "rpass_cap": 200, "fixed_point": 0, "nospec": 0, "own_min": 64, "own_blk": 1, "bn_chunk": 8,
           "bn_wave": 2, "bn_slack": 64, "lws": 1, "lws_leaf": 512, "bn_run": 253}
STATS = ["spec_redo", "poison_hits", "fix_trips", "fix_edges", "bn_sym_layers"]


def test_options_and_stats_by_name():
    from chainpartitioners_jl_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cp_last_error.restype = C.c_char_p
    for name, default in OPTIONS.items():
        assert lib.cp_set_option(name.encode(), C.c_int64(default)) == 0, name
    assert lib.cp_set_option(b"no_such_option", C.c_int64(1)) == 1            # CP_EINVAL
    assert lib.cp_last_error() == b"unknown option"
    assert lib.cp_set_option(None, C.c_int64(1)) == 1
    out = C.c_int64(-1)
    assert lib.cp_set_option(b"stat_reset", C.c_int64(0)) == 0
    for name in STATS:
        out.value = -1
        assert lib.cp_get_stat(name.encode(), C.byref(out)) == 0 and out.value == 0, name
    assert lib.cp_get_stat(b"no_such_stat", C.byref(out)) == 1
    assert lib.cp_get_stat(b"spec_redo", None) == 1


# ---------------------------------------------------------------- the Python side's prototypes are the header's
def prototypes(path, prefix):
    """{name: (return type, [(parameter type, parameter name)])} of a header whose declarations read `type name(args);`"""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    norm = lambda t: re.sub(r"\s*\*\s*", "*", " ".join(t.split()))
    out = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+[\s\*]+)(%s\w+)\s*\(([^)]*)\)\s*;" % prefix, txt, flags=re.M):
        params = [re.match(r"(.*?)(\w+)$", a.strip()).groups() for a in args.split(",") if a.strip() != "void"]
        out[name] = (norm(ret), [(norm(t), n) for t, n in params])
    return out


def expected_argtype(mod, fname, ctype, pname, scalars, structs, out_scalars):
    """the ctypes class, or ("array" | "words" | "struct", ...) for the binding's own argument classes"""
    if ctype in scalars:
        return scalars[ctype]
    if ctype in structs:
        return structs[ctype]
    if ctype in ("void*", "const void*") or pname.endswith("_device"):
        return ("words", pname) if pname == "val" else C.c_void_p
    base = {"int64_t*": C.c_int64, "int32_t*": C.c_int32, "double*": C.c_double}[ctype.replace("const ", "")]
    if (fname, pname) in out_scalars:
        assert not ctype.startswith("const")
        return C.POINTER(base)
    return ("array", np.dtype(base), pname)


def same_argtype(mod, want, got):
    if isinstance(want, tuple) and want[0] == "array":
        return type(got) is mod._Array and got.dtype == want[1] and got.name == want[2]
    if isinstance(want, tuple) and want[0] == "words":
        return type(got) is mod._Words and got.name == want[1]
    if isinstance(want, tuple) and want[0] == "struct":
        return type(got) is mod._Struct and got.name == want[1]
    return got is want


def check_table(mod, protos, scalars, structs, out_scalars, returns):
    for name, (restype, argtypes) in mod.SIGNATURES.items():
        ret, params = protos[name]
        assert restype is returns[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for pos, ((ctype, pname), got) in enumerate(zip(params, argtypes)):
            want = expected_argtype(mod, name, ctype, pname, scalars, structs, out_scalars)
            assert same_argtype(mod, want, got), (name, pos, ctype, pname, want, got)
    assert not set(out_scalars) - {(f, p) for f, (_, ps) in protos.items() for _, p in ps}     # (the list below names real parameters)


def test_signature_table_is_the_header():
    """name by name, arity, every position and the return type; which `T *` is one value written back rather than an array is
    what the header's comments say, listed here"""
    from chainpartitioners_jl_amd import _lib, models as M
    protos = prototypes(os.path.join(ROOT, "include", "chainpart.h"), "cp_")
    assert sorted(protos) == sorted(_lib.SIGNATURES) == declared_symbols()
    handle = dict.fromkeys(("cp_csr_t", "cp_count_t", "cp_wsum_t", "cp_dp_t"), C.c_void_p)
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "const char*": C.c_char_p,
               "const char**": C.POINTER(C.c_char_p), **handle, **{h + "*": C.POINTER(C.c_void_p) for h in handle}}
    structs = {"const cp_model_t*": C.POINTER(M.cp_model_t), "const cp_rowpart_t*": C.POINTER(M.cp_rowpart_t)}
    out_scalars = {("cp_partwise", "nprime_out"), ("cp_objective", "out_i64"), ("cp_objective", "out_f64"),
                   ("cp_partition_lazy_bisect_cost_probes", "nprobes_out"), ("cp_dp_ptr_at", "out"), ("cp_dp_block_tables", "nplanes_out"),
                   ("cp_get_stat", "out"), ("cp_prof_get", "launches"), ("cp_prof_get", "total_ms"), ("cp_prof_get", "alg_bytes")}
    out_scalars |= {(f, p) for f in ("cp_bound_stripe", "cp_bound_stripe_pi") for p in ("lo_i64", "hi_i64", "lo_f64", "hi_f64")}
    check_table(_lib, protos, scalars, structs, out_scalars, {"int32_t": C.c_int32, "const char*": C.c_char_p})
    lib = _lib.load_library()                                  # ... and load_library() applied it
    assert _lib.SYMBOLS == list(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) and callable(getattr(lib, name)) for name in _lib.SYMBOLS)


def test_oracle_signature_table_is_its_header():
    import orc_binding
    protos = prototypes(os.path.join(ROOT, "oracle", "orc.h"), "orc_")
    assert set(orc_binding.SIGNATURES) <= set(protos) and len(orc_binding.SIGNATURES) >= 25
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "orc_dom*": C.c_void_p, "orc_net*": C.c_void_p}
    structs = ("const cp_model_t*", "const cp_rowpart_t*")     # the oracle's _Struct, which carries the parameter's name
    out_scalars = {(f, p) for f in ("orc_bound_stripe", "orc_bound_stripe_pi") for p in ("lo_i64", "hi_i64", "lo_f64", "hi_f64")}
    out_scalars |= {("orc_objective", "out_i64"), ("orc_objective", "out_f64")}
    returns = {"int32_t": C.c_int32, "int64_t": C.c_int64, "void": None, "orc_dom*": C.c_void_p, "orc_net*": C.c_void_p}
    for name, (restype, argtypes) in orc_binding.SIGNATURES.items():
        ret, params = protos[name]
        assert restype is returns[ret], (name, ret, restype)
        assert len(argtypes) == len(params), name
        for pos, ((ctype, pname), got) in enumerate(zip(params, argtypes)):
            want = ("struct", pname) if ctype in structs else expected_argtype(orc_binding, name, ctype, pname, scalars, {}, out_scalars)
            assert same_argtype(orc_binding, want, got), (name, pos, ctype, pname, want, got)
    L = orc_binding.lib()
    assert all(getattr(L, n).restype is r and list(getattr(L, n).argtypes) == a for n, (r, a) in orc_binding.SIGNATURES.items())


# ---------------------------------------------------------------- the boundary refuses what used to be passed on
def test_boundary_checks_arrays_and_keeps_wide_ints():
    from chainpartitioners_jl_amd import _lib
    lib = _lib.load_library()
    with pytest.raises(TypeError, match="spl_out.*int64"):
        lib.cp_partition_equi(5, 2, np.zeros(3, dtype=np.float64))                 # double where int64_t * is declared
    with pytest.raises(TypeError, match="spl_out.*contiguous"):
        lib.cp_partition_equi(5, 2, np.zeros(6, dtype=np.int64)[::2])              # a strided view
    with pytest.raises(TypeError, match="spl_out"):
        lib.cp_partition_equi(5, 2, [0, 0, 0])                                      # not an array at all
    with pytest.raises(TypeError):
        lib.cp_partition_equi(5.0, 2, np.zeros(3, dtype=np.int64))                 # a float where int64_t is declared
    assert lib.cp_partition_equi(5, 2, None) == 1                                  # None is NULL: the library's own CP_EINVAL
    assert lib.cp_set_option(None, 1) == 1 and lib.cp_set_option(b"no_such_option", 1) == 1
    assert lib.cp_last_error() == b"unknown option"                                # (a declared return type: bytes, not an address)
    out = np.zeros(2, dtype=np.int64)
    assert lib.cp_partition_equi(2**40, 1, out) == 0 and out.tolist() == [1, 2**40 + 1]   # a plain int >= 2^31 arrives whole
    assert lib.cp_partition_equi(np.int64(2**40), np.int32(1), out) == 0 and out.tolist() == [1, 2**40 + 1]
    assert lib.cp_set_option(b"brute_max_n", 2**40) == 0 and lib.cp_set_option(b"brute_max_n", OPTIONS["brute_max_n"]) == 0


# ---------------------------------------------------------------- marshalling: unchanged, and it writes nothing to the model
def test_marshalling_reproduces_the_recorded_bytes():
    """tests/golden/marshal.json was recorded (tools/make_golden_marshal.py) before marshal() took its ranges as arguments"""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_marshal as G
    gold = json.load(open(G.PATH))
    cases = G.cases()
    assert len(cases) == len(gold) >= 25
    for name, fn in cases:
        assert json.loads(json.dumps(fn())) == gold[name], name


def test_marshalling_leaves_the_model_alone():
    from chainpartitioners_jl_amd import api, models as M
    sq = lambda w: w * w
    A = cp.SparseMatrixCSC(7, 9, np.ones(10, dtype=np.int64), np.zeros(0, dtype=np.int64))
    for mdl in (M.ColumnBlockComponentCostModel(sq, sq), M.BlockComponentCostModel(sq, sq, (sq,), (sq,)),
                M.BlockComponentCostModel(sq, sq, (sq,), (sq,), w_table=3, u_table=2), M.AffineConnectivityModel(0, 1, 2, 3, alpha_k=[1, 2])):
        before = dict(vars(mdl))
        a = mdl.marshal(w_table=5, w_lo=-3)
        b = mdl.marshal(w_table=8, w_lo=0)
        api._marshal(A, mdl, None, True); api._marshal(A, M.ConstrainedCost(mdl, M.VertexCount(), 2), None)
        assert vars(mdl) == before, type(mdl).__name__
        if mdl.kind in (M.CP_MODEL_COLBLOCK, M.CP_MODEL_BLOCK):                    # (and the two calls did not see each other's range)
            assert (a.struct.alpha_col.lo, a.struct.alpha_col.len) == (-3, 9) and (b.struct.alpha_col.lo, b.struct.alpha_col.len) == (0, 9)
            assert mdl.marshal(w_table=5).struct.alpha_col.lo == 0


# ---------------------------------------------------------------- partition_stripe / pack_stripe: which backend call, with what
class StubBackend:
    """records every backend call and answers CP_OK"""
    name = "hip"

    def __init__(self):
        self.calls = []

    def last_error(self):
        return ""

    def __getattr__(self, meth):
        if meth.startswith("_"):
            raise AttributeError(meth)
        return lambda *args: self.calls.append((meth, args)) or 0


# written from the arms of partition_stripe / pack_stripe as they stood before the dispatch table: the backend method, the layout
# of its arguments, stack_method, when Pi is passed ("always" | "needed": only to a model with needs_rowpart | "never") and the
# refusal of a ConstrainedCost
DYN = ("partition_dynamic", "A K combine order mm rp wm wi wf arr", False, "always", None)
BCOST = ("partition_bisect_cost", "A K mm eps flip arr rp", False, "needed", "BisectCost on a ConstrainedCost errors in the reference (Costs.jl:150)")
BINDEX = ("partition_bisect_index", "A K mm flip arr rp", False, "needed", "BisectIndex on a ConstrainedCost errors in the reference (Costs.jl:150)")
PARTITION_ARMS = {
    "DynamicTotalSplitter": DYN, "DynamicBottleneckSplitter": DYN, "DynamicTotalChunker": DYN, "DynamicBottleneckChunker": DYN,
    "ReferenceTotalSplitter": DYN, "ReferenceBottleneckSplitter": DYN, "ReferenceTotalChunker": DYN,
    "BisectCostBottleneckSplitter": BCOST, "FlipBisectCostBottleneckSplitter": BCOST,
    "BisectIndexBottleneckSplitter": BINDEX, "FlipBisectIndexBottleneckSplitter": BINDEX,
    "LazyBisectCostBottleneckSplitter": ("partition_lazy_bisect_cost", "A K mm eps arr", False, "never",
                                         "LazyBisectCost on a ConstrainedCost has no method in the reference"),
    "ConvexTotalSplitter": ("partition_convex", "A K mm rp wm wi wf arr", True, "always", None),
    "ConcaveTotalSplitter": ("partition_concave", "A K mm rp wm wi wf arr", True, "always", None),
}
PACK_ARMS = {
    "DynamicTotalChunker": ("pack_dynamic", "A mm rp wm wi wf arr arr", False, "always", None),
    "ReferenceTotalChunker": ("pack_dynamic", "A mm rp wm wi wf arr arr", False, "always", None),
    "ConvexTotalChunker": ("pack_convex", "A mm rp wm wi wf arr arr", True, "always", None),
    "ConcaveTotalChunker": ("pack_concave", "A mm rp wm wi wf arr arr", True, "always", None),
}


def _make(cls, f):
    import inspect
    return cls(f, 0.25) if "eps" in inspect.signature(cls.__init__).parameters else cls(f)


@pytest.mark.parametrize("fixed_K", [True, False], ids=["partition_stripe", "pack_stripe"])
def test_dispatch_reaches_the_backend_as_the_arms_did(fixed_K):
    from chainpartitioners_jl_amd import models as M
    A = cp.SparseMatrixCSC(4, 6, np.ones(7, dtype=np.int64), np.zeros(0, dtype=np.int64))
    Pi = cp.SplitPartition(2, [1, 3, 5])
    K = 3
    run = (lambda m, Pi, b: cp.partition_stripe(A, K, m, Pi, backend=b)) if fixed_K else (lambda m, Pi, b: cp.pack_stripe(A, m, Pi, backend=b))
    plain, needs = M.ColumnBlockComponentCostModel(3, lambda w: 1 + w), M.AffinePrimaryConnectivityModel(0, 1, 1, 2, 3)
    for cname, (meth, layout, stack, pi, refusal) in (PARTITION_ARMS if fixed_K else PACK_ARMS).items():
        cls = getattr(M, cname)
        for f, constrained in ((plain, False), (needs, False), (M.ConstrainedCost(plain, M.VertexCount(), 4), True)):
            b = StubBackend()
            method = _make(cls, f)
            if constrained and refusal:
                with pytest.raises(NotImplementedError) as e:
                    run(method, Pi, b)
                assert str(e.value) == refusal and b.calls == [], cname
                continue
            P = run(method, Pi, b)
            assert isinstance(P, cp.SplitPartition) and len(b.calls) == 1 and b.calls[0][0] == meth, (cname, b.calls)
            args = dict(zip(layout.split(), b.calls[0][1]))
            assert len(b.calls[0][1]) == len(layout.split()), (cname, b.calls[0][1])
            assert args["A"] is A and args.get("K", K) == K and isinstance(args["mm"], M.Marshalled) and args["arr"].dtype == np.int64
            if "combine" in args:
                assert (args["combine"], args["order"]) == (method.combine, method.order)
            assert args.get("eps", 0.25) == 0.25 and args.get("flip", getattr(method, "flip", None)) == getattr(method, "flip", None)
            passed = pi == "always" or (pi == "needed" and f is needs)
            assert ("rp" in args) == (pi != "never") and (isinstance(args.get("rp"), M.cp_rowpart_t) if passed else args.get("rp") is None), cname
            if "wm" in args:
                assert (args["wm"] is not None) == constrained and (args["wi"], args["wf"]) == ((4, 4.0) if constrained else (0, 0.0))
            if f is plain:                                       # stack_method shows in the range the closure was tabulated for
                assert len(args["mm"].keep[0]) == (2 * A.n + 3 if stack else A.n + 2), cname
    class Other:                                               # noqa: E306
        f = plain
    with pytest.raises(NotImplementedError, match="method Other is outside the hot path"):
        run(Other(), None, StubBackend())
