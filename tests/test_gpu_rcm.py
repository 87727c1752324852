"""cp_rcm and cp_csr_permute on the device (csrc/rcm.hip): permute_plaid(A, CuthillMcKeePermuter(...)) bit for bit against the host
models of tests/rcm_model.py -- forwards and reversed, with the one-workgroup walker forced off, forced on and at its default -- and
A[sigma, tau] against the numpy construction.  The small cases and the three fixture matrices are held against the reference's
loops (model A); the large ones against the key form (model B), which tests/test_rcm_model.py holds against A."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

from util import cp, golden_matrices, banded, HERE
from rcm_model import permute_plaid_model, rcm_loops, rcm_keys, permuted, from_mask, tying_pattern, is_symmetric

gpu = pytest.mark.gpu

DEFAULT_NARROW = 256                   # the library's default of the option "rcm_narrow" (csrc/rcm.hip)
WALK_NODES, WALK_EDGES = 1024, 4096    # the walker's capacity (csrc/rcm.hip)
SETTINGS = {"off": 0, "on": 1 << 20, "default": DEFAULT_NARROW}
CP_EINVAL = 1


@contextlib.contextmanager
def narrow(hip, value):
    hip.set_option("rcm_narrow", value)
    try:
        yield
    finally:
        hip.set_option("rcm_narrow", DEFAULT_NARROW)


def from_edges(n, u, v, diag=None):
    """the symmetric n x n pattern with the entries (u, v) and (v, u) (0-based arrays) and the diagonal entries `diag`"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    d = np.zeros(0, dtype=np.int64) if diag is None else np.asarray(diag, dtype=np.int64)
    key = np.unique(np.concatenate([u * n + v, v * n + u, d * n + d]))       # column * n + row
    cols, rows = key // n, key % n
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, rows + 1)


def random_symmetric(n, seed):
    """many trees: a few edges, a few diagonal entries, the rest of the vertices alone"""
    rng = np.random.default_rng(seed)
    e = n // 2
    return from_edges(n, rng.integers(0, n, e), rng.integers(0, n, e), rng.integers(0, n, max(n // 4, 1)))


def path_graph(n):
    return from_edges(n, np.arange(n - 1), np.arange(1, n))


HUB = WALK_EDGES + 904                 # the hub's column is beyond the walker's edge capacity
LONG_TAILS, TAIL = 9, 5


def star_with_tails():
    """hub 0, leaves 1 .. HUB; every leaf carries a tail of one vertex, LONG_TAILS of them a tail of TAIL vertices.  From a tail's
    end the walk is narrow up to the hub, wide over the hub and its leaves, and narrow again along the long tails."""
    u, v = [np.zeros(HUB, dtype=np.int64)], [np.arange(1, HUB + 1)]
    nxt = HUB + 1
    for leaf in range(1, HUB + 1):
        length = TAIL if leaf % (HUB // LONG_TAILS) == 1 else 1
        chain = np.concatenate([[leaf], np.arange(nxt, nxt + length)])
        u.append(chain[:-1]); v.append(chain[1:])
        nxt += length
    return from_edges(nxt, np.concatenate(u), np.concatenate(v))


def small_star(hub, every):
    """hub 0 with `hub` leaves, every `every`-th of them with one more vertex behind it: one level of `hub` candidates of two degrees
    inside the walker (up to 256 of them are ranked, more are sorted by the bitonic network)"""
    leaves = np.arange(1, hub + 1)
    tailed = leaves[::every]
    return from_edges(hub + 1 + len(tailed), np.concatenate([np.zeros(hub, dtype=np.int64), tailed]),
                      np.concatenate([leaves, hub + 1 + np.arange(len(tailed))]))


def rectangular(m, n, seed, p=None):
    rng = np.random.default_rng(seed)
    D = rng.random((m, n)) < (2.5 / max(m, n) if p is None else p)
    D[rng.random(m) < 0.2, :] = False
    D[:, rng.random(n) < 0.2] = False
    return from_mask(D)


def nonsymmetric_square(n, seed):
    rng = np.random.default_rng(seed)
    D = rng.random((n, n)) < 2.0 / n
    A = from_mask(D)
    assert not is_symmetric(A)
    return A


TYING_SQUARE_SEED = 2                  # a seed of tying_pattern whose pattern is square (34 x 34), not symmetric, with several trees

CASES = {
    "can_292": lambda: (golden_matrices()["HB/can_292"], {}, rcm_loops),
    "west0132": lambda: (golden_matrices()["HB/west0132"], {}, rcm_loops),
    "lp_etamacro": lambda: (golden_matrices()["LPnetlib/lp_etamacro"], {}, rcm_loops),
    **{f"random_symmetric_{n}": (lambda n=n: (random_symmetric(n, 40 + n), {}, rcm_loops)) for n in (1, 2, 3, 8, 65, 300)},
    "all_empty": lambda: (from_mask(np.zeros((300, 300), dtype=bool)), {}, rcm_loops),
    "diagonal_only": lambda: (from_mask(np.eye(257, dtype=bool)), {}, rcm_loops),
    "path_3000": lambda: (path_graph(3000), {}, rcm_keys),
    "small_star_200": lambda: (small_star(200, 3), {}, rcm_loops),
    "small_star_600": lambda: (small_star(600, 3), {}, rcm_loops),
    "small_star_1500": lambda: (small_star(1500, 7), {}, rcm_keys),
    "star_with_tails": lambda: (star_with_tails(), {}, rcm_keys),
    "banded_4096": lambda: (banded(4096, 3, 0.7, 5), {}, rcm_keys),
    "banded_4096_assume": lambda: (banded(4096, 3, 0.7, 5), {"assumesymmetry": True}, rcm_keys),
    "rectangular_37x90": lambda: (rectangular(37, 90, 1), {}, rcm_loops),
    "rectangular_300x70": lambda: (rectangular(300, 70, 2), {}, rcm_loops),
    "rectangular_unchecked": lambda: (random_symmetric(65, 9), {"checksymmetry": False}, rcm_loops),      # symmetric, walked as bipartite
    "tying_rectangular": lambda: (tying_pattern(7, False), {}, rcm_loops),
    "nonsymmetric_assume": lambda: (nonsymmetric_square(200, 3), {"assumesymmetry": True}, rcm_loops),
    "tying_square_assume": lambda: (tying_pattern(TYING_SQUARE_SEED, False), {"assumesymmetry": True}, rcm_loops),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the pattern, the permuter's keywords and the model's answers for both directions, computed once"""
    A, kw, walk = CASES[name]()
    return A, kw, {rev: permute_plaid_model(A, reverse=rev, walk=walk, **kw) for rev in (False, True)}


def device_perms(hip, A, kw, reverse):
    s, t = cp.permute_plaid(A, cp.CuthillMcKeePermuter(reverse=reverse, **kw), backend=hip)
    return s, t, dict(hip.last_rcm_stats)


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_model(hip, name, setting):
    A, kw, want = case(name)
    with narrow(hip, SETTINGS[setting]):
        for reverse in (False, True):
            s, t, stats = device_perms(hip, A, kw, reverse)
            iprm, jprm, sym, trees = want[reverse]
            assert s.prm.dtype == np.int64 and np.array_equal(s.prm, iprm), (name, setting, reverse, stats)
            assert np.array_equal(t.prm, jprm), (name, setting, reverse, stats)
            assert (s is t) == sym and stats["path"] == (1 if sym else 2)
            assert stats["trees"] == trees, (name, setting, stats)
            if setting == "off":
                assert stats["walker_launches"] == 0, stats
            assert cp.permute_stripe(A, cp.CuthillMcKeePermuter(reverse=reverse, **kw), backend=hip) == t


@gpu
@pytest.mark.parametrize("name", ["can_292", "west0132", "lp_etamacro"])
def test_fixtures_equal_committed_permutations(hip, name):
    gold = json.load(open(os.path.join(HERE, "golden", "rcm.json")))
    full = {"can_292": "HB/can_292", "west0132": "HB/west0132", "lp_etamacro": "LPnetlib/lp_etamacro"}[name]
    A = golden_matrices()[full]
    for reverse in (False, True):
        g = gold[f"{full},reverse={int(reverse)}"]
        s, t, stats = device_perms(hip, A, {}, reverse)
        assert s.prm.tolist() == g["rowprm"] and t.prm.tolist() == g["colprm"] and (s is t) == g["symmetric"] and stats["trees"] == g["trees"]


@gpu
def test_regimes_hand_over(hip):
    """the path graph runs in ONE walker launch when the walker is on; the star leaves the walker at the hub (its column is beyond the
    edge capacity), runs wide over the leaves and goes back to the walker for the long tails"""
    A, kw, want = case("path_3000")
    with narrow(hip, SETTINGS["on"]):
        _, _, stats = device_perms(hip, A, kw, False)
    assert stats["walker_launches"] == 1 and stats["wide_levels"] == 0 and stats["trees"] == 1, stats
    with narrow(hip, SETTINGS["off"]):
        _, _, stats = device_perms(hip, A, kw, False)
    assert stats["walker_launches"] == 0 and stats["wide_levels"] == stats["levels"] == rcm_keys(A.colptr - 1, A.rowval - 1, A.n)[2], stats
    A, kw, want = case("star_with_tails")
    assert HUB > WALK_EDGES and HUB > WALK_NODES
    with narrow(hip, SETTINGS["on"]):
        _, _, stats = device_perms(hip, A, kw, False)
    assert stats["walker_launches"] >= 2 and 2 <= stats["wide_levels"] < stats["levels"], stats
    assert stats["levels"] == rcm_keys(A.colptr - 1, A.rowval - 1, A.n)[2], stats


@gpu
def test_adjoint_handle_is_used_and_checked(hip):
    A, kw, want = case("rectangular_37x90")
    T = cp.adjointpattern(A, backend=hip)
    s, t = cp.permute_plaid(A, cp.CuthillMcKeePermuter(), adj_A=T, backend=hip)
    assert np.array_equal(s.prm, want[False][0]) and np.array_equal(t.prm, want[False][1])
    rc, _, _, _ = hip.rcm(A, A, 0, False)                                   # not the adjoint's shape
    assert rc == CP_EINVAL


@gpu
def test_bad_arguments_return(hip):
    A = rectangular(37, 90, 1)
    rc, _, _, _ = hip.rcm(A, None, 1, False)                                # assumesymmetry with m != n
    assert rc == CP_EINVAL and "square" in hip.last_error()
    with pytest.raises(AssertionError):
        cp.permute_plaid(A, cp.CuthillMcKeePermuter(assumesymmetry=True), backend=hip)
    rc, _, _, _ = hip.rcm(A, None, 3, False)
    assert rc == CP_EINVAL
    ident_r, ident_c = np.arange(1, A.m + 1), np.arange(1, A.n + 1)
    for rows, cols in ((np.where(ident_r == 2, 1, ident_r), None),          # a repeated index
                       (None, np.where(ident_c == 90, 89, ident_c)),
                       (np.where(ident_r == 5, A.m + 1, ident_r), None),    # out of range
                       (np.where(ident_r == 5, 0, ident_r), None),
                       (None, np.where(ident_c == 1, -(2 ** 40), ident_c)),
                       (None, np.where(ident_c == 1, 2 ** 40, ident_c))):
        rc, B = hip.csr_permute(A, rows, cols)
        assert rc == CP_EINVAL and B is None and "permutation" in hip.last_error()
    with pytest.raises(AssertionError):
        cp.permute(A, cp.DomainPermutation(np.where(ident_r == 2, 1, ident_r)), backend=hip)
    with pytest.raises(ValueError):
        hip.csr_permute(A, ident_c, None)                                   # the wrong length never reaches the library


# ---------------------------------------------------------------- cp_csr_permute
def same_pattern(B, want):
    return (B.m, B.n) == (want.m, want.n) and np.array_equal(B.colptr, want.colptr) and np.array_equal(B.rowval, want.rowval)


PERMUTE_CASES = {
    "rectangular_37x90": lambda: rectangular(37, 90, 1),
    "rectangular_300x70": lambda: rectangular(300, 70, 2),
    "lp_etamacro": lambda: golden_matrices()["LPnetlib/lp_etamacro"],
    "can_292": lambda: golden_matrices()["HB/can_292"],
    "one_by_one": lambda: from_mask(np.ones((1, 1), dtype=bool)),
    "all_empty": lambda: from_mask(np.zeros((5, 9), dtype=bool)),
    "wide_1300": lambda: rectangular(3, 1300, 6, 0.5),                         # more than one block of columns and of entries
}


@gpu
@pytest.mark.parametrize("name", list(PERMUTE_CASES))
def test_permute_equals_numpy(hip, name):
    A = PERMUTE_CASES[name]()
    rng = np.random.default_rng(17)
    s = cp.DomainPermutation(rng.permutation(A.m) + 1)
    t = cp.DomainPermutation(rng.permutation(A.n) + 1)
    for sigma, tau in ((s, t), (s, None), (None, t), (None, None), (cp.to_map_permutation(s), t),
                       (cp.DomainPermutation(np.arange(1, A.m + 1)), cp.DomainPermutation(np.arange(1, A.n + 1)))):
        B = cp.permute(A, sigma, tau, backend=hip)
        want = permuted(A, None if sigma is None else cp.perm(sigma), None if tau is None else cp.perm(tau))
        assert same_pattern(B, want), (name, sigma is None, tau is None)
        assert B.colptr.dtype == np.int64 and B.rowval.dtype == np.int64
    # the result keeps its device handle: it is partitioned without an upload and downloads as itself
    B = cp.permute(A, s, t, backend=hip)
    assert id(B) in hip._handles
    T = cp.adjointpattern(B, backend=hip)
    assert same_pattern(cp.adjointpattern(T, backend=hip), B)


@gpu
def test_permute_by_rcm_narrows_the_band(hip):
    """test/test_CuthillMcKee.jl:38-39 with both steps on the device"""
    from rcm_model import bandwidth, transpose
    for name in ("HB/can_292", "HB/west0132", "LPnetlib/lp_etamacro"):
        A = golden_matrices()[name]
        s, t = cp.permute_plaid(A, cp.CuthillMcKeePermuter(), backend=hip)
        B = cp.permute(A, s, t, backend=hip)
        assert bandwidth(B) < bandwidth(A) and bandwidth(transpose(B)) < bandwidth(transpose(A))
