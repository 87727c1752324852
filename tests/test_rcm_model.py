"""The reordering layer on the host (no library needed): the reference's Cuthill-McKee loops (model A of tests/rcm_model.py) against
the key statement the device implements (model B), the reference's own properties (test/test_CuthillMcKee.jl) on the three committed
matrices, the committed permutations (tests/golden/rcm.json), and the permutation algebra of chainpartitioners.jl_amd/types.py."""
import functools
import json
import os

import numpy as np
import pytest

from util import cp, golden_matrices, HERE
from rcm_model import (rcm_loops, rcm_keys, sym_graph, bip_graph, is_symmetric, permute_plaid_model, permuted, bandwidth, transpose,
                       tying_pattern, from_mask)

NAMES = ("HB/can_292", "HB/west0132", "LPnetlib/lp_etamacro")
SEEDS = range(2400)


@functools.lru_cache(maxsize=None)
def tying(seed):
    return tying_pattern(seed, symmetric=seed % 3 == 0)


def same_walk(g):
    a, ta = rcm_loops(*g)
    b, tb, _ = rcm_keys(*g)
    return np.array_equal(a, b) and ta == tb and np.array_equal(np.sort(a), np.arange(g[2]))


def test_stable_sort_claim_on_tying_patterns():
    """The block reordering of CuthillMcKeePermuter.jl:60-77 is a stable ascending sort by degree: the loops (A) and the walk by
    (parent position, degree, index) (B) give one queue and one tree count -- on the bipartite graph of every pattern, and on the
    column graph of every square one, symmetric or not (the directed walk assumesymmetry makes)."""
    walks = square = asym = rect = 0
    for seed in SEEDS:
        A = tying(seed)
        assert same_walk(bip_graph(A)), seed
        walks += 1
        rect += A.m != A.n
        if A.m == A.n:
            assert same_walk(sym_graph(A)), seed
            walks += 1
            square += 1
            asym += not is_symmetric(A)
    assert walks >= 2000 and square >= 500 and asym >= 100 and rect >= 500, (walks, square, asym, rect)


def test_tying_patterns_do_tie():
    """a condition on the inputs: most patterns have a repeated degree, several trees, an empty column and a diagonal-only column
    somewhere in the family"""
    tied = forests = empty = diag = 0
    for seed in SEEDS:
        A = tying(seed)
        dg = np.diff(A.colptr)
        tied += len(set(dg.tolist())) < A.n
        forests += rcm_keys(*bip_graph(A))[1] > 1
        empty += bool((dg == 0).any())
        k = min(A.m, A.n)
        diag += any(dg[j] == 1 and A.rowval[A.colptr[j] - 1] == j + 1 for j in range(k))
    n = len(SEEDS)
    assert tied > 0.9 * n and forests > 0.5 * n and empty > 0.3 * n and diag > 0.2 * n, (tied, forests, empty, diag)


def test_permute_plaid_models_agree():
    for seed in range(0, 600):
        A = tying(seed)
        for reverse in (False, True):
            for kw in ({}, {"checksymmetry": False}) + (({"assumesymmetry": True},) if A.m == A.n else ()):
                a = permute_plaid_model(A, reverse=reverse, walk=rcm_loops, **kw)
                b = permute_plaid_model(A, reverse=reverse, walk=rcm_keys, **kw)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:], (seed, reverse, kw)


@functools.lru_cache(maxsize=None)
def fixture_perms(name, reverse):
    return permute_plaid_model(golden_matrices()[name], reverse=reverse)


@pytest.mark.parametrize("name", NAMES)
def test_reference_properties(name):
    """test/test_CuthillMcKee.jl:25-54"""
    A = golden_matrices()[name]
    s, t, sym, _ = fixture_perms(name, False)
    sr, tr, _, _ = fixture_perms(name, True)
    assert np.array_equal(s, sr[::-1]) and np.array_equal(t, tr[::-1])
    assert sym == (name == "HB/can_292")
    if sym:
        assert s is t
    B = permuted(A, s, t)
    assert bandwidth(B) < bandwidth(A)
    assert bandwidth(transpose(B)) < bandwidth(transpose(A))


@pytest.mark.parametrize("name", NAMES)
def test_golden_permutations(name):
    gold = json.load(open(os.path.join(HERE, "golden", "rcm.json")))
    for reverse in (False, True):
        g = gold[f"{name},reverse={int(reverse)}"]
        s, t, sym, trees = fixture_perms(name, reverse)
        assert s.tolist() == g["rowprm"] and t.tolist() == g["colprm"] and sym == g["symmetric"] and trees == g["trees"]


def test_permuted_is_fancy_indexing():
    rng = np.random.default_rng(5)
    D = rng.random((7, 11)) < 0.3
    A = from_mask(D)
    s, t = rng.permutation(7) + 1, rng.permutation(11) + 1
    assert np.array_equal(cp_dense(permuted(A, s, t)), D[np.ix_(s - 1, t - 1)])
    assert np.array_equal(cp_dense(permuted(A, None, t)), D[:, t - 1])
    assert np.array_equal(cp_dense(permuted(A, s, None)), D[s - 1, :])


def cp_dense(A):
    D = np.zeros((A.m, A.n), dtype=bool)
    for j in range(A.n):
        D[A.rowval[A.colptr[j] - 1:A.colptr[j + 1] - 1] - 1, j] = True
    return D


# ---------------------------------------------------------------- Permutations.jl against numpy
def test_permutation_types():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 9, 40):
        p = rng.permutation(n).astype(np.int64) + 1
        s = cp.DomainPermutation(p)
        inv = np.argsort(p - 1).astype(np.int64) + 1          # numpy's inverse permutation
        assert np.array_equal(cp.invperm(p), inv)
        mp = cp.to_map_permutation(s)
        assert isinstance(mp, cp.MapPermutation) and np.array_equal(mp.asg, inv)
        assert cp.to_domain_permutation(mp) == s and cp.to_domain_permutation(s) is s and cp.to_map_permutation(mp) is mp
        assert np.array_equal(cp.perm(s), p) and np.array_equal(cp.perm(mp), p)
        assert s == cp.DomainPermutation(p.copy()) and mp == cp.MapPermutation(inv.copy())
        assert not (s == mp)
        if n >= 2:
            q = p.copy(); q[[0, 1]] = q[[1, 0]]
            assert s != cp.DomainPermutation(q)
    for bad in ([1, 1], [0, 1], [1, 3], [2, 3]):
        with pytest.raises(ValueError):
            cp.invperm(bad)


def test_permutation_applied_to_partitions():
    """sigma[Pi] (Permutations.jl:43-53): B = A[perm(sigma)]; a partition of B's indices told in A's"""
    rng = np.random.default_rng(4)
    n, K = 23, 4
    p = rng.permutation(n).astype(np.int64) + 1
    spl = np.array([1, 6, 6, 15, 24], dtype=np.int64)
    for s in (cp.DomainPermutation(p), cp.to_map_permutation(cp.DomainPermutation(p))):
        Pi = cp.SplitPartition(K, spl)
        got = s[Pi]
        assert isinstance(got, cp.DomainPartition) and np.array_equal(got.prm, p) and np.array_equal(got.spl, spl)
        # the part of original index p[i'] is the part of position i'
        asg_b = cp.to_map(Pi).asg
        want = np.zeros(n, dtype=np.int64)
        want[p - 1] = asg_b
        assert np.array_equal(cp.to_map(got).asg, want)
        # a DomainPartition of B: its prm composed with the permutation
        q = rng.permutation(n).astype(np.int64) + 1
        got = s[cp.DomainPartition(K, q, spl)]
        assert np.array_equal(got.prm, q[p - 1]) and np.array_equal(got.spl, spl)
        # a MapPartition: asg[invperm(perm(sigma))], as the reference writes it
        asg = rng.integers(1, K + 1, size=n).astype(np.int64)
        got = s[cp.MapPartition(K, asg)]
        assert isinstance(got, cp.MapPartition) and np.array_equal(got.asg, asg[np.argsort(p - 1)])
    with pytest.raises(TypeError):
        cp.DomainPermutation(p)[3]


def test_identity_permuter_and_method_types():
    A = golden_matrices()["LPnetlib/lp_blend"]
    s, t = cp.permute_plaid(A, cp.IdentityPermuter())
    assert np.array_equal(s.prm, np.arange(1, A.m + 1)) and np.array_equal(t.prm, np.arange(1, A.n + 1))
    assert cp.permute_stripe(A, cp.IdentityPermuter()) == t
    m = cp.CuthillMcKeePermuter()
    assert (m.reverse, m.assumesymmetry, m.checksymmetry) == (False, False, True)
    m = cp.CuthillMcKeePermuter(reverse=True, assumesymmetry=True, checksymmetry=False)
    assert (m.reverse, m.assumesymmetry, m.checksymmetry) == (True, True, False)
    pp = cp.PermutingPartitioner(m, cp.EquiSplitter())
    assert pp.prm is m and isinstance(pp.prt, cp.EquiSplitter)
    with pytest.raises(NotImplementedError):
        cp.permute_plaid(A, object())
