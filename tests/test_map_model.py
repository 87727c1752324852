"""The host model of the two map partitioners (tests/map_model.py: the loops of the reference's src/MagneticPartitioner.jl) against
the definitions, a hand-worked example, and the package's statement of the draws.  No GPU."""
import numpy as np

import map_model as mm
import synth
from greedy_model import from_columns
from util import cp


def test_draw_is_the_generator_hash_shifted():
    from chainpartitioners_jl_amd import draws
    idx = np.concatenate([np.arange(0, 300, dtype=np.int64), np.array([2**31 - 1, 2**31, 2**40 + 7, 2**62], dtype=np.int64)])
    for seed in (0, 1, 0xDEADBEEF, 2**63 - 5):
        for stream in (1, 2, 5):
            want = (synth.hash_np(seed, stream, idx) >> np.uint64(1)).astype(np.int64)
            got = draws.draw(seed, stream, idx)
            assert got.dtype == np.int64 and got.min() >= 0 and np.array_equal(got, want)
            assert [draws.draw(seed, stream, int(i)) for i in idx[:5]] == want[:5].tolist()
    n = 50
    order = draws.greedy_order(3, n)
    keys = draws.draw(3, 2, np.arange(1, n + 1))
    assert sorted(order.tolist()) == list(range(1, n + 1)) and np.all(np.diff(keys[order - 1]) >= 0)
    assert np.array_equal(draws.magnetic_draws(3, n), draws.draw(3, 1, np.arange(1, n + 1)))


def test_method_classes():
    m = cp.MagneticPartitioner()
    assert m.seed == 0 and m.draws is None
    assert cp.MagneticPartitioner(5, draws=[1, 2, 3]).draws.dtype == np.int64
    mdl = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    g = cp.GreedyBottleneckPartitioner(mdl, seed=7)
    assert g.mdl is mdl and g.seed == 7 and g.order is None
    assert cp.GreedyBottleneckPartitioner(mdl, order=cp.DomainPermutation([2, 1, 3])).order.tolist() == [2, 1, 3]


def test_setup_counts_equal_the_definition():
    for m, density in mm.SHAPES:
        for n in (1, 3, 65, 257):
            A, T = mm.matrix(m, density, n)
            for K in mm.KS:
                mdl = mm.models(K)[3]
                for kind in ("split", "map", "domain"):
                    Pi = mm.row_partition(kind, m, K)
                    nv, npins, nr = mm.setup_counts(A, K, Pi)
                    states = [mm.greedy_setup_domain(A, T, K, Pi, mdl)] + ([mm.greedy_setup_split(A, T, K, Pi, mdl)] if kind == "split" else [])
                    for st in states:
                        assert st[0][1:] == nv.tolist() and st[1][1:] == npins.tolist() and st[3][1:] == nr.tolist() and not any(st[2])
                        assert st[4][1:] == [mdl.alpha_k[k] + 10 * nv[k] + npins[k] + 100 * nr[k] for k in range(K)]
                    assert nv.sum() == m and npins.sum() == A.nnz


def test_magnetic_takes_the_part_of_the_drawn_row():
    rng = np.random.default_rng(5)
    for m, density in mm.SHAPES:
        for n in (2, 64, 257):
            A, _ = mm.matrix(m, density, n)
            for K in (1, 5, 300):
                for kind in ("split", "map"):
                    Pi = mm.row_partition(kind, m, K)
                    pasg = cp.to_map(Pi).asg
                    u = rng.integers(0, 2**62, n)
                    asg = mm.magnetic(A, K, Pi, u)
                    for j in range(n):
                        lo, d = A.colptr[j] - 1, A.colptr[j + 1] - A.colptr[j]
                        if d == 0:
                            assert asg[j] == 1 + u[j] % K
                        else:
                            assert asg[j] == pasg[A.rowval[lo + u[j] % d] - 1]
                            assert asg[j] in set(pasg[A.rowval[lo:lo + d] - 1].tolist())


def test_greedy_hand_worked_example():
    """4 x 5, rows {1, 2} in part 1 and {3, 4} in part 2, cost 10 nv + np + 100 nr.  Setup: nv = (2, 2), np = (3, 4), nr = (3, 3), cst =
    (323, 324).  Column 1 = rows {1, 3}: part 2 (324 > 323), cst_2 = 24 + 200 = 224.  Column 2 = {2}: part 1, cst_1 = 23 + 200 = 223.
    Column 3 = {3, 4}: part 2, cst_2 = 124.  Column 4 is empty: part 1, nothing changes.  Column 5 = {1, 4}: part 1 (223 > 124), cst_1 = 123."""
    A = from_columns(4, [np.array(c, dtype=np.int64) for c in ([0, 2], [1], [2, 3], [], [0, 3])])
    mdl = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    order = np.arange(1, 6)
    for Pi in (cp.SplitPartition(2, [1, 3, 5]), cp.MapPartition(2, [1, 1, 2, 2]), cp.to_domain(cp.MapPartition(2, [1, 1, 2, 2]))):
        asg, cst = mm.greedy(A, 2, Pi, mdl, order)
        assert asg.tolist() == [2, 1, 2, 1, 1] and cst.tolist() == [123, 124]
        assert cst.tolist() == mm.secondary_costs(A, 2, Pi, cp.MapPartition(2, asg), mdl).tolist()
        asg0, cst0 = mm.greedy(A, 2, Pi, mdl, order, update=False)
        assert asg0.tolist() == [2, 1, 2, 1, 2] and cst0.tolist() == [323, 324]
    # ties: the first entry in column order among the maxima; visiting order matters
    flat = cp.AffineSecondaryConnectivityModel(0, 0, 0, 0, 1)
    asg, cst = mm.greedy(A, 2, cp.SplitPartition(2, [1, 3, 5]), flat, order)
    assert asg.tolist() == [1, 1, 2, 1, 2] and cst.tolist() == [1, 1]
    asg, _ = mm.greedy(A, 2, cp.SplitPartition(2, [1, 3, 5]), flat, order[::-1])
    assert asg.tolist() == [2, 1, 2, 1, 1]


def test_final_costs_are_the_definition_and_the_update_matters():
    """every final cost equals the secondary model's cost of the returned column sets; and in at least half of the family the result
    differs from the loop without the cost update (a scratch run of this family: 401 of 600; n = 1 and K = 1 cannot differ), so
    a kernel that forgets the update cannot pass the parity tests"""
    from chainpartitioners_jl_amd import draws
    differ = total = 0
    for idx, (m, density, n, K, c, kind) in enumerate(mm.family()):
        A, T = mm.matrix(m, density, n)
        mdl, Pi = mm.models(K)[c], mm.row_partition(kind, m, K)
        setup = mm.greedy_setup_split if kind == "split" else mm.greedy_setup_domain
        state = setup(A, T, K, Pi, mdl)
        order = draws.greedy_order(idx, n)
        asg, cst = mm.greedy_walk(A, K, Pi, mdl, order, state)
        asg0, _ = mm.greedy_walk(A, K, Pi, mdl, order, state, update=False)
        total += 1
        differ += not np.array_equal(asg, asg0)
        if n <= 65:
            assert cst.tolist() == mm.secondary_costs(A, K, Pi, cp.MapPartition(K, asg), mdl).tolist()
    assert total == 600 and 2 * differ >= total, (differ, total)
