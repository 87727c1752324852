"""The merge of the own-tile partials of a DP round (csrc/dp_total_own.hip, k_fix_own): one launch, a lane per task of up to
FIX_SERIAL tiles, a block per (task, trip of 2 048 tiles) item of the longer ones, the trips of a task folded by whichever block
finishes last.

 * through cp_test_fix_merge against a serial numpy merge (a running base over all of a task's tiles, smallest value, then
   largest column), tile counts on both sides of every split of the kernel, three launches on one workspace;
 * through cp_dp_layer against the path without own tiles, at sizes whose top task is one trip and four trips;
 * around a layer whose rounds are all dropped by their verdict.
"""
import functools

import numpy as np
import pytest
import torch

from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

FIX_SERIAL = 16          # csrc/dp_total.hpp: tasks of up to FIX_SERIAL tiles are merged by one lane
TRIP = 2048              # ... longer ones in trips of 256 * FIX_U tiles, one block each
MODELS = [cp.AffineConnectivityModel(1, 10, 1, 100), cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3),
          cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0), cp.AffineHyperedgeCutModel(0.0, 1.0, 0.0, -1.0, 2.0)]
IDS = ["conn-i64", "hyper-i64", "conn-f64", "hyper-f64"]
LAYER_MODELS = MODELS + [cp.AffineWorkModel(1, 10, 1)]
LAYER_IDS = IDS + ["work-i64"]

# tile counts per task: both sides of the lane / block split, of one / two trips, a second trip of one tile, whole trips, a
# ragged third trip, more trips than the top task of the bench configuration (32 768 tiles), and a crowd of short tasks (several
# lane blocks, tasks between the listed ones)
NT_EDGES = [1, FIX_SERIAL, FIX_SERIAL + 1, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP, 2 * TRIP + 1, 3 * TRIP + 5, 40_000]
ALL_EMPTY, EMPTY_TRIP_1, EMPTY_TRIP_0 = 10, 11, 12       # tasks added below: no candidate at all / none in the second / in the first trip


def is_hyp(mdl):
    return isinstance(mdl, cp.AffineHyperedgeCutModel)


def base_cost(mdl, base, base2):
    """what the counts made before a tile add to its winner: the model's net terms (exact integers in either element type)"""
    if is_hyp(mdl):
        return int(mdl.beta_self_net) * base2 + int(mdl.beta_cut_net) * (base - base2)
    return int(mdl.beta_net) * base


def make_case(mdl, seed):
    rng = np.random.default_rng(seed)
    nts = NT_EDGES + [2 * TRIP + 1, 2 * TRIP + 1, 2 * TRIP + 1] + [int(x) for x in rng.integers(1, 40, 700)] + [TRIP + 7, FIX_SERIAL + 1, 5 * TRIP]
    order = rng.permutation(len(nts))
    where = {int(old): new for new, old in enumerate(order)}          # the listed tasks sit anywhere among the short ones
    nts = np.asarray(nts, dtype=np.int64)[order]
    toffs = np.concatenate([[0], np.cumsum(nts)])
    NT = int(toffs[-1])
    # counts of up to 2^21 per tile: the base of the 40 000-tile task passes 2^31 (nn wraps as the kernels' int32 does) while
    # 100 * base stays far below 2^53
    tile_s = rng.integers(0, 1 << 21, NT).astype(np.int32)
    tile_s2 = rng.integers(0, 1 << 20, NT).astype(np.int32)
    anchor = rng.integers(0, 1 << 20, len(nts)).astype(np.int32)
    anchor2 = rng.integers(0, 1 << 19, len(nts)).astype(np.int32)
    part_p = rng.permutation(NT).astype(np.int32)                      # distinct columns in no order: ties fall either way across trips
    part_p[rng.random(NT) < 0.1] = -1                                  # tiles without a candidate, in places
    for t, trips in ((ALL_EMPTY, (0, 1, 2)), (EMPTY_TRIP_1, (1,)), (EMPTY_TRIP_0, (0,))):
        k0 = int(toffs[where[t]])
        for j in trips:
            part_p[k0 + j * TRIP:min(k0 + (j + 1) * TRIP, int(toffs[where[t] + 1]))] = -1
    part_nn = rng.integers(0, 1000, NT).astype(np.int32)
    part_nl = rng.integers(0, 1000, NT).astype(np.int32)
    # totals from a handful of values: every task of some length has equal minima in several tiles, the long ones in several trips
    total = rng.integers(0, 4, NT).astype(np.int64) + 1_000_000
    part_v = np.zeros(NT, dtype=np.int64)
    want = []
    for t in range(len(nts)):
        k0, k1 = int(toffs[t]), int(toffs[t + 1])
        base = int(anchor[t]) + np.concatenate([[0], np.cumsum(tile_s[k0:k1 - 1].astype(np.int64))])
        base2 = int(anchor2[t]) + np.concatenate([[0], np.cumsum(tile_s2[k0:k1 - 1].astype(np.int64))]) if is_hyp(mdl) else 0 * base
        part_v[k0:k1] = total[k0:k1] - base_cost(mdl, base, base2)
        # the serial merge: running base, smallest total, then largest column
        live = np.flatnonzero(part_p[k0:k1] >= 0)
        if live.size == 0:
            want.append((-1, 0, 0))
        else:
            i = int(live[np.lexsort((-part_p[k0:k1][live].astype(np.int64), total[k0:k1][live]))[0]])
            wrap = lambda x: (x + 2**31) % 2**32 - 2**31                # (the records carry int32 counts)
            want.append((int(part_p[k0 + i]), wrap(int(part_nn[k0 + i]) + int(base[i])), wrap(int(part_nl[k0 + i]) + int(base2[i]))))
    items = int(sum(-(-int(x) // TRIP) for x in nts if x > FIX_SERIAL))
    trips = int(sum(1 for x in nts if x > TRIP))
    return dict(toffs=toffs, part_v=part_v, part_p=part_p, part_nn=part_nn, part_nl=part_nl, tile_s=tile_s, tile_s2=tile_s2, anchor=anchor,
                anchor2=anchor2, want=want, items=items, trips=trips, ntask=len(nts))


@pytest.mark.parametrize("mi", range(len(MODELS)), ids=IDS)
def test_merge_launch_against_serial_numpy(hip, mi):
    """every task's winner, its counts, the item / trip / edge statistics and the tickets after three launches on one workspace"""
    mdl = MODELS[mi]
    c = make_case(mdl, 70 + mi)
    hyp = is_hyp(mdl)
    ntask = c["ntask"]
    n = ntask + 5
    row = np.arange(1, ntask + 1, dtype=np.int32)
    plane = (np.arange(ntask) % 3).astype(np.int32)
    part_v = c["part_v"].astype(np.float64) if mdl.dtype != cp.models.CP_I64 else c["part_v"]
    assert np.array_equal(part_v.astype(np.int64), c["part_v"])       # (integral Float64 costs, exactly)
    assert hip.set_option("stat_reset", 1) == 0
    p, nn, nl, res = hip.test_fix_merge(mdl.marshal(), c["toffs"], part_v, c["part_p"], c["part_nn"], c["part_nl"] if hyp else None, c["tile_s"],
                                        c["tile_s2"] if hyp else None, c["anchor"], c["anchor2"] if hyp else None, row, plane, n, reps=3)
    print("items %d (expected %d), folded tasks %d (expected %d), edges %d, tickets left %d" % (res["items"], c["items"], res["trips"], c["trips"],
                                                                                              res["edges"], res["tickets_left"]))
    want_p = np.array([w[0] for w in c["want"]], dtype=np.int32)
    want_nn = np.array([w[1] for w in c["want"]], dtype=np.int32)
    assert np.array_equal(p, want_p)
    assert np.array_equal(nn, want_nn)
    if hyp:
        assert np.array_equal(nl, np.array([w[2] for w in c["want"]], dtype=np.int32))
    assert res == {"items": c["items"], "trips": c["trips"], "edges": 7, "tickets_left": 0}
    assert hip.get_stat("fix_items") == 3 * c["items"]


# ---- through the layer: own tiles against the path without them
def w_rows(rng, n, dt, scale=1_000_000):
    """an arbitrary, a monotone and two flat-with-wells previous layers (arg-min staircases whose steps -- the task lengths -- run
    from a few candidates to thousands of tiles)"""
    rows = [rng.integers(0, scale + 1, n + 1), np.sort(rng.integers(0, scale + 1, n + 1))]
    for dens in (1.0 / 4096, 1.0 / 65536):
        rows.append(np.where(rng.random(n + 1) < dens, 0, scale * 8).astype(np.int64))
    return [r.astype(dt) for r in rows]


def run(hip, A, mdl, steps, stats=None):
    """steps: (W, dbg) per layer, on ONE DP handle (each layer is sized from the one before).  Returns (cst, ptr) per step; stats: a
    list that receives (fix_items, spec_redo) as they stand after every layer."""
    n = A.n
    dev = torch.device("cuda", 0)
    dt = torch.int64 if mdl.dtype == cp.models.CP_I64 else torch.float64
    dp = hip.dp_begin(A, 3, 0, 0, mdl.marshal(), 1, n + 2)
    out = []
    try:
        for W, dbg in steps:
            assert hip.set_option("dbg", dbg) == 0
            prev = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
            cur = torch.zeros(n + 1, dtype=dt, device=dev)
            hip.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
            out.append((cur.cpu().numpy(), hip.dp_ptr_row(dp, 2, n)))
            if stats is not None:
                stats.append((hip.get_stat("fix_items"), hip.get_stat("spec_redo")))
    finally:
        hip.set_option("dbg", 0)
        hip.dp_destroy(dp)
    return out


def same(got, want):
    for (c0, p0), (c1, p1) in zip(got, want):
        assert np.array_equal(p0, p1)
        assert np.array_equal(c0, c1)


@functools.lru_cache(maxsize=1)
def matrix(n):
    return suitesparse_shaped(n, 3, 21)


@pytest.mark.parametrize("mi", range(len(LAYER_MODELS)), ids=LAYER_IDS)
@pytest.mark.parametrize("lg,top_trips", [(20, 1), (22, 4)])
def test_layer_with_own_tiles_against_the_path_without(hip, lg, top_trips, mi):
    """n = 2^lg + 3: the top rectangle's last row owns a task over its whole block of 2^(lg - 1) columns -- 2 048 tiles, one trip,
    finished by its block; 8 192 tiles, four trips, folded by the last of four blocks"""
    n = (1 << lg) + 3
    A = matrix(n)
    mdl = LAYER_MODELS[mi]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    Ws = w_rows(np.random.default_rng(80 + mi), n, dt)
    if lg > 20:
        Ws = [Ws[0], Ws[3]]                                     # (the larger size: an arbitrary row and the one with the longest tasks)
    assert hip.set_option("stat_reset", 1) == 0
    got = run(hip, A, mdl, [(W, 0) for W in Ws])
    trips, items = hip.get_stat("fix_trips"), hip.get_stat("fix_items")
    want = run(hip, A, mdl, [(W, 64) for W in Ws])
    assert (hip.get_stat("fix_trips"), hip.get_stat("fix_items")) == (trips, items)       # the reference path has no tiles of its own
    print("tasks folded from more than one trip: %d, items: %d" % (trips, items))
    assert items >= top_trips
    if top_trips > 1:
        assert trips > 0
    same(got, want)


@pytest.mark.parametrize("mi", range(len(MODELS)), ids=IDS)
def test_a_dropped_round_lists_no_items(hip, mi):
    """a layer whose buffers are declared too small (dbg 2048: every round dropped by its verdict, the layer redone) followed by a
    normal layer: the same tables as without it, and the dropped attempt adds nothing to the items counted.  (fix_items counts
    every attempt of a layer; all layers get the same previous row, so no layer but the marked one is mispredicted and redone.)"""
    n = 70_001
    A = suitesparse_shaped(n, 5, 3)
    mdl = MODELS[mi]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    W = w_rows(np.random.default_rng(90 + mi), n, dt)[2]
    assert hip.set_option("stat_reset", 1) == 0
    st = []
    got = run(hip, A, mdl, [(W, 0), (W, 2048), (W, 0)], st)
    per_layer = [st[0][0], st[1][0] - st[0][0], st[2][0] - st[1][0]]
    print("items per layer (the second: a dropped attempt and its redo):", per_layer, "layers redone:", [x[1] for x in st])
    assert [x[1] for x in st] == [0, 1, 1]                      # the second layer was redone, and only that one
    # layer by layer: the marked layer -- two attempts -- counts what ONE attempt of its neighbours counts (same previous row)
    assert per_layer[0] > 0 and per_layer[1] == per_layer[0] and per_layer[2] == per_layer[0]
    assert hip.set_option("stat_reset", 1) == 0 and hip.get_stat("fix_items") == 0
    want = run(hip, A, mdl, [(W, 0), (W, 0), (W, 0)])
    assert hip.get_stat("spec_redo") == 0 and hip.get_stat("fix_items") == st[2][0]
    same(got, want)
