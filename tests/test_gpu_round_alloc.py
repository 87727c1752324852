"""The shortened round chain of the total-cost DP layer (csrc/dp_total.hip, csrc/dp_total_rpass.hip), each part against the launches
it replaces:

  * "round_alloc": k_setup_short reserves a list's slots and its offsets with one 64-bit atomic per block and its last block gives
    the round's verdict (cp_test_list_alloc drives the same device helpers) -- against k_round_scans (cp_test_round_scans);
  * "cr_consume": set-up zeroes the right-pass counters it reads, the clearing launch runs only while the planes may be dirty.

Layer parity (check_layer of tests/test_gpu_blocks.py: every layer against the brute-force tables) with each option on and off
and all of them off, under the driver options, on a row tile and in windowed layers; whole partitions against the oracle.

Off-diagonal guard as in tests/test_gpu_own_split.py: the winners off the diagonal must exceed 10 000 over the three mid-size
matrices (6 525 columns in all), each case its share in proportion to its n."""
import numpy as np
import pytest
import torch

from test_gpu_blocks import check_layer, Tables, w_rows
from test_gpu_own_split import tables, MATS, MID, MID_COLUMNS, MODELS, NET, WORK
from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

LT = 256                 # csrc/dp_total.hpp: steps per tile
FIX_SERIAL = 16          # ... tasks of more tiles than this are merged by blocks, one item per trip of
TRIP = 2048              # ... this many tiles
PARTS = ["round_alloc", "cr_consume"]
DEFAULTS = {"round_alloc": 1, "cr_consume": 1, "own_blk": 1, "own_pair": 1, "gap_tau": 6, "gap_min": 64, "nospec": 0,
            "own_min": 64, "poison": 0, "block_tables": 0, "rpass_ch": 256, "dbg": 0}
KEYS = ("T", "NT", "nlong", "nown", "ntile", "err")


def restore(hip):
    for k, v in DEFAULTS.items():
        hip.set_option(k, v)


def list_alloc(hip, a, b, bs=1024, cap_t=2**62, cap_nt=2**62, o_cap=None, err_in=0, reps=1, fit=(1, 1, 64)):
    """cp_test_list_alloc: (offs, slot_a, toffs, slot_b, ioffs, {T, NT, nlong, nown, ntile, err, items, ticket, words, fits})"""
    a = np.ascontiguousarray(a, dtype=np.int32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    offs, toffs = np.zeros(len(a) + 1, np.int64), np.zeros(len(b) + 1, np.int64)
    sa, sb, io = np.zeros(len(a) + 1, np.int32), np.zeros(len(b) + 1, np.int32), np.zeros(len(b) + 1, np.int32)
    res = np.zeros(10, np.int64)
    rc = hip.lib.cp_test_list_alloc(a, len(a), b, len(b), bs, cap_t, cap_nt, len(b) if o_cap is None else o_cap, err_in, reps, fit[0], fit[1], fit[2],
                                    offs, sa, toffs, sb, io, res)
    assert rc == 0, hip.last_error() if hasattr(hip, "last_error") else rc
    return offs, sa[:len(a)], toffs, sb[:len(b)], io[:len(b)], dict(zip(KEYS + ("items", "ticket", "words", "fits"), (int(v) for v in res)))


def items_of(ntl):
    return np.where(ntl > FIX_SERIAL, -(-ntl // TRIP), 0)


def check_structure(lens, offs, slots):
    """the slots are a permutation; offs[0] = 0; offs[s + 1] - offs[s] is the length placed in slot s; the closing entry is the total"""
    n = len(lens)
    assert np.array_equal(np.sort(slots), np.arange(n))
    placed = np.zeros(n, np.int64)
    placed[slots] = lens
    assert offs[0] == 0 and np.array_equal(np.diff(offs), placed)
    assert offs[n] == int(np.sum(lens, dtype=np.int64))


COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000]
TILES = np.array([1, 16, 17, 2048, 2049, 4097])


@pytest.mark.parametrize("bs", [1024, 256, 64])
@pytest.mark.parametrize("na", COUNTS)
def test_allocation_against_the_scans(hip, na, bs):
    """every count of the first list with every count of the second: the totals and the verdict of the scans' launch, the structure
    of the offsets, disjoint item ranges of the right sizes; three launches on one record leave the ticket and the words zero"""
    for nb in COUNTS:
        rng = np.random.default_rng(1000 * na + nb + bs)
        a = rng.integers(1, 64, na).astype(np.int32)
        b = TILES[rng.integers(0, len(TILES), nb)].astype(np.int32)
        offs, sa, toffs, sb, io, res = list_alloc(hip, a, b, bs=bs, reps=3)
        _, _, want = hip.test_round_scans(a, na + 1, b, nb + 1)
        assert {k: res[k] for k in KEYS} == want
        assert res["ticket"] == 0 and res["words"] == 0
        check_structure(a, offs, sa)
        check_structure(b, toffs, sb)
        it = items_of(b.astype(np.int64))
        assert res["items"] == int(it.sum())
        has = np.flatnonzero(it > 0)
        base = io[sb[has]]                                      # (by slot) the first item of every task that lists any
        order = np.argsort(base, kind="stable")
        assert np.array_equal(base[order], np.concatenate([[0], np.cumsum(it[has][order])[:-1]]) if len(has) else base[order])


@pytest.mark.parametrize("na,nb", [(1025, 65), (65, 1025), (5000, 5000), (5, 0), (0, 5)])
def test_the_verdict_drops_the_round(hip, na, nb):
    """a total beyond its capacity, a list longer than its slots, or a flag set earlier in the round: all four counts read 0 with
    err set, and no merge item is listed -- as after k_round_scans"""
    rng = np.random.default_rng(na + 3 * nb)
    a = rng.integers(1, 64, na).astype(np.int32)
    b = TILES[rng.integers(0, len(TILES), nb)].astype(np.int32)
    T, NT = int(a.sum(dtype=np.int64)), int(b.sum(dtype=np.int64))
    dropped = {"T": 0, "NT": 0, "nlong": 0, "nown": 0, "ntile": 0, "err": 1}
    kept = {"T": T, "NT": NT, "nlong": na, "nown": nb, "ntile": -(-T // LT), "err": 0}

    def verdict(**kw):
        res = list_alloc(hip, a, b, reps=2, **kw)[5]
        assert res["ticket"] == 0 and res["words"] == 0
        if res["err"]:
            assert res["items"] == 0
        return {k: res[k] for k in KEYS}

    assert verdict(cap_t=T, cap_nt=NT) == kept == hip.test_round_scans(a, na + 1, b, nb + 1, cap_t=T, cap_nt=NT)[2]
    if na:
        assert verdict(cap_t=T - 1, cap_nt=NT) == dropped
    if nb:
        assert verdict(cap_t=T, cap_nt=NT - 1) == dropped
        assert verdict(o_cap=nb - 1) == dropped
    assert verdict(err_in=1) == dropped


def test_the_host_bound_at_its_edges(hip):
    """round_alloc_fits(ntask, n, own_min): fewer than 2^24 tasks, both products below 2^40, own_min at most 2^24"""
    def fits(ntask, n, own_min):
        return list_alloc(hip, [], [], fit=(ntask, n, own_min))[5]["fits"]

    assert fits(2**24 - 1, 1000, 64) == 1 and fits(2**24, 1000, 64) == 0
    assert fits(2**20, 1000, 2**20 - 1) == 1 and fits(2**20, 1000, 2**20) == 0                    # ntask x own_min just below / at 2^40
    assert fits(2**20, (2**20 - 3) * 256, 64) == 1 and fits(2**20, (2**20 - 2) * 256, 64) == 0    # ntask x (n / 256 + 2) likewise
    assert fits(1, 1000, 2**24) == 1 and fits(1, 1000, 2**24 + 1) == 0
    assert fits(0, 1000, 64) == 1 and fits(1, 1000, 0) == 0


# ---- layers: every part on and off
def variants():
    """all on; each part off; all off"""
    return [{}] + [{p: 0} for p in PARTS] + [{p: 0 for p in PARTS}]


def stats(hip):
    return {k: hip.get_stat(k) for k in ("round_alloc_rounds", "cr_consume_rounds", "cr_clear_launches")}


def all_variants(hip, A, T, mdl, rows, rows_off, opts=None, tile=None):
    """check_layer under every variant (the full set of rows with everything on, rows_off for the others); returns the winners off
    the diagonal with everything on and the statistics per variant"""
    try:
        for k, v in (opts or {}).items():
            assert hip.set_option(k, v) == 0
        moved, st = None, []
        for i, var in enumerate(variants()):
            for p in PARTS:
                assert hip.set_option(p, var.get(p, 1)) == 0
            assert hip.set_option("stat_reset", 1) == 0
            m = check_layer(hip, A, T, mdl, rows if i == 0 else rows_off, tile=tile)
            moved = m if i == 0 else moved
            st.append(stats(hip))
        return moved, st
    finally:
        restore(hip)


def check_stats(st, tile=False):
    on, no_alloc, no_consume, off = st
    assert on["round_alloc_rounds"] > 0 and no_alloc["round_alloc_rounds"] == 0 and off["round_alloc_rounds"] == 0
    assert no_consume["cr_consume_rounds"] == 0 and off["cr_consume_rounds"] == 0
    if tile:
        assert on["cr_consume_rounds"] == 0


@pytest.mark.parametrize("mi", range(len(MATS)))
@pytest.mark.parametrize("ki", range(len(MODELS)))
def test_layer_parity_on_and_off(hip, mi, ki):
    T = tables(mi)
    A, mdl = T.A, MODELS[ki][1]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    rng = np.random.default_rng(2100 + 10 * mi + ki)
    scale = int(abs(T.F(mdl, 2)).max()) + 1
    rows = w_rows(rng, A.n, scale, dt)
    # rpass_ch 16: the rounds tau >= 6 of these sizes add a row's right-pass counts chunk by chunk
    moved, st = all_variants(hip, A, T, mdl, rows, [rows[0], rows[5]], opts={"rpass_ch": 16})
    check_stats(st)
    if A.n >= 1024:
        # (the work object belongs to the matrix: an earlier case may have left the planes dirty -- then ONE layer clears as before)
        assert st[0]["cr_consume_rounds"] > 0 and st[0]["cr_clear_launches"] < st[2]["cr_clear_launches"]
    if mi < len(MID):
        assert moved * MID_COLUMNS > 10000 * A.n, (MATS[mi][0], MODELS[ki][0], moved)


OPTION_SETS = [{"own_blk": 0}, {"own_pair": 0}, {"gap_tau": -1}, {"gap_tau": 8, "gap_min": 8}, {"nospec": 1}, {"own_min": 1000}, {"poison": 1},
               {"dbg": 1024}, {"dbg": 2048}, {"dbg": 64}]


@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_layer_parity_under_driver_options(hip, oi):
    """(dbg 1024 / 2048: every layer after the first is redone; dbg 64: no own tiles -- the lists are scanned by k_round_scans)"""
    for mi, models in ((0, [NET]), (2, [NET, WORK])):
        T = tables(mi)
        A = T.A
        for k, mdl in enumerate(models):
            rng = np.random.default_rng(2200 + 10 * oi + 3 * mi + k)
            scale = int(abs(T.F(mdl, 2)).max()) + 1
            rows = w_rows(rng, A.n, scale, np.int64)
            moved, st = all_variants(hip, A, T, mdl, [rows[0], rows[2], rows[5]], [rows[0], rows[5]], opts=dict(OPTION_SETS[oi], rpass_ch=16))
            assert 2 * moved * MID_COLUMNS > 10000 * A.n       # (half the rows of a mid-size case: half its share)
            if OPTION_SETS[oi] == {"dbg": 64}:
                assert all(s["round_alloc_rounds"] == 0 for s in st)
            else:
                check_stats(st)


def test_row_tiles_with_injected_rows(hip):
    A = suitesparse_shaped(2000, 6, 5)
    T = Tables(A)
    n = A.n
    rng = np.random.default_rng(212)
    for mdl in (NET, WORK):
        scale = int(abs(T.F(mdl, 2)).max()) + 1
        for (lo, hi) in [(1, n // 3), (n // 3, n // 2 + 7), (n // 2 + 7, n + 2)]:
            rows = w_rows(rng, n, scale, np.int64)
            moved, st = all_variants(hip, A, T, mdl, [rows[0], rows[5]], [rows[5]], opts={"rpass_ch": 16}, tile=(max(1, lo), hi))
            check_stats(st, tile=(lo, hi) != (1, n + 2))


def layers(hip, A, mdl, steps):
    """steps: (W, dbg, rows or None) per layer on ONE handle; returns per layer (cst, ptr, clearing launches, rounds without one,
    layers redone)"""
    n = A.n
    dev = torch.device("cuda", 0)
    dp = hip.dp_begin(A, 3, 0, 0, mdl.marshal(), 1, n + 2)
    out = []
    try:
        for W, dbg, rows in steps:
            assert hip.set_option("dbg", dbg) == 0 and hip.set_option("stat_reset", 1) == 0
            if rows is not None:
                hip.dp_set_rows(dp, rows[0], rows[1])
            prev = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
            cur = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            hip.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
            out.append((cur.cpu().numpy(), hip.dp_ptr_row(dp, 2, n), hip.get_stat("cr_clear_launches"), hip.get_stat("cr_consume_rounds"),
                        hip.get_stat("spec_redo")))
    finally:
        hip.set_option("dbg", 0)
        hip.dp_destroy(dp)
    return out


@pytest.mark.parametrize("mdl", [NET, MODELS[4][1]], ids=["net", "hyp"])
def test_cr_consume_over_many_layers(hip, mdl):
    """four full layers on one handle, the third one redone (dbg 1024), then a row tile, then two full layers again: every layer
    equals the one computed with the clear in front of every chunked right pass, and the clear runs exactly where it has to -- in
    the row-tiled layer and in the first full layer after it (the tile's right passes add into rows next to it that nobody read)"""
    n = 20_011
    A = suitesparse_shaped(n, 5, 3)
    rng = np.random.default_rng(61)
    Ws = w_rows(rng, n, 1_000_000, np.int64)
    tile = (n // 3, n // 2 + 7)
    steps = [(Ws[0], 0, None), (Ws[5], 0, None), (Ws[1], 1024, None), (Ws[3], 0, None), (Ws[5], 0, tile), (Ws[0], 0, (1, n + 2)), (Ws[5], 0, None)]
    try:
        assert hip.set_option("rpass_ch", 16) == 0
        got = layers(hip, A, mdl, steps)
        assert got[2][4] > 0                                        # the third layer was redone
        for p in PARTS:
            assert hip.set_option(p, 0) == 0
        want = layers(hip, A, mdl, steps)
    finally:
        restore(hip)
    for i, (g, w) in enumerate(zip(got, want)):
        sl = slice(tile[0] - 1, tile[1] - 1) if i == 4 else slice(None)
        assert np.array_equal(g[0][sl], w[0][sl]) and np.array_equal(g[1][sl], w[1][sl]), i
        assert w[2] > 0 and w[3] == 0
    assert [g[2] > 0 for g in got] == [False, False, False, False, True, True, False]
    assert [g[3] > 0 for g in got] == [True, True, True, True, False, False, True]


WIN_OPTIONS = [{}, {"nospec": 1}, {"poison": 1}, {"own_min": 1000}, {"gap_tau": -1}, {"rpass_ch": 16}, {"dbg": 1024}, {"dbg": 2048}]


@pytest.mark.parametrize("oi", range(len(WIN_OPTIONS)))
def test_windowed_layers_on_and_off(hip, orc, oi):
    """windowed layers under every variant: the layer kernel on injected rows against brute force (min over max(0, r - w) <= p <= r),
    and the K layers of a width-constrained DP on one handle against the oracle's tables (dbg 1024 / 2048: layers redone)"""
    import brute
    A = suitesparse_shaped(1500, 6, 5)
    n = A.n
    F = brute.cost_table(A, NET, 2, brute.net_table(A), brute.selfnet_table(A))
    scale = int(abs(F).max()) + 1
    rng = np.random.default_rng(300 + oi)
    rows = [rng.integers(0, scale + 1, n + 1), np.where(rng.random(n + 1) < 0.02, 0, scale * 8).astype(np.int64)]
    want = {(w, i): brute.layer(W, F, lo=np.maximum(0, np.arange(n + 1) - w)) for w in (129, n // 2) for i, W in enumerate(rows)}
    B = suitesparse_shaped(3000, 8, 1)
    mm, K, wB = NET.marshal(), 7, B.n // 4
    _, _, _, p2, c2 = orc.dynamic_tables_constrained(B, K, 0, mm, None, cp.VertexCount().marshal(), wB, float(wB))
    try:
        for k, v in WIN_OPTIONS[oi].items():
            assert hip.set_option(k, v) == 0
        for var in variants():
            for p in PARTS:
                assert hip.set_option(p, var.get(p, 1)) == 0
            assert hip.set_option("stat_reset", 1) == 0
            for (w, i), (cb, pb) in want.items():
                cst, ptr = hip.windowed_layer(A, mm, rows[i].astype(np.int64), w)
                assert np.array_equal(ptr, pb) and np.array_equal(cst, cb), (var, w, i)
            rc1, _, _, p1, c1 = hip.dynamic_tables_constrained(B, K, mm, wB)
            assert rc1 == 0 and np.array_equal(p1, p2) and np.array_equal(c1, c2), var
            assert (hip.get_stat("round_alloc_rounds") > 0) == (var.get("round_alloc", 1) == 1)
    finally:
        restore(hip)


def test_fix_items_count_the_same_with_a_skipped_stage(hip):
    """a mispredicted attempt (dbg 1024: the own-tile stage of every odd round skipped on the host, the layer redone) reserves its
    items in set-up but lists none: cp_get_stat("fix_items") is what it is with round_alloc 0"""
    n = 70_001
    A = suitesparse_shaped(n, 5, 3)
    W = w_rows(np.random.default_rng(93), n, 1_000_000, np.int64)[5]
    dev = torch.device("cuda", 0)
    counts = []
    try:
        for on in (1, 0):
            assert hip.set_option("round_alloc", on) == 0 and hip.set_option("stat_reset", 1) == 0
            dp = hip.dp_begin(A, 3, 0, 0, NET.marshal(), 1, n + 2)
            try:
                for dbg in (0, 1024, 0):
                    assert hip.set_option("dbg", dbg) == 0
                    prev = torch.from_numpy(W).to(dev)
                    cur = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                    hip.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
            finally:
                hip.set_option("dbg", 0)
                hip.dp_destroy(dp)
            counts.append((hip.get_stat("fix_items"), hip.get_stat("spec_redo")))
    finally:
        restore(hip)
    assert counts[0] == counts[1] and counts[0][0] > 0 and counts[0][1] > 0


def test_whole_partitions_and_windowed_layers(hip, orc):
    """n = 3000, K = 8: equal split vectors with the parts on and off, equal to the oracle's -- for the four models and for a
    width-constrained cost (windowed layers: they keep the clear)"""
    A = suitesparse_shaped(3000, 8, 1)
    n, K = A.n, 8
    costs = [m for name, m in MODELS if name in ("net", "work", "conn_f64", "hyp")] + [cp.ConstrainedCost(NET, cp.VertexCount(), -(-3 * n // (2 * K)))]
    try:
        for f in costs:
            want = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=orc)
            for var in variants():
                for p in PARTS:
                    assert hip.set_option(p, var.get(p, 1)) == 0
                assert hip.set_option("stat_reset", 1) == 0
                got = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(f), backend=hip)
                assert np.array_equal(got.spl, want.spl), (f, var)
                st = stats(hip)
                assert (st["round_alloc_rounds"] > 0) == (var.get("round_alloc", 1) == 1)
                if not isinstance(f, cp.ConstrainedCost):
                    assert (st["cr_consume_rounds"] > 0) == (var.get("cr_consume", 1) == 1)
    finally:
        restore(hip)
