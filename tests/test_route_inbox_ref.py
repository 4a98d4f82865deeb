"""tests/route_inbox_ref.py held to account on the CPU, so that the GPU tests (tests/test_route_inbox_kernels_gpu.py) compare the kernels with
something that has itself been checked:
  * its definitions are oracle/ref_np.py's route_ids / gather_inbox on random and on the listed cases;
  * its models of the kernels' order (chunk histogram -> stepped scan -> cell prefix -> ballot rank; prefix search; classic tiles; the ring's
    persistent walk) equal the definitions on every listed case;
  * its restated workspace arithmetic is the library's, where the library loads;
  * the case lists reach every edge they were computed for, by name;
  * one planted mistake per model leaves the definition on a listed case -- among them the ring's resolve loop with the trip count
    NS * TB // 256 it had before, which resolves nothing exactly at tb = 4 (rows of 132..256 floats)."""
import functools

import numpy as np
import pytest

from oracle import ref_np as R
from tests import route_inbox_ref as P

ROUTE_NAMES = sorted(P.route_cases())


@functools.lru_cache(maxsize=None)
def _route(name):
    ids, world, cap, view = P.route_case(name)
    return ids, world, cap, P.route_def(ids, world, cap, -1)


# ------------------------------------------------------------------------------------------------- definitions against the oracle
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_route_definition_is_the_oracles(name):
    ids, world, cap, d = _route(name)
    send, slot, counts2d, worst = R.route_ids(ids, world, cap)
    assert np.array_equal(d.send_rows, send) and np.array_equal(d.slot, slot) and np.array_equal(d.counts2d, counts2d) and d.worst == worst
    live = d.slot >= 0                                                   # positions: the id's place inside its feature, where it was sent
    within = np.concatenate([np.arange(a.size) for a in ids])
    assert np.array_equal(d.send_pos[d.slot[live]], within[live])
    assert (d.send_pos[np.setdiff1d(np.arange(world * cap), d.slot[live])] == -1).all()


def test_route_definition_is_the_oracles_on_random_exchanges():
    rng = np.random.default_rng(5)
    for _ in range(60):
        world, F = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        ids = [rng.integers(-3, 1 << 33 if rng.random() < 0.3 else 50, int(rng.integers(0, 300))) for _ in range(F)]
        cap = int(rng.integers(1, 200))
        d = P.route_def(ids, world, cap, -1)
        send, slot, counts2d, worst = R.route_ids(ids, world, cap)
        assert np.array_equal(d.send_rows, send) and np.array_equal(d.slot, slot) and np.array_equal(d.counts2d, counts2d) and d.worst == worst
        assert P.same_route(P.route_model(ids, world, cap, -1), d)


def test_bad_ids_go_to_rank_0_and_int32_max_is_a_row():
    ids = [np.array([-1, -(1 << 63), 1 << 31, P.I32MAX, 1 << 40, 7], np.int64)]
    d = P.route_def(ids, 5, 8, -9)
    assert d.send_rows[:3].tolist() == [-1, -1, P.I32MAX] and d.send_rows[3] == P.I32MAX and d.counts2d[:, 0].tolist() == [4, 0, 2, 0, 0]
    assert d.send_rows[2 * 8:2 * 8 + 2].tolist() == [P.I32MAX // 5, 1] and P.I32MAX % 5 == 2      # 2^31 - 1 is a row of rank 2, like 7
    assert (np.delete(d.send_rows, [0, 1, 2, 3, 16, 17]) == -9).all()                             # the other slots are left alone


@pytest.mark.parametrize("dim", [1, 5, 16, 300])
def test_gather_definition_is_the_oracles(dim):
    rng = np.random.default_rng(dim)
    tables = [rng.standard_normal((r, dim)).astype(np.float32) for r in P.TABLE_ROWS]
    for name in P.classic_cases(dim):
        ib = P.classic_case(dim, name, bad=False)
        want = R.gather_inbox(tables, ib.feat_table, ib.world, ib.cap, ib.recv2d, ib.rows, dim)
        assert np.array_equal(P.gather_def(ib, tables, dim, fill=0.0), want), name
        g = P.gather_index(ib)
        assert not g.bad.any() and not g.reports
        grads, _ = P.scatter_def(ib, np.ones((ib.world * ib.cap, dim)), [np.zeros((r, dim)) for r in P.TABLE_ROWS], 0)
        for t in range(2):                                               # scatter-add of ones = how often a row is named
            assert np.array_equal(grads[t][:, 0], np.bincount(g.row[g.tab == t], minlength=P.TABLE_ROWS[t])), name


def test_out_of_range_rows_read_row_0_are_counted_and_are_dropped_by_the_scatter():
    ib = P.classic_case(16, "w3-f3")
    g = P.gather_index(ib)
    raw = ib.rows[g.flat]
    assert g.bad.sum() >= 6 and {-1, P.I32MAX} <= set(raw[g.bad].tolist()) and (g.row[g.bad] == 0).all() and len(g.reports) == g.bad.sum()
    assert (raw[g.bad & (raw > 0)] >= np.asarray(ib.table_rows)[g.tab[g.bad & (raw > 0)]]).all()
    ones = np.ones((ib.world * ib.cap, 1))
    for skip in (0, 1):
        grads, mag = P.scatter_def(ib, ones, [np.zeros((r, 1)) for r in P.TABLE_ROWS], skip)
        keep = ~g.bad & ~((g.row == 0) & bool(skip))
        assert sum(int(t.sum()) for t in grads) == keep.sum() and all(np.array_equal(a, b) for a, b in zip(grads, mag))
        assert (grads[0][0, 0] == 0) == bool(skip)
    pl = P.place_index(P.place_case(16, "w3"))
    assert pl.dropped.sum() >= 3 and pl.n_reports == pl.bad.sum() + pl.dropped.sum() and {-1, P.I32MAX} <= set(pl.at[pl.dropped].tolist())


# ------------------------------------------------------------------------------------------------- the kernels' order against the definitions
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_route_model_equals_the_definition(name):
    ids, world, cap, d = _route(name)
    assert P.same_route(P.route_model(ids, world, cap, -1), d)


def _same_features(model, ib):
    flat, feat = P.slot_features(ib)
    return np.array_equal(model[0], flat) and np.array_equal(model[1], feat)


@pytest.mark.parametrize("dim", P.CLASSIC_DIMS)
def test_classic_model_equals_the_definition(dim):
    for name in P.classic_cases(dim):
        assert _same_features(P.classic_model(P.classic_case(dim, name), dim), P.classic_case(dim, name)), name


@pytest.mark.parametrize("dim", P.RING_DIMS)
def test_ring_model_equals_the_definition(dim):
    ib = P.ring_case(dim)
    flat, feat, facts = P.ring_model(ib, dim)
    assert _same_features((flat, feat), ib) and facts.unresolved == 0 and facts.grid == facts.nwork == P.RING_MIN_ITEMS
    assert _same_features(P.classic_model(P.ring_case(dim, 63), dim), P.ring_case(dim, 63))
    if dim in P.PLACE_DIMS:
        for name in P.place_cases(dim):
            ib = P.place_case(dim, name)
            flat, feat, facts = P.ring_model(ib, dim, place=True)
            assert _same_features((flat, feat), ib) and facts.unresolved == 0, name


@pytest.mark.parametrize("dim", P.WRAP_DIMS)
def test_ring_model_equals_the_definition_past_the_wrap(dim):
    ib = P.wrap_case(dim)
    for place in (False, True):
        flat, feat, facts = P.ring_model(ib, dim, place=place)
        assert _same_features((flat, feat), ib) and facts.unresolved == 0
        assert facts.nwork == 1600 and facts.grid == P.RING_GRID
        assert facts.skipped > 1000 and facts.switches_live >= 1 and facts.past_wrap_live >= 4


def test_workspace_arithmetic_is_the_librarys():
    from news_recsys_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    sizes = [0, 1, 2047, 2048, 2049, 256 * 2048 + 1, 512 * 2048 + 1, P.I32MAX] + rng.integers(0, 1 << 31, 200).tolist()
    for n in sizes:
        for world in (1, 2, 5, 63, 64):
            assert lib.nrx_route_workspace(n, world) == P.route_workspace(n, world), (n, world)
    assert lib.nrx_route_workspace(-1, 2) == -1 == P.route_workspace(-1, 2) and lib.nrx_route_workspace(5, 0) == -1 == P.route_workspace(5, 0)
    for name in ROUTE_NAMES:                                             # the histogram [world][nchunks] of every listed case fits
        ids, world, cap, _ = P.route_case(name)
        lens = [a.size for a in ids]
        assert P.nchunks(lens) * world * 4 <= P.route_workspace(sum(lens), world) * 8, name


# ------------------------------------------------------------------------------------------------- the lists reach what they were computed for
def test_route_cases_reach_every_edge():
    cases = P.route_cases()
    lens = {n: c["lens"] for n, c in cases.items()}
    assert {c["world"] for c in cases.values()} >= {1, 2, 5, 64}
    assert {P.scan_steps(l) for l in lens.values()} >= {1, 2, 3}
    assert P.scan_steps(lens["w2-scan2"]) == 2 and P.nchunks(lens["w2-scan2"]) == P.SCAN_STEP + 1          # the smallest second step
    assert {cases[n]["world"] for n in lens if P.scan_steps(lens[n]) == 3} >= {2, 5}
    assert P.chunk0(lens["w5-scan3"])[1] == 1                            # the long feature's chunks do not start a step
    assert any(P.scan_trips(c["world"]) > 1 for c in cases.values()) and P.scan_trips(64) == 16 and P.scan_trips(2) == 1
    for n in ("w1-edges", "w2-edges", "w5-edges"):
        l = lens[n]
        assert set(l) == set(P.FEATURE_LENS) and l[0] == l[1] == 0 and l[-1] == l[-2] == 0 and 0 in l[2:-2]
    assert len(lens["w5-f64"]) == P.MAX_FEATURES and set(lens["w5-f64"]) == set(P.FEATURE_LENS)
    assert {c["bits"] for c in cases.values()} == {32, 64} and {c["bits"] for c in cases.values() if c.get("view")} == {32, 64}
    ids, world, cap, d = _route("w5-over1")
    per_owner = d.counts2d.sum(1)
    assert d.worst == cap + 1 and (per_owner > cap).sum() == 1 and (d.slot == -1).sum() == 1
    ids, world, cap, d = _route("w5-skew")
    assert (d.counts2d.sum(1) > 0).tolist() == [False, False, False, True, False] and d.worst > cap and (d.slot == -1).sum() == d.worst - cap
    ids, world, cap, d = _route("w1-over")
    assert d.worst == sum(lens["w1-over"]) > cap
    for n in ("w1-edges", "w5-edges", "w64-edges"):
        flat = np.concatenate(_route(n)[0]).astype(np.int64)
        assert set(P.BAD_IDS_64) <= set(flat.tolist()), n
    assert set(P.BAD_IDS_32) <= set(np.concatenate(_route("w2-edges")[0]).tolist())
    for n in ROUTE_NAMES:                                                # every block keeps slots past its count: "left untouched" is checked
        ids, world, cap, d = _route(n)
        assert (np.minimum(d.counts2d.sum(1), cap) < cap).any() or n == "w1-over", n
    for must in ("world 0", "world 65", "cap 0", "cap * world = 2^31", "n_feats 0", "n_feats 65"):
        assert must in P.ROUTE_REFUSALS


def test_inbox_cases_reach_every_edge():
    assert set(P.CLASSIC_DIMS) == {1, 3, 4, 5, 8, 12, 16, 17, 32, 64, 100, 256, 260, 300} | {101, 257}
    assert {P.ql(d) for d in P.CLASSIC_DIMS} == set(range(7))
    assert [P.k0_trips(d) for d in (256, 257, 260, 300)] == [1, 2, 2, 2] and {d % 4 != 0 for d in P.CLASSIC_DIMS} == {True, False}
    assert {P.ql(d) for d in P.CLASSIC_DIMS if d % 4} >= {0, 1, 3, 5, 6}                                   # the scalar path / the scatter's tails
    for dim in P.CLASSIC_DIMS:
        T, cases = P.classic_tile(dim), P.classic_cases(dim)
        assert T == 8 * (256 >> P.ql(dim)) and {w for w, *_ in cases.values()} == {1, 3, 64}
        for name, (world, cap, counts, feat_table) in cases.items():
            assert P.form(dim, cap, world) == "classic" and P.form(dim, cap, world, scatter=True) == "classic", (dim, name)
            assert cap % T and cap % 256 and P.classic_grid(dim, cap, world) == (4, world)
        sums = np.asarray(cases["w64-f64"][2]).sum(1).tolist()
        assert set(sums) == set(P.count_menu(T, cases["w64-f64"][1])) and max(sums) > cases["w64-f64"][1]
        c64 = np.asarray(cases["w64-f64"][2])
        assert c64.shape == (64, 64) and not c64[:, [0, 1, 2, 19, 62]].any() and c64[:, [3, 17, 18, 40, 63]].any(0).all()
        w3 = np.asarray(cases["w3-f3"][2])
        assert w3[1].sum() == 0 and w3[2].sum() > cases["w3-f3"][1] and sorted(set(cases["w3-f3"][3])) == [0, 1] and len(cases["w3-f3"][3]) == 3
        pre = np.cumsum(w3[0])[:-1]                                      # a feature boundary off the tile edge: some thread's 8 strided slots straddle it
        assert (pre % T != 0).any() and (pre < 3 * T + 5).all(), dim
        assert cases["w1-f1"][2] == [[T + 1]]
    assert P.RING_DIMS == [12, 16, 20, 32, 36, 64, 68, 128, 132, 256] and sorted({P.ql(d) for d in P.RING_DIMS}) == [2, 3, 4, 5, 6]
    for q in range(2, 7):
        assert {d == 4 << q for d in P.RING_DIMS if P.ql(d) == q} == {True, False}, q                   # every lane busy / idle lanes
    for dim in P.RING_DIMS:
        ib, I = P.ring_case(dim), P.ring_item(dim)
        assert I == 32 * P.tb(dim) and ib.cap == 7 * I + 1 and P.cps(dim, ib.cap) == 8
        assert P.form(dim, ib.cap, 64) == "ring" and P.form(dim, ib.cap, 63) == "classic" and P.cps(dim, ib.cap) * 64 == P.RING_MIN_ITEMS
        assert {0, 1, I - 1, I, I + 1, ib.cap} <= set(P.totals(ib).tolist()) and (ib.recv2d.sum(1) > ib.cap).any()
    for dim in P.WRAP_DIMS:
        ib, I = P.wrap_case(dim), P.ring_item(dim)
        assert P.cps(dim, ib.cap) == P.WRAP_CPS and P.form(dim, ib.cap, 64) == "ring" and 64 * P.WRAP_CPS == 1600 > P.ring_grid(dim, ib.cap, 64) == 1536
        assert np.flatnonzero(ib.recv2d.sum(1)).tolist() == P.WRAP_LIVE and {I - 1 + 2, I, 3 * I + 5} <= set(P.totals(ib).tolist())
    assert sorted({P.ql(d) for d in P.PLACE_DIMS}) == [2, 3, 4, 5, 6] and all(d in P.RING_DIMS and d >= 16 for d in P.PLACE_DIMS)
    for dim in P.PLACE_DIMS:
        items = []
        for name in P.place_cases(dim):
            ib = P.place_case(dim, name)
            assert P.place_shape_ok(dim, ib.out_ld, ib.feat_col) and ib.out_ld > 3 * dim and ib.feat_col != sorted(ib.feat_col)
            items.append(P.cps(dim, ib.cap) * ib.world)
            g = P.place_index(ib)
            assert {-1, ib.out_rows, P.I32MAX} <= set(g.at[g.dropped].tolist()) or g.flat.size < 100, (dim, name)
        assert items == [1, 2, 6]
    assert not P.place_shape_ok(8, 32, [0]) and not P.place_shape_ok(18, 32, [0]) and not P.place_shape_ok(260, 300, [0])
    assert not P.place_shape_ok(16, 34, [0]) and not P.place_shape_ok(16, 32, [2]) and not P.place_shape_ok(16, 32, [20])
    for must in ("world 0", "world 65", "cap 0", "n_feats 0", "n_feats 65", "feat_table out of range", "null table", "misaligned table"):
        assert must in P.INBOX_REFUSALS
    for must in ("dim 8", "dim 18", "dim 260", "out_ld % 4", "feat_col % 4", "feat_col + dim > out_ld", "misaligned peer_out"):
        assert must in P.PLACE_REFUSALS


# ------------------------------------------------------------------------------------------------- planted mistakes are caught by a listed case
def _route_mutant_caught(carry):
    return [n for n in ROUTE_NAMES if not P.same_route(P.route_model(*_route(n)[:3], -1, carry=carry), _route(n)[3])]


def test_a_scan_without_its_carry_is_caught_from_the_second_step_on():
    assert _route_mutant_caught("none") == sorted(n for n in ROUTE_NAMES if "scan" in n)


def test_a_carry_one_chunk_short_is_caught_from_the_second_step_on():
    assert _route_mutant_caught("short") == sorted(n for n in ROUTE_NAMES if "scan" in n)


def _classic_caught(**kw):
    return {(d, n) for d in P.CLASSIC_DIMS for n in P.classic_cases(d) if not _same_features(P.classic_model(P.classic_case(d, n), d, **kw), P.classic_case(d, n))}


def test_a_strict_prefix_search_is_caught():
    caught = _classic_caught(strict=True)
    assert {d for d, _ in caught} == set(P.CLASSIC_DIMS) and all((d, "w3-f3") in caught for d in P.CLASSIC_DIMS)
    ib = P.ring_case(16)
    assert not _same_features(P.ring_model(ib, 16, strict=True)[:2], ib)


def test_a_missing_clamp_to_cap_is_caught():
    caught = _classic_caught(clamp=False)
    assert all((d, "w3-f3") in caught and (d, "w64-f64") in caught and (d, "w1-f1") not in caught for d in P.CLASSIC_DIMS)


def test_a_grid_that_misses_the_partial_tile_is_caught():
    caught = _classic_caught(floor_grid=True)
    assert all((d, "w3-f3") in caught and (d, "w64-f64") in caught for d in P.CLASSIC_DIMS)


def test_a_source_switch_that_keeps_the_old_prefix_is_caught_by_the_wrap_cases():
    for dim in P.WRAP_DIMS:
        ib = P.wrap_case(dim)
        assert not _same_features(P.ring_model(ib, dim, rebuild=False)[:2], ib)
    ib = P.ring_case(16)                                                 # (512 items on 512 blocks: no block meets a second source)
    assert _same_features(P.ring_model(ib, 16, rebuild=False)[:2], ib)


def test_the_parents_resolve_trip_count_leaves_slots_unresolved_exactly_at_tb_4():
    for dim in P.RING_DIMS:
        ib = P.ring_case(dim)
        flat, feat, facts = P.ring_model(ib, dim, parent_trips=True)
        ref_flat, _ = P.slot_features(ib)
        assert np.array_equal(flat, ref_flat)                            # the walk still visits every live slot ...
        if P.tb(dim) == 4:                                               # ... but 128 // 256 = 0 trips resolved none of them
            assert dim in (132, 256) and P.resolve_trips(dim, parent=True) == 0 and facts.unresolved == flat.size > 0
            assert (feat == P.UNRESOLVED).all()
        else:
            assert P.resolve_trips(dim, parent=True) == P.resolve_trips(dim) == P.ring_item(dim) and facts.unresolved == 0
            assert _same_features((flat, feat), ib)
    for dim in P.PLACE_DIMS:
        if P.tb(dim) == 4:
            ib = P.place_case(dim, "w3")
            assert P.ring_model(ib, dim, place=True, parent_trips=True)[2].unresolved == P.slot_features(ib)[0].size
    assert [P.resolve_trips(d) for d in (16, 32, 64, 128, 132, 256)] == [2048, 1024, 512, 256, 128, 128]
