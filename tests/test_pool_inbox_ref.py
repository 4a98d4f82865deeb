"""tests/pool_inbox_ref.py held to account on the CPU, so that the GPU tests (tests/test_pool_inbox_kernels_gpu.py) compare the kernels with
something that has itself been checked:
  * its float32 forward is oracle/ref_np.py's pool_inbox bit for bit on every in-contract inbox, and lies inside gamma(n) sum |w row| of its
    float64 forward on every inbox;
  * owner partials summed over the owners reproduce array_feature_pooling on a routed batch, and its run bounds are route_bags_runs';
  * the expansion's definition scattered by its owner ids is the dense backward's definition; the norm weights are the oracle's;
  * the case lists reach every lane-group width, pass count, exchange width, run-length class and inbox edge they claim, by name;
  * two structural mistakes of the forward (run bounds swapped; the entries past a run's end keeping their weight) leave the bound."""
import numpy as np
import pytest

from oracle import ref_np as R
from tests import pool_inbox_ref as P

F32 = np.float32
CASES = [(d, key) for d in P.DIMS for key, *_ in P.inbox_cases(d)]
CASE_IDS = [f"D{d}-{key}" for d, key in CASES]


def _ratio(got, ref, bound):
    """Largest |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------- the case lists say what they claim
def test_dims_and_run_lengths_are_the_lists_asked_for():
    assert P.DIMS == [1, 3, 4, 5, 8, 12, 16, 17, 24, 32, 33, 64, 100, 128, 129, 256, 257, 300, 512, 1024]
    assert P.RUN_MENU == [0, 1, 2, 15, 16, 17, 31, 32, 33, 50]
    assert P.NORM_LS == [1, 15, 16, 17, 50, 64, 65, 128, 130]
    assert [P.norm_pb(L) for L in (64, 65)] == [16, 4]


def test_case_lists_reach_every_instantiation_and_edge():
    assert {P.qlog2(d) for d in P.DIMS} == set(range(7)), "QLOG2 0..6"
    assert {P.passes(d) for d in P.DIMS} >= {1, 2, 4}, "1, 2 and 4 passes"
    assert [P.passes(d) for d in (256, 257, 300, 512, 1024)] == [1, 2, 2, 2, 4]
    assert {P.epl(d) for d in P.DIMS if P.lanes(d) > 1} == {8, 4, 2, 1}, "EPL 8, 4, 2, 1"
    assert any(P.lanes(d) == 1 for d in P.DIMS), "the Q == 1 load path"
    assert {P.lanes_beyond_ahead(d) for d in P.DIMS} >= {0, 16, 48}, "lanes beyond AHEAD at Q = 32 and 64"
    for ql in range(7):                                                  # each width with dim == 4 Q and with dim != 4 Q (Q = 1: dim 1, 3)
        assert {P.expand_vector_path(d) for d in P.DIMS if P.qlog2(d) == ql} == {True, False}, ql
    assert [d for d in P.DIMS if P.expand_vector_path(d)] == [4, 8, 16, 32, 64, 128, 256]
    assert any(d % 4 for d in P.DIMS) and all(P.qlog2(d) in {P.qlog2(x) for x in P.DIMS if x % 4} for d in (5, 17, 33))
    assert set(P.BF16_DIMS) <= set(P.DIMS) and {d % 4 == 0 for d in P.BF16_DIMS} == {True, False}
    for d in P.DIMS:
        t = P.tb(d)
        ntags = sorted(nf * b for _, _, nf, b, _ in P.inbox_cases(d))
        assert ntags == sorted([1, t - 1, t, t + 1, 3 * t + 5, 3 * (t + 2)]), d
        assert {w for _, w, *_ in P.inbox_cases(d)} == {1, 2, 3}, d
        assert {nf for _, _, nf, _, _ in P.inbox_cases(d)} == {1, 3}, d


@pytest.mark.parametrize("dim", P.DIMS)
def test_every_dim_meets_every_inbox_edge(dim):
    t = P.tb(dim)
    seen = set()
    for key, world, n_feats, batch, _ in P.inbox_cases(dim):
        ib = P.case_inbox(dim, key)
        facts = P.inbox_facts(ib)
        assert ib.cap % t != 0 and ib.cap % 256 != 0, key
        assert P.feat_table_of(n_feats) != list(range(n_feats))
        if ib.ntag >= len(P.RUN_MENU):
            seen |= facts["run classes"]
        if key == "main":
            assert ib.recv2d[1].sum() == 0 and ib.recv2d[2].sum() > ib.cap and 0 < ib.recv2d[0].sum() <= ib.cap
            for name in ("empty block", "clipped block", "row out of range with weight", "row out of range without weight", "tag out of range",
                         "run of rows out of range only"):
                assert facts[name], (name, dim)
            assert facts["hot row hits"] >= 200, facts["hot row hits"]
            assert len(set(ib.table_rows)) == 2 and set(ib.feat_table) == {0, 1}
            lens = (ib.run[0, :, 1] - ib.run[0, :, 0]).tolist()
            assert set(lens) >= set(P.RUN_MENU) - {0} and 0 in lens, "every run length in the block that fits"
            e = P.entries(ib)
            bad = np.flatnonzero(e.counted & ~e.tag_ok)                  # a bad tag never sits inside a run
            for i in bad:
                left = ib.tag[i - 1] if e.j[i] > 0 else None
                right = ib.tag[i + 1] if e.j[i] + 1 < ib.total[e.s[i]] else None
                assert left is None or right is None or left != right, i
        else:
            assert not facts["tag out of range"] and not facts["row out of range with weight"]
        # the layout itself: tags of the counted entries that are in range never decrease
        e = P.entries(ib)
        for s in range(ib.world):
            tg = ib.tag[s * ib.cap:s * ib.cap + ib.total[s]][e.tag_ok[s * ib.cap:s * ib.cap + ib.total[s]]]
            assert np.all(np.diff(tg) >= 0)
        past = ~e.counted
        assert np.all(ib.rows[past] == P.GARBAGE_ROW) and np.all(ib.tag[past] == P.GARBAGE_TAG) and np.isnan(ib.w[past]).all()
    assert seen >= set(P.RUN_CLASSES), (dim, seen)


# ------------------------------------------------------------------------------------------------- forward
def _in_contract(dim, key):
    for i, (k, world, n_feats, batch, opt) in enumerate(P.inbox_cases(dim)):
        if k == key:
            opt = {x: v for x, v in opt.items() if x not in ("oob",)}
            return P.build_inbox(i, world, n_feats, batch, 5, dim, P.TABLE_ROWS, P.feat_table_of(n_feats), P.RUN_MENU, **opt)


@pytest.mark.parametrize("dim", P.DIMS)
def test_fp32_forward_is_the_oracles_pool_inbox_bit_for_bit(dim):
    tables = P.case_tables(dim)
    for key, *_ in P.inbox_cases(dim):
        ib = _in_contract(dim, key)
        want = R.pool_inbox(list(tables), ib.feat_table, ib.batch, ib.world, ib.cap, ib.recv2d, ib.rows, ib.tag, ib.w, dim)
        assert P.same_bits(P.pool_fwd32(ib, tables), want), key


def test_fp32_forward_within_gamma_n_of_float64():
    worst = 0.0
    for dim, key in CASES:
        ib, tables = P.case_inbox(dim, key), P.case_tables(dim)
        ref, scale, n = P.pool_fwd64(ib, tables)
        got = P.pool_fwd32(ib, tables)
        r = _ratio(got, ref, P.gamma(n)[..., None] * scale)
        assert r <= 1.0, (dim, key, r)
        assert np.all(got[n == 0] == 0) and not np.signbit(got[n == 0]).any()
        worst = max(worst, r)
    print(f"pool_inbox ref worst error / bound: fp32 forward against float64 {worst:.4f}")


def _routed(world, cap, B=9, Ls=(6, 20), rows=211, dim=16, seed=5):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((rows, dim)).astype(F32)
    ids, masks, wn = [], [], []
    for f, L in enumerate(Ls):
        kind = ("masked_mean", "mean")[f % 2]
        lens = rng.integers(0, L + 1, B)
        lens[0] = 0
        m = (np.arange(L)[None] < lens[:, None]).astype(F32)
        ids.append(rng.integers(0, rows, (B, L)))
        masks.append(m if kind == "masked_mean" else None)
        wn.append(R.bag_norm_weights(masks[-1], B, L, kind))
    return table, ids, masks, wn, R.route_bags(ids, wn, world, cap)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_owner_partials_summed_reproduce_array_pool(world):
    """One source, `world` owners (the composition of test_pooled_bag_channel_vs_oracle).  Against float64 the summed partials carry at most
    L + world + 3 roundings per term (the weight m / den: 2, the product: 1, the run's adds: <= L - 1, the owners' adds: <= world, one spare) and
    array_pool's own float32 evaluation L + 2 (product, L - 1 adds, den, the division); the two may differ by the sum of both bounds."""
    B, Ls, dim, cap = 9, (6, 20), 16, 233
    table, ids, masks, wn, (send, tag, sw, c2, worst) = _routed(world, cap, B, Ls, dim=dim)
    assert worst <= cap
    nf = len(Ls)
    total = np.zeros((nf * B, dim), F32)
    for o in range(world):
        shard = table[o::world]
        recv = np.zeros((world, nf), np.int64)
        recv[0] = c2[o]
        rows_, tag_, w_ = (np.r_[a[o * cap:(o + 1) * cap], np.full((world - 1) * cap, fill)] for a, fill in ((send, 10 ** 9), (tag, -5), (sw, np.nan)))
        ib = P.inbox_from_arrays(world, nf, B, cap, dim, [shard.shape[0]], [0] * nf, rows_, tag_, w_, recv)
        part = P.pool_fwd32(ib, [shard])
        assert np.all(part[1:] == 0)
        assert P.same_bits(part, R.pool_inbox([shard], [0] * nf, B, world, cap, recv, ib.rows, ib.tag, ib.w, dim))
        total = total + part[0]
    for f, L in enumerate(Ls):
        emb = table[ids[f]]
        m = np.ones((B, L)) if masks[f] is None else masks[f].astype(np.float64)
        den = m.sum(1) + (0.0 if masks[f] is None else np.float64(P.EPS32))
        scale = (np.abs(emb.astype(np.float64)) * m[..., None]).sum(1) / den[:, None]
        bound = (P.gamma(L + world + 3) + P.gamma(L + 2)) * scale
        r = _ratio(total[f * B:(f + 1) * B], R.array_pool(emb, masks[f]).astype(np.float64), bound)
        print(f"pool_inbox ref worst error / bound: summed partials against array_pool world={world} L={L} {r:.4f}")
        assert r <= 1.0, (f, r)


@pytest.mark.parametrize("world,cap", [(1, 400), (2, 150), (3, 97), (3, 40)])
def test_run_bounds_are_route_bags_runs(world, cap):
    """pool_mark_kernel's bounds from the routed tags = the bounds the routing launch writes itself.  cap = 40 overflows: a run cut at cap agrees;
    a run wholly past cap is empty in both, (cap, cap) there and (0, 0) here."""
    table, ids, masks, wn, (send, tag, sw, c2, worst) = _routed(world, cap)
    assert (worst > cap) == (cap == 40)
    want = R.route_bags_runs(ids, wn, world, cap)
    got = P.mark_runs(tag, c2, world, cap, want.shape[1])
    live = want[..., 1] > want[..., 0]
    assert np.array_equal(got[live], want[live]) and live.any()
    assert np.all(got[~live] == 0)
    if worst <= cap:
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------- backward, norm weights, element-wise
@pytest.mark.parametrize("skip_row0", [0, 1])
def test_expansion_scattered_by_its_owner_ids_is_the_dense_backward(skip_row0):
    for dim in (5, 16):
        ib = P.case_inbox(dim, "ntag1" if dim == 5 else f"ntag{3 * P.tb(dim) + 5}")          # one feature, one table (index 1)
        big = P.case_inbox(dim, f"ntag{3 * P.tb(dim) + 5}")
        for box in (ib, big):
            g = P.case_g_partial(box)
            ids, live, g_rows = P.pool_expand(box, P.TABLE_ROWS[1], skip_row0, g)
            grad, n, scale, single = P.pool_bwd64(box, g, skip_row0)[1]
            acc = np.zeros_like(grad)
            np.add.at(acc, ids[live] - 1, g_rows[live].astype(np.float64))
            assert _ratio(acc, grad, P.gamma(1) * scale) <= 1.0              # (g_rows is fp32(w g): one rounding per term)
            assert np.isnan(g_rows[~live]).all() and np.all(ids[~live] == 0)
            assert np.array_equal(np.bincount(ids[live] - 1, minlength=grad.shape[0]), n)
            assert P.same_bits(single[n == 1], acc[n == 1].astype(F32))
            assert np.array_equal(P.pool_payload(box, P.TABLE_ROWS[1], skip_row0) != 0,
                                  live & (np.repeat(np.arange(box.world), box.cap) * box.ntag + box.tag != 0))


def test_norm_weights_are_the_oracles():
    for L in P.NORM_LS:
        for B in P.norm_batches(L):
            binary, weighted = P.norm_masks(B, L)
            assert not binary[0].any() and (B == 1 or binary[1].all())
            for kind in P.NORM_KINDS:
                out, inv = P.norm_weights32(binary, B, L, kind)
                assert P.same_bits(out, R.bag_norm_weights(binary, B, L, kind)), (L, B, kind)
                if kind != "masked_mean":
                    assert P.same_bits(P.norm_weights32(None, B, L, kind)[0], R.bag_norm_weights(None, B, L, kind)), (L, B, kind)
            out, inv = P.norm_weights32(binary, B, L, "masked_mean")
            assert np.all(out[0] == 0) and inv[0] == 0
            ref, rinv = P.norm_weights64(binary, B, L)
            assert _ratio(out, ref, P.gamma(L + 2) * np.abs(ref)) <= 1.0
            ne = binary.any(1)                                               # (an empty bag: inv is 0 by definition, not 1 / 1e-8)
            assert _ratio(inv[ne], rinv[ne], P.gamma(L + 2) * np.abs(rinv[ne])) <= 1.0 and np.all(inv[~ne] == 0)
            assert P.same_bits(P.norm_weights32(None, B, L, "mean")[0], np.full((B, L), F32(1) / F32(L), F32))


def test_element_wise_definitions_on_hand_made_inputs():
    g = np.arange(12, dtype=F32).reshape(2, 6)
    got = P.upstream_rows(g, 1, 3, np.array([2, -1], F32), 2)
    assert got.shape == (2, 2, 3) and np.array_equal(got[1], [[2, 4, 6], [-7, -8, -9]])
    assert np.array_equal(P.upstream_rows(g, 2, 2, None, 1)[0], [[2, 3], [8, 9]])
    keys = P.table_keys([np.array([3, -4], np.int32), np.zeros(0, np.int32), np.array([(1 << 40) - 1], np.int64)], [5, 0, 7])
    assert keys.tolist() == [(5 << 40) | 3, 5 << 40, (7 << 40) | ((1 << 40) - 1)]
    tag = np.array([0, 1, -5, 2, 9, 1], np.int32)                           # cap 3, n_tags 3, world 2
    order = np.array([0, 1, 2, 3, 4, 5, -1, 6, 1 << 40], np.int64)
    assert P.order_remap(order, 6, tag, 3, 3, 2).tolist() == [0, 1, 0, 5, 3, 4, 0, 0, 0]
    assert P.UPSTREAM_WRAP[0] * P.UPSTREAM_WRAP[1] > P.UPSTREAM_GRID_CAP * P.NRX_BLOCK
    assert sum(P.KEYS_LENS_WRAP) > P.KEYS_GRID_CAP * P.NRX_BLOCK and 0 in P.KEYS_LENS_WRAP and 0 in P.KEYS_LENS_SMALL
    assert {c[4] for c in P.UPSTREAM_CASES} == {1, 3} and {c[0] for c in P.UPSTREAM_CASES} == {1, 16, 257}
    assert all(c[2] > 0 and c[3] > 0 for c in P.UPSTREAM_CASES) and any(c[4] > 1 and c[5] > 0 for c in P.UPSTREAM_CASES)


# ------------------------------------------------------------------------------------------------- mistakes the checks must not hide
def test_structural_mistakes_of_the_forward_leave_the_bound():
    """(a) run bounds swapped in the marking pass: every run is empty, every partial zero.  (b) the slots of a trip past the run's end keep their
    weight: they re-read the run's first entry (e = lo), which is then added once per padded slot."""
    for dim in (3, 16, 300):
        ib, tables = P.case_inbox(dim, "main"), P.case_tables(dim)
        ref, scale, n = P.pool_fwd64(ib, tables)
        bound = P.gamma(n)[..., None] * scale
        swapped = np.zeros_like(ref)
        assert _ratio(swapped, ref, bound) > 1e3
        lo = ib.run[..., 0].astype(np.int64) + np.arange(ib.world)[:, None] * ib.cap
        pad = (-n) % P.AHEAD
        first = np.zeros_like(ref)
        for x, table in enumerate(tables):
            sel = (np.asarray(ib.feat_table)[np.arange(ib.ntag) // ib.batch] == x)[None] & (n > 0)
            row = ib.rows[lo]
            ok = sel & (row >= 0) & (row < table.shape[0])
            first[ok] = table[row[ok]].astype(np.float64) * ib.w[lo][ok][:, None]
        stale = ref + pad[..., None] * first
        bad = (np.abs(stale - ref) > bound).any(-1)
        assert bad[(pad > 0) & (n > 0) & np.any(first != 0, -1)].all() and bad.any()
