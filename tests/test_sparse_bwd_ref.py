"""tests/sparse_bwd_ref.py held to account on the CPU, so that the GPU tests (tests/test_sparse_bwd_kernels_gpu.py) compare the reduction kernels of
the row-sparse backward with something that has itself been checked:
  * its definition is oracle/ref_np.py's (embedding_grad_dense, array_pool_bwd, fm_logit_bwd), float64 autograd of nn.Embedding + pooling + the
    FM formula (base_model.py:262-308, fm/model.py:18-26, widedeep/model.py:53-69), and the embedding goldens;
  * its restated workspace sizes are the library's, where the library loads;
  * every integer case keeps every sum of |terms| below 2^24;
  * the model of the decomposition equals the definition on every listed case, and its work-list counters are the ones the plan implies;
  * the case lists reach every edge they were computed for -- the test fails when a list stops reaching one;
  * nine planted mistakes in the model each leave the definition on a listed case."""
import functools

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib
from oracle import ref_np as R
from tests import sparse_bwd_ref as P
from tests.test_oracle_golden import batch_of, load, params_of, space_of, tables_of

NAMES = sorted(P.cases())
SMALL = [n for n in NAMES if P.case(n).n_lookups <= 4000]


def _dense(case, plan, vals):
    out = [np.zeros((r, case.dim), np.float64) for r in case.rows]
    for u, key in enumerate(plan.uniq):
        out[int(key >> 40)][int(key & P.ROW_MASK)] = vals[u]
    return out


# ------------------------------------------------------------------------------------------------- the definition
def _oracle_dense(case):
    """The dense table gradients from oracle/ref_np.py's pieces: per feature the upstream rows (wide split, FM term, pooling backward), scattered."""
    D, B = case.dim, case.batch
    out = [np.zeros((r, D), np.float64) for r in case.rows]
    fields = [i for i, f in enumerate(case.feats) if f.fm] if case.fm is not None else []
    if fields:
        x = np.stack([case.fm.feat[:, case.feats[i].out_col:case.feats[i].out_col + D] for i in fields], axis=1)        # [B, F, D]
        gw, gv, _ = R.fm_logit_bwd(x[:, :, 0], x[:, :, 1:], case.fm.g_fm.reshape(B, 1))
    for i, f in enumerate(case.feats):
        if f.wide_col >= 0:
            up = np.concatenate([case.g_wide[:, f.wide_col:f.wide_col + 1], case.g_out[:, f.out_col:f.out_col + D - 1]], axis=1)
        else:
            up = case.g_out[:, f.out_col:f.out_col + D] if case.g_out is not None else np.zeros((B, D), np.float32)
        if i in fields:
            k = fields.index(i)
            up = up + np.concatenate([gw[:, k].reshape(B, 1), gv[:, k]], axis=1)
        ids = P.mapped_ids(case, i)
        if f.kind == P.SPARSE:
            rows = up
        elif f.kind == P.SUM:
            rows = up[:, None, :] * case.weights[i][:, :, None]
        else:
            rows = R.array_pool_bwd(np.zeros((B, f.bag_len, D), np.float32), case.weights[i] if f.kind == P.MASKED else None, up.astype(np.float32))
        out[f.table] += R.embedding_grad_dense(ids, np.asarray(rows, np.float32), case.rows[f.table])
    return out


@pytest.mark.parametrize("name", SMALL)
def test_definition_is_the_oracles(name):
    c, p, _, _, (vals, _) = P.solved(name)
    for a, b in zip(_dense(c, p, vals), _oracle_dense(c)):
        assert np.array_equal(a, b)


def _autograd_dense(case, rng):
    """float64 autograd of the forward the reference computes: nn.Embedding(padding_idx=0) rows, pooled, routed, concatenated; the FM logit."""
    D, B = case.dim, case.batch
    tabs = case.fm.tables if case.fm is not None else [rng.standard_normal((r, D)) for r in case.rows]
    ts = [torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in tabs]
    loss, fw, fv = 0.0, [], []
    for i, f in enumerate(case.feats):
        ids = torch.from_numpy(P.mapped_ids(case, i).reshape(case.ids[i].shape))
        e = torch.nn.functional.embedding(ids, ts[f.table], padding_idx=0)
        if f.kind == P.MASKED:
            w = torch.from_numpy(np.asarray(case.weights[i], np.float64))
            e = (e * w[:, :, None]).sum(1) / (w.sum(1, keepdim=True) + 1e-8)
        elif f.kind == P.MEAN:
            e = e.mean(1)
        elif f.kind == P.SUM:
            e = (e * torch.from_numpy(np.asarray(case.weights[i], np.float64))[:, :, None]).sum(1)
        if f.wide_col >= 0:
            loss = loss + (e[:, 0] * torch.from_numpy(case.g_wide[:, f.wide_col].astype(np.float64))).sum()
            loss = loss + (e[:, 1:] * torch.from_numpy(case.g_out[:, f.out_col:f.out_col + D - 1].astype(np.float64))).sum()
        elif case.g_out is not None:
            loss = loss + (e * torch.from_numpy(case.g_out[:, f.out_col:f.out_col + D].astype(np.float64))).sum()
        if case.fm is not None and f.fm:
            fw.append(e[:, 0])
            fv.append(e[:, 1:])
    if fw:
        v = torch.stack(fv, 1)
        fm = torch.stack(fw, 1).sum(1) + 0.5 * (v.sum(1) ** 2 - (v ** 2).sum(1)).sum(1)
        loss = loss + (fm * torch.from_numpy(case.fm.g_fm.astype(np.float64))).sum()
    loss.backward()
    return [t.grad.numpy() for t in ts]


AUTOGRAD = [n for n in SMALL if n.startswith(("b-d16", "gen-", "pad-", "ld-", "lines-f7"))]


@pytest.mark.parametrize("name", AUTOGRAD)
def test_definition_is_float64_autograd_of_the_reference_forward(name):
    c, p, _, _, (vals, _) = P.solved(name)
    for a, b in zip(_dense(c, p, vals), _autograd_dense(c, np.random.default_rng(1))):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)        # (integers against float64 sums of integers and power-of-two fractions; 1e-8 in the masked mean)


@pytest.mark.parametrize("name", sorted(P.real_cases()))
def test_real_valued_reference_is_float64_autograd(name):
    c = P.real_cases()[name]
    p = P.plan_of(c)
    vals, bound = P.real_reference(c, p)                              # (it reads the forward's float32 field sums; autograd forms them in float64)
    for a, b in zip(_dense(c, p, vals), _autograd_dense(c, np.random.default_rng(1))):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-4)
    assert np.isfinite(bound).all() and (bound >= 0).all()


@pytest.mark.parametrize("gname,cfg", [("model_deep", "cf_deep_small.yaml"), ("model_deep_array", "cf_array_small.yaml")])
def test_definition_reproduces_the_embedding_goldens(gname, cfg):
    """The golden table gradients of the reference's own backward, from the upstream gradient of the concat (recovered through the MLP in
    float64 as tests/test_oracle_golden.py does): one case per embedding width."""
    g = load(gname)
    space, names, _ = space_of(cfg)
    p, b = params_of(g), batch_of(g)
    ws, bs = R.mlp_params(p, "score_fc.network.network")
    acts = [g["out/features"].astype(np.float64)]
    for i, (W, bb) in enumerate(zip(ws, bs)):
        h = acts[-1] @ W.T.astype(np.float64) + bb
        acts.append(np.maximum(h, 0) if i < len(ws) - 1 else h)
    y = b["label"][:, :1].astype(np.float64)
    gz = (1 / (1 + np.exp(-acts[-1])) - y) / y.shape[0]
    for i in reversed(range(len(ws))):
        if i < len(ws) - 1:
            gz = gz * (acts[i + 1] > 0)
        gz = gz @ ws[i].astype(np.float64)
    _, dims, _, used = R.embed_concat_ex(space, tables_of(p), b, names)
    cols = np.concatenate([[0], np.cumsum(dims)])
    checked = 0
    for dim in sorted(set(dims)):
        feats, ids, weights, tnames = [], [], [], []
        for k, (fname, d) in enumerate(zip(used, dims)):
            tname = R.emb_table_name(fname, space.share)
            if d != dim or f"embedding_tables.{tname}.weight" not in p:
                continue
            if tname not in tnames:
                tnames.append(tname)
            arr = fname in space.array
            mask = b.get(fname + "_mask") if arr else None
            feats.append(P.Feat((P.MASKED if mask is not None else P.MEAN) if arr else P.SPARSE, tnames.index(tname), b[fname].shape[1] if arr else 0, int(cols[k])))
            ids.append(np.asarray(b[fname], np.int64))
            weights.append(None if mask is None else np.asarray(mask, np.float32))
        if not feats:
            continue
        c = P.Case(name=gname, dim=int(dim), batch=gz.shape[0], feats=feats, rows=[p[f"embedding_tables.{t}.weight"].shape[0] for t in tnames], ids=ids,
                   weights=weights, index_bits=64, g_out=gz.astype(np.float32), g_wide=None, fm=None, pads=P.NS(out=0, wide=0, feat=0, sums=0), shift=set(),
                   mode="sorted", dense=False, accumulate=0, ws=True, n_dev=None, place_feats=0)
        plan = P.plan_of(c)
        vals, _ = P.real_reference(c, plan)
        for t, got in zip(tnames, _dense(c, plan, vals)):
            want = g[f"grad/embedding_tables.{t}.weight"]
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7)
            checked += 1
    assert checked >= 2


# ------------------------------------------------------------------------------------------------- the library's sizes
def _c_feats(case):
    arr = (_lib.NrxFeature * len(case.feats))()
    for i, f in enumerate(case.feats):
        arr[i].kind, arr[i].bag_len, arr[i].dim = f.kind, f.bag_len, case.dim
    return arr


def test_workspace_sizes_are_the_librarys():
    lib = _lib.load()
    rng = np.random.default_rng(0)
    for n, dim in [(0, 1), (1, 16), (255, 16), (256, 64), (257, 32), (2047, 16), (2048, 16), (8192, 64), (8193, 300)] + \
                  [(int(rng.integers(0, 1 << 22)), int(rng.integers(1, 400))) for _ in range(200)]:
        assert lib.nrx_embed_bwd_sorted_workspace(n, dim) == P.sorted_workspace(n, dim), (n, dim)
    assert lib.nrx_embed_bwd_sorted_workspace(-1, 16) == -1 and lib.nrx_embed_bwd_sorted_workspace(5, 0) == -1
    for name in NAMES:
        c = P.case(name)
        assert lib.nrx_embed_bwd_workspace_for(_c_feats(c), len(c.feats), c.batch, c.dim) == P.workspace_for(c), name
    assert P.long_slots(32) == 32 and P.long_slots(33) == 33 + 2 + 1 and P.long_slots(129) == 129 + 5 + 2
    for n in (300, 9000, 70000, 1 << 20):                     # the capacities the workspace is sized by hold the worst case of n lookups
        worst_items = max(n // (P.LONG_T + 1), -(-n // P.CHUNK))
        assert worst_items <= n // P.LONG_T + 8
        assert P.long_slots(-(-n // P.CHUNK)) <= 2 * n // P.CHUNK + n // 2048 + 8
        assert (n // (P.CHUNK + 1)) * P.long_slots(2) <= 2 * n // P.CHUNK + n // 2048 + 8


# ------------------------------------------------------------------------------------------------- exactness, and the model
@pytest.mark.parametrize("name", NAMES)
def test_case_is_exact_and_the_model_equals_the_definition(name):
    c, p, sh, T, (vals, mag) = P.solved(name)
    assert P.exact_margin(c, mag) < 2 ** 24, name
    assert np.array_equal(vals, np.round(vals)) or not c.integer
    got, facts = P.model(c, p, sh, terms=T)
    written = ~np.isnan(got).any(1)
    assert np.array_equal(got[written], vals[written].astype(np.float64))
    small = isinstance(c.n_dev, int)
    assert written.all() or small, "only a device-side count below the host bound leaves rows unwritten"
    if small:
        assert not written.all()
    # the counters, from the plan alone
    seg_len = (p.seg[1:] - p.seg[:-1])
    listed = p.walk if sh.fast and sh.placed else np.arange(len(p.uniq))
    if small:
        listed = listed[:c.n_dev]
    live = listed[(p.uniq[listed] & P.ROW_MASK) != 0]
    lng = seg_len[live][seg_len[live] > getattr(sh, "long_t", 0)] if sh.fast and c.ws else np.zeros(0, np.int64)
    items = -(-lng // P.CHUNK)
    assert facts.items == items.sum() and facts.multi == (items > 1).sum() and facts.slots == sum(P.long_slots(int(k)) for k in items if k > 1)
    assert facts.items <= c.n_lookups // P.LONG_T + 8 and facts.slots <= 2 * c.n_lookups // P.CHUNK + c.n_lookups // 2048 + 8


# ------------------------------------------------------------------------------------------------- the lists reach their edges
@functools.lru_cache(maxsize=None)
def _reach():
    r = P.NS(lens={16: set(), 32: set()}, walk=set(), long=set(), place=set(), counts={4: set(), 2: set()}, pad=set(), strides=set(), general=set(),
             place_b=set(), lines=set(), layouts=set(), items=set(), entry=set())
    for name in NAMES:
        c, p, sh, _, _ = P.solved(name)
        seg_len = p.seg[1:] - p.seg[:-1]
        row = p.uniq & P.ROW_MASK
        if not sh.fast:
            r.general.add((c.dim, c.index_bits))
            if c.dim > 16 * 64:
                r.general.add("slow-loop" + ("-fm" if c.fm is not None else ""))
            if c.fm is not None and any(f.kind != P.SPARSE for f in c.feats):
                r.general.add("fm+bag")
            if any(f.wide_col >= 0 for f in c.feats) and c.dim % 2:
                r.general.add("wide-odd")
            if c.shift:
                r.layouts.add(("shift-off-fast", tuple(sorted(c.shift)), sh.refused))
            continue
        r.entry.add((c.mode, c.dense, c.accumulate, c.ws, c.index_bits))
        listed = p.walk if sh.placed else np.arange(len(p.uniq))
        if isinstance(c.n_dev, int):
            r.pad.add("n_dev-below-bound-" + c.mode)
            listed = listed[:c.n_dev]
        r.walk.add((sh.ql,) + sh.walk_inst)
        if sh.long_inst is not None and (seg_len[listed][row[listed] != 0] > sh.long_t).any():
            r.long.add((sh.ql,) + sh.long_inst)
        if sh.place_runs:
            r.place.add((sh.ql,) + sh.place_inst)
            r.place_b.add((sh.ql, c.batch - sh.tb))
            if sh.ql == 2:
                r.lines.add((sh.lines, c.batch, len(c.feats) % 2, len(c.feats), c.variant) if sh.lines else ("refused", c.name))
        if c.ws:
            for L in seg_len[listed][row[listed] != 0]:
                r.lens[sh.long_t].add(int(L))
                k = -(-int(L) // P.CHUNK)
                if k >= 65 and k % P.GROUP:
                    r.items.add("65+partial-group")
        n = len(listed)
        r.counts[sh.R].add((n - sh.R * sh.tb, n - 3 * sh.R * sh.tb))
        # padding rows
        for i, u in enumerate(listed):
            if row[u] != 0:
                continue
            t = int(p.uniq[u] >> 40)
            first_of_table = u == p.counts[1 + t]
            assert first_of_table
            r.pad.add("first-of-table")
            if t > 0:
                r.pad.add("second-table")
            if i % sh.R != 0 or (i + 1 < n and (i + 1) % sh.R != 0 and row[listed[i + 1]] != 0):
                r.pad.add("inside-a-lane-group")
            if c.ws and seg_len[u] > sh.long_t:
                r.pad.add("longer-than-long_t")
        if any(((np.asarray(a) < 0) | (np.asarray(a) >= c.rows[f.table])).any() for a, f in zip(c.ids, c.feats)):
            r.pad.add("ids-that-are-no-rows")
        if c.dim == 64:
            if c.mode != "pairs" and -(-sh.groups // sh.tb) > sh.grid == P.WALK_CAP:
                r.strides.add("walk")
            if c.mode == "pairs" and p.n_pairs > sh.pair_grid * sh.tb and sh.pair_grid == P.PAIR_CAP:
                r.strides.add("pairs")
            if c.mode == "pairs" and -(-sh.groups // sh.tb) > sh.grid == P.PAIR_WALK_CAP:
                r.strides.add("pair-walk")
        for k, v in vars(c.pads).items():
            if v:
                r.layouts.add("pad-" + k)
        if c.shift:
            r.layouts.add(("shift-stays-fast", tuple(sorted(c.shift))))
    return r


def test_lists_reach_every_segment_length():
    r = _reach()
    for t in (16, 32):
        assert {1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257} <= r.lens[t], (t, sorted(r.lens[t])[:40])
    both = r.lens[16] | r.lens[32]
    assert {P.COOP * P.CHUNK, P.COOP * P.CHUNK + 1, P.GROUP * P.CHUNK, P.GROUP * P.CHUNK + 1} <= both
    assert {1024, 1025} <= r.lens[16] and {1024, 1025} <= r.lens[32]
    assert r.items == {"65+partial-group"}


def test_lists_reach_every_padding_position_and_count():
    r = _reach()
    assert {"first-of-table", "second-table", "inside-a-lane-group", "longer-than-long_t", "ids-that-are-no-rows", "n_dev-below-bound-sorted",
            "n_dev-below-bound-placed"} <= r.pad, r.pad
    for R_ in (4, 2):
        assert {-1, 0, 1} <= {a for a, _ in r.counts[R_]} and 5 in {b for _, b in r.counts[R_]}, R_
    assert r.strides == {"walk", "pairs", "pair-walk"}
    for mode in ("sorted", "placed", "pairs"):
        assert any(e[0] == mode and e[4] == 32 for e in r.entry) and any(e[0] == mode and e[4] == 64 for e in r.entry)
    assert {("sorted", False, 0, False, 64), ("placed", True, 0, True, 64), ("placed", True, 1, True, 64), ("pairs", True, 1, True, 64)} <= \
        {e[:4] + (64,) for e in r.entry}


def test_lists_reach_every_branch_of_the_launch_tables():
    r = _reach()
    walk, long_, place = set(), set(), set()
    for ql in (2, 3, 4):
        for fm in (False, True):
            for dec in (0, 1):
                walk.add((ql, 2, fm, False, False, 4, dec, True))                  # pair records in the walk launch
            walk |= {(ql, 2, fm, False, False, 4, 1, False), (ql, 4, fm, False, False, 1, 1, False)}      # regular: placed, not placed
            long_.add((ql, fm, False, False, 1))
        for d in (2, 0):
            walk |= {(ql, 2, True, False, False, 4, d, False), (ql, 2, False, True, True, 4, d, False), (ql, 2, False, False, False, 4, d, False),
                     (ql, 4, True, False, False, 1, d, False), (ql, 4, False, True, True, 1, d, False), (ql, 2, False, True, False, 4, d, False),
                     (ql, 4, False, False, False, 1, d, False)}
            long_ |= {(ql, True, False, False, d), (ql, False, True, True, d), (ql, False, True, False, d), (ql, False, False, False, d)}
        place |= {(ql, "rows", fm, unal, dense) for fm, unal in ((False, False), (True, False), (False, True)) for dense in (False, True)}
    place |= {(2, "lines", fm, dense, hasg) for fm, hasg in ((False, True), (True, True), (True, False)) for dense in (False, True)}
    assert walk == r.walk, (sorted(walk - r.walk), sorted(r.walk - walk))
    assert long_ == r.long, (sorted(long_ - r.long), sorted(r.long - long_))
    assert place <= r.place, sorted(place - r.place)


def test_lists_reach_the_placement_pass_and_the_general_kernel_and_the_layouts():
    r = _reach()
    for ql in (2, 3, 4):
        assert {(ql, -1), (ql, 0), (ql, 1)} <= r.place_b
    lines = {x for x in r.lines if x[0] is True}
    assert {31, 32, 33} <= {x[1] for x in lines} and {0, 1} <= {x[2] for x in lines} and 64 in {x[3] for x in lines}
    assert {"plain", "fm", "fm_nog"} <= {x[4] for x in lines}
    assert {("refused", "lines-refused-ld"), ("refused", "lines-refused-cols")} <= r.lines
    assert {d for d, _ in (x for x in r.general if isinstance(x, tuple))} >= set(P.GENERAL_DIMS)
    assert {b for _, b in (x for x in r.general if isinstance(x, tuple))} == {32, 64}
    assert {"slow-loop", "slow-loop-fm", "fm+bag", "wide-odd"} <= r.general
    assert {"pad-out", "pad-wide", "pad-feat", "pad-sums"} <= r.layouts
    off = {x[1] for x in r.layouts if isinstance(x, tuple) and x[0] == "shift-off-fast"}
    assert {("values",), ("g_out",), ("feat",), ("sums",)} <= off
    assert ("shift-off-fast", ("values",), True) in r.layouts                      # pair records outside the placement shapes: refused
    assert ("shift-stays-fast", ("g_out",)) in r.layouts                           # one element in is 4-byte aligned: the unaligned kernels


# ------------------------------------------------------------------------------------------------- planted mistakes
@pytest.mark.parametrize("bug", P.BUGS)
def test_a_planted_mistake_in_the_model_is_caught_by_a_listed_case(bug):
    caught = []
    for name in NAMES:
        c, p, sh, T, (vals, _) = P.solved(name)
        if c.n_lookups > 60000 and bug not in ("no_second_trip",):
            continue
        good, gfacts = P.model(c, p, sh, terms=T)
        got, facts = P.model(c, p, sh, bug=bug)
        if not np.array_equal(np.nan_to_num(got, nan=1e30), np.nan_to_num(good, nan=1e30)) or vars(facts) != vars(gfacts):
            caught.append(name)
    assert caught, bug
    want = dict(ge_long_t="mid-", last_item_short="mid-", group_dropped="hot-", no_second_trip="stride-walk", no_second_pair_trip="stride-pairs",
                padding_summed="pad-", pair_second_dropped="pairs", walk_index_as_unique="placed", fm_col0_everywhere="fm")[bug]
    assert any(want in n for n in caught), (bug, caught[:5])
    if bug == "group_dropped":                                 # 33 items: the second group is one item
        assert any(P.GROUP * P.CHUNK + 1 in (P.solved(n)[1].seg[1:] - P.solved(n)[1].seg[:-1]) for n in caught)
