"""Replicated tables in the bound sharded step (shard_step.PreparedShardedStep(replicated_grads=True), shard_model_step_(replicate=...)) on one
GPU:
  * the three kernels of csrc/nrx_replicated.hip (nrx_rep_pack, nrx_rep_ordered_sum, nrx_rep_compact) at W = 3 and W = 8 shapes with fabricated
    partials, equal to their numpy definitions (tests/test_replicated_grads_gloo.py) bit for bit -- and the pipeline to the rank-order fold
    (W = 2 could not tell a wrong order: x + y = y + x);
  * world 1: a step mixing routed and replicated features -- single-valued, a bag, an FM plan, a wide plan -- returns the concat, the wide
    columns, the FM logit and the replicated tables' (keys, values) bit for bit as the direct path does on full tables; a captured step replays
    the eager bits; an out-of-range replicated id raises IndexError naming the feature at check();
  * shard_model_step_(replicate=...) on Deep (a replicated bag), FM and Wide&Deep (the wide tables replicated) trains like the unsharded model
    in `sparse_grad: fused` mode over three steps; full_state_dict round-trips.
No reference counterpart for the exchange (the reference is single-device: src/model/sort/deep/train.py:38-44); the arithmetic is autograd of
src/model/BaseModel/base_model.py:262-308 and src/model/sort/widedeep/model.py:58-66."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops, shard_step, sharding
from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_SPARSE
from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
from tests.conftest import CONFIGS, GOLDEN
from tests.test_replicated_grads_gloo import MASK, fold, layout_of, local_lists, np_compact, np_ordered_sum, np_pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------ the kernels
def _kernel_pipeline(rows, dims, world, touch):
    lib = _lib.load()
    lay, groups, per_t = layout_of(rows, dims, world)
    cf, cr, Cw = lay["cf"], lay["cr"], lay["C"]
    n = len(rows)
    voff = (C.c_int64 * n)(*[per_t[t][0] for t in range(n)])
    roff = (C.c_int64 * n)(*[per_t[t][1] for t in range(n)])
    rws = (C.c_int64 * n)(*rows)
    tdims = (C.c_int32 * n)(*dims)
    stream = torch.cuda.current_stream().cuda_stream
    sends = []
    for r in range(world):
        lists = local_lists(r, rows, dims, groups, touch)
        keys, vals, cnts, caps = [], [], [], []
        for k, v in lists:
            cap = len(k) + 5                                   # (a tail past the count: never read)
            kk = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
            kk[:len(k)] = torch.from_numpy(k).to(DEV)
            vv = torch.full((cap, v.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
            vv[:len(k)] = torch.from_numpy(v).to(DEV)
            keys.append(kk)
            vals.append(vv)
            cnts.append(torch.tensor([len(k), 0], dtype=torch.int64, device=DEV))
            caps.append(cap)
        buf = torch.full((world * Cw,), float("nan"), dtype=torch.float32, device=DEV)      # (the call zero-fills it)
        L = len(lists)
        ops.check(lib.nrx_rep_pack((C.c_void_p * L)(*[x.data_ptr() for x in keys]), (C.c_void_p * L)(*[x.data_ptr() for x in vals]),
                                   (C.c_void_p * L)(*[x.data_ptr() for x in cnts]), (C.c_int64 * L)(*caps),
                                   (C.c_int32 * L)(*[v.shape[1] for _, v in lists]), L, voff, roff, rws, tdims, n, world, cf, cr,
                                   buf.data_ptr(), stream), "nrx_rep_pack")
        torch.cuda.synchronize()
        want = np_pack(lists, per_t, world, cf, cr)
        assert np.array_equal(buf.cpu().numpy().view(np.int32), want.view(np.int32)), f"pack, rank {r}"
        sends.append(buf)
    full = torch.empty(world * Cw, dtype=torch.float32, device=DEV)
    for q in range(world):                                     # the all-to-all: chunk q of every rank, rank order
        recv = torch.stack([s[q * Cw:(q + 1) * Cw] for s in sends]).reshape(-1).contiguous()
        red = torch.full((Cw,), float("nan"), dtype=torch.float32, device=DEV)
        ops.check(lib.nrx_rep_ordered_sum(recv.data_ptr(), world, cf, cr, red.data_ptr(), stream), "nrx_rep_ordered_sum")
        torch.cuda.synchronize()
        want = np_ordered_sum(recv.cpu().numpy(), world, cf, cr)
        assert np.array_equal(red.cpu().numpy().view(np.int32), want.view(np.int32)), f"ordered sum, chunk {q}"
        full[q * Cw:(q + 1) * Cw] = red                        # the all-gather
    expect = fold(world, rows, dims, groups, touch)
    for g, (wk, wv) in zip(groups, expect):
        k = len(g)
        cap = sum(rows[t] for t in g)
        keys = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
        vals = torch.full((cap, dims[g[0]]), float("nan"), dtype=torch.float32, device=DEV)
        cnt = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        ws = torch.empty(max(8, lib.nrx_rep_compact_workspace(cap)), dtype=torch.uint8, device=DEV)
        ops.check(lib.nrx_rep_compact(full.data_ptr(), world, cf, cr, (C.c_int64 * k)(*[per_t[t][0] for t in g]),
                                      (C.c_int64 * k)(*[per_t[t][1] for t in g]), (C.c_int64 * k)(*[rows[t] for t in g]), (C.c_int32 * k)(*g), k,
                                      dims[g[0]], keys.data_ptr(), vals.data_ptr(), cap, cnt.data_ptr(), ws.data_ptr(), stream), "nrx_rep_compact")
        torch.cuda.synchronize()
        nu = int(cnt[0])
        ck, cv = np_compact(full.cpu().numpy(), world, cf, cr, [(t,) + per_t[t][:2] + (rows[t], dims[t]) for t in g])
        assert nu == len(ck) == len(wk)
        assert np.array_equal(keys[:nu].cpu().numpy(), ck) and np.array_equal(ck, wk)
        assert np.array_equal(vals[:nu].cpu().numpy().view(np.int32), cv.view(np.int32))
        assert np.array_equal(cv.view(np.int32), wv.view(np.int32))


@pytest.mark.parametrize("world", [3, 8])
def test_kernels_equal_their_definitions_and_give_the_rank_order_fold(world):
    _kernel_pipeline([18, 270, 18, 5, 41, 1], [8, 8, 8, 3, 5, 3], world, 0.4)


@pytest.mark.parametrize("world", [3, 8])
def test_kernels_at_c3_shapes(world):
    """C3's small tables (category 18, subcategory 270, user_click_category 18 rows at D = 64): every rank touches most rows."""
    _kernel_pipeline([18, 270, 18], [64, 64, 64], world, 0.9)


def test_kernels_at_c5_shapes():
    """C5's 10 smallest tables (1 000 - 20 661 rows, D = 32) at W = 8: tiles of the compaction, chunk boundaries inside tables."""
    rows = [1000, 1500, 2300, 3100, 4400, 6000, 8100, 11000, 15500, 20661]
    _kernel_pipeline(rows, [32] * 10, 8, 0.3)


# ------------------------------------------------------------------ world 1 against the direct path
def _case(case, rng, gen):
    """(features, rows per table, dims per table, replicated tables, batch, bag length)."""
    R = True
    if case == "single":
        spec = [("a", "a", 16, 5000, False), ("b", "b", 32, 9000, False), ("cat", "cat", 16, 18, R), ("uc", "cat", 16, 18, R),
                ("sub", "sub", 16, 270, R), ("c", "c", 32, 40, R)]
    elif case == "bag":
        spec = [("a", "a", 16, 5000, False), ("cat", "cat", 16, 18, R), ("hist", "tags", 16, 40, R)]
    elif case == "fm":
        spec = [("a", "a", 16, 5000, False), ("b", "b", 16, 3000, False), ("cat", "cat", 16, 18, R), ("sub", "sub", 16, 270, R)]
    else:   # wide
        spec = [("a", "a", 16, 5000, False), ("cat", "cat", 17, 18, R), ("sub", "sub", 17, 270, R), ("uc", "uc", 17, 18, R)]
    wide = {"cat", "sub"} if case == "wide" else set()
    L = 6
    feats = [ShardedFeature(nm, NRX_BAG_MASKED_MEAN if nm == "hist" else NRX_SPARSE, tb, d, L if nm == "hist" else 0, nm in wide, case == "fm", rp)
             for nm, tb, d, _, rp in spec]
    rows = {tb: r for _, tb, _, r, _ in spec}
    dims = {tb: d for _, tb, d, _, _ in spec}
    return feats, rows, dims, L


def _inputs(feats, rows, B, L, rng):
    inputs, weights = [], []
    for f in feats:
        if f.kind == NRX_BAG_MASKED_MEAN:
            mask = (np.arange(L)[None, :] < rng.integers(0, L + 1, B)[:, None]).astype(np.float32)
            inputs.append(torch.from_numpy(np.where(mask > 0, rng.integers(1, rows[f.table], (B, L)), 0)).to(DEV))
            weights.append(torch.from_numpy(mask).to(DEV))
        else:
            x = rng.integers(0, rows[f.table], B)
            x[:3] = 0
            inputs.append(torch.from_numpy(x).to(DEV))
            weights.append(None)
    return inputs, weights


def _build(case, B=4000, one_sided=False, check_index=False, seed=5):
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    feats, rows, dims, L = _case(case, rng, gen)
    full = {t: torch.randn((rows[t], dims[t]), device=DEV, generator=gen) for t in rows}
    for t in full:
        full[t][0].zero_()
    arenas = {t: (full[t] if any(f.replicated for f in feats if f.table == t) else shard_step.make_arena(rows[t], dims[t], 0, 1, DEV, full=full[t]))
              for t in rows}
    inputs, weights = _inputs(feats, rows, B, L, rng)
    eng = RowShardedEmbedding(0, 1, overflow_policy="defer")
    step = shard_step.PreparedShardedStep(eng, feats, inputs, weights, arenas, one_sided=one_sided, check_index=check_index, replicated_grads=True,
                                          train=True)
    g_out = torch.randn((B, step.ld), device=DEV, generator=gen)
    g_fm = torch.randn((B,), device=DEV, generator=gen) if case == "fm" else None
    g_wide = torch.randn((B, step.plan.wide_width), device=DEV, generator=gen) if case == "wide" else None
    step.bind_backward(g_out, g_fm, g_wide=g_wide)
    return step, feats, full, inputs, weights, g_out, g_fm, g_wide


def _direct(step, feats, full, inputs, weights, g_out, g_fm, g_wide):
    names = sorted(full)
    slots = [dataclasses.replace(step.plan.slots[i], table=names.index(f.table), flags=0) for i, f in enumerate(feats)]
    plan = ops.EmbedPlan(slots, out_width=step.plan.out_width, wide_width=step.plan.wide_width, use_fm=step.plan.use_fm)
    sums = torch.empty((inputs[0].shape[0], 16), dtype=torch.float32, device=DEV) if plan.use_fm else None
    fwd = ops.PreparedEmbed(plan, [full[t] for t in names], inputs, weights, out_ld=step.ld, fm_sums=sums)
    out, wide, fmv = fwd.run()
    groups = ops.PreparedSparseBackward(fwd, g_out, g_fm, g_wide=g_wide).run()
    torch.cuda.synchronize()
    return out, wide, fmv, groups, names


def _rows_of(entries, table_name_of):
    """{(table name, row): value bits} over entries whose key table maps to a name (table_name_of(entry, t) -> name or None)."""
    res = {}
    for e in entries:
        nu = int(e["counts"][0])
        k = e["uniq"][:nu].cpu().numpy()
        v = e["values"][:nu].cpu().numpy().view(np.int32)
        for kk, vv in zip(k, v):
            nm = table_name_of(e, int(kk >> 40))
            if nm is not None:
                assert (nm, int(kk & MASK)) not in res
                res[(nm, int(kk & MASK))] = vv.tolist()
    return res


@pytest.mark.parametrize("case,one_sided", [("single", False), ("single", True), ("bag", False), ("fm", False), ("wide", False)])
def test_world_1_step_with_replicated_tables_equals_the_direct_path_bit_for_bit(case, one_sided):
    step, feats, full, inputs, weights, g_out, g_fm, g_wide = _build(case, one_sided=one_sided)
    for _ in range(2):
        out, wide, fmv = step.run()
        entries = step.backward()
    torch.cuda.synchronize()
    d_out, d_wide, d_fm, d_groups, names = _direct(step, feats, full, inputs, weights, g_out, g_fm, g_wide)
    assert torch.equal(out.view(torch.int32), d_out.view(torch.int32))
    if case == "wide":
        assert wide is not None and torch.equal(wide.view(torch.int32), d_wide.view(torch.int32))
    if case == "fm":
        assert torch.equal(fmv.view(torch.int32), d_fm.view(torch.int32))
    rep = step.rep_names
    assert sorted(rep) == sorted({f.table for f in feats if f.replicated})
    rep_entries = [e for e in entries if e["tables"] is step.rep["tables"]]
    assert len(rep_entries) == len({f.dim for f in feats if f.replicated})
    got = _rows_of(rep_entries, lambda e, t: rep[t])
    want = _rows_of(d_groups, lambda e, t: names[t] if names[t] in rep else None)
    assert got.keys() == want.keys() and len(got) > 0
    assert got == want
    # the routed tables still train (their entries are the exchange groups')
    assert len(entries) > len(rep_entries)


def test_world_1_step_with_replicated_tables_is_capturable():
    step, *_ = _build("fm")
    for _ in range(3):
        out, _, fm = step.run()
        entries = step.backward()
    torch.cuda.synchronize()
    want = (out.clone(), fm.clone(), [(e["uniq"].clone(), e["values"].clone(), int(e["counts"][0])) for e in entries])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2, _, fm2 = step.run()
        entries2 = step.backward()
    out2.zero_()
    for e in entries2:
        e["values"].zero_()
        e["counts"].zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2.view(torch.int32), want[0].view(torch.int32)) and torch.equal(fm2.view(torch.int32), want[1].view(torch.int32))
    assert len(entries2) == len(want[2])
    for e, (k, v, n) in zip(entries2, want[2]):
        assert int(e["counts"][0]) == n and torch.equal(e["uniq"][:n], k[:n]) and torch.equal(e["values"][:n].view(torch.int32), v[:n].view(torch.int32))


def test_out_of_range_replicated_id_raises_index_error_naming_the_feature():
    step, feats, full, inputs, *_ = _build("single", check_index=True)
    step.run()
    step.check()                                       # clean batch: nothing recorded
    k = next(i for i, f in enumerate(feats) if f.name == "sub")
    inputs[k][7] = 270                                 # one past the table
    step.run()
    with pytest.raises(IndexError, match="'sub'"):
        step.check()
    inputs[k][7] = 1
    step.run()
    step.check()                                       # the record was cleared


def test_routed_wide_feature_is_refused():
    eng = RowShardedEmbedding(0, 1, overflow_policy="defer")
    t = torch.zeros((18, 17), device=DEV)
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="replicate"):
        shard_step.PreparedShardedStep(eng, [ShardedFeature("cat", NRX_SPARSE, "cat", 17, 0, True)], [ids], [None],
                                       {"cat": shard_step.make_arena(18, 17, 0, 1, DEV, full=t)})


# ------------------------------------------------------------------ the module surface
def _model(cls, cfg, g):
    m = cls(os.path.join(CONFIGS, cfg))
    m.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
    m = m.to(DEV)
    m.sparse_grad = "fused"
    return m


def _classes():
    from news_recsys_amd.model.sort.deep.model import Deep
    from news_recsys_amd.model.sort.fm.model import FM
    from news_recsys_amd.model.sort.widedeep.model import WideDeep
    return {"Deep": Deep, "FM": FM, "WideDeep": WideDeep}


@pytest.mark.parametrize("cls_name,cfg,gname,replicate,below", [
    ("Deep", "cf_array_small.yaml", "model_deep_array", ("category", "user_click_cats"), 0),
    ("FM", "cf_fm_small.yaml", "model_fm", (), 18 * 16 * 4),
    ("WideDeep", "cf_widedeep_small.yaml", "model_widedeep", ("category", "subcategory", "user_click_category"), 0),
    ("WideDeep", "cf_widedeep_small.yaml", "model_widedeep", ("category", "subcategory", "user_click_category", "user_id", "item_id"), 0),
])
def test_model_with_replicated_tables_trains_like_the_unsharded_fused_model(cls_name, cfg, gname, replicate, below):
    cls = _classes()[cls_name]
    g = dict(np.load(os.path.join(GOLDEN, gname + ".npz"), allow_pickle=False))
    batch = {k[6:]: torch.from_numpy(v).to(DEV) for k, v in g.items() if k.startswith("batch/")}
    ref, shd = _model(cls, cfg, g), _model(cls, cfg, g)
    keys_before = sorted(shd.state_dict())
    shard_step.shard_model_step_(shd, 0, 1, replicate=replicate, replicate_below_bytes=below)
    assert sorted(shd.state_dict()) == keys_before
    assert shd._replicated_tables
    for t in shd._replicated_tables:
        w = shd.embedding_tables[t].weight
        assert w.shape == ref.embedding_tables[t].weight.shape and not w.requires_grad
    opt_r = ref.configure_optimizers()["optimizer"]
    opt_s = shd.configure_optimizers()["optimizer"]
    for it in range(3):
        for m, opt in ((ref, opt_r), (shd, opt_s)):
            opt.zero_grad()
            out = m(batch)
            loss = m.bceLoss(out, batch["label"][:, 0])
            loss.backward()
            opt.step()
            if m is ref:
                o_ref = out.detach().clone()
        torch.testing.assert_close(out.detach(), o_ref, rtol=1e-5, atol=1e-6)
    dp = sharding.data_parallel_params(shd)
    assert all(p.grad is None for p in dp if any(p is shd.embedding_tables[t].weight for t in shd._replicated_tables))
    full = sharding.full_state_dict(shd)
    want = ref.state_dict()
    assert sorted(full) == sorted(want)
    for k in want:
        torch.testing.assert_close(full[k], want[k], rtol=1e-5, atol=1e-6, msg=lambda s, k=k: f"{k}: {s}")
    for t in shd._replicated_tables:      # the replicated tables moved (they are not frozen)
        assert not torch.equal(full[f"embedding_tables.{t}.weight"], torch.from_numpy(g[f"param/embedding_tables.{t}.weight"]).to(DEV))
    again = _model(cls, cfg, g)
    shard_step.shard_model_step_(again, 0, 1, replicate=replicate, replicate_below_bytes=below)
    sharding.load_full_state_dict_(again, full)
    fresh = _model(cls, cfg, g)
    fresh.load_state_dict(full, strict=True)
    with torch.no_grad():
        torch.testing.assert_close(again(batch), fresh(batch), rtol=1e-5, atol=1e-6)
