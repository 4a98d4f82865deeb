"""Replicated tables in the bound sharded step at world 2 and 3 with the PRODUCT kernels: the rank processes share cuda:0 and exchange through
gloo with host-staged buffers (RowShardedEmbedding(host_staged=True), a test transport; engine _a2a / _all_gather).

  * PreparedShardedStep(replicated_grads=True), buffered forms: the replicated entries are identical on every rank (keys and bits) and equal to
    the rank-order fold s = G_0; s = s + G_1; ... of every rank's DIRECT-path gradient (ops.PreparedSparseBackward on the full tables over that
    rank's batch), recomputed in the parent; after two FusedSparseAdam steps the replicas are identical across ranks.
  * shard_model_step_ at world 2 on a skewed-category batch (60 % of the category lookups hit one odd id): all-row-sharded, the first training
    step raises the overflow; with replicate=("category",) the same batch trains and matches the unsharded `sparse_grad: fused` model on the
    concatenated batch.
Every rank process honours NRX_TEST_POISON=1 (recycled memory filled with 0xFF).  No reference counterpart (the reference is single-device:
src/model/sort/deep/train.py:38-44)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from news_recsys_amd import ops, shard_step
from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_SPARSE
from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
from tests.test_sharding_gloo import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASK = (1 << 40) - 1

# (name, table, dim, rows, replicated, bag length)
SPEC = [("a", "a", 16, 5000, False, 0), ("b", "b", 32, 9000, False, 0), ("cat", "cat", 16, 18, True, 0), ("uc", "cat", 16, 18, True, 0),
        ("sub", "sub", 16, 270, True, 0), ("c", "c", 32, 40, True, 0), ("hist", "tags", 16, 40, True, 6)]
B = 1500


def _tables():
    rng = np.random.default_rng(21)
    tabs = {}
    for _, t, d, r, _, _ in SPEC:
        if t not in tabs:
            x = rng.standard_normal((r, d)).astype(np.float32)
            x[0] = 0
            tabs[t] = x
    return tabs


def _feats():
    return [ShardedFeature(nm, NRX_BAG_MASKED_MEAN if L else NRX_SPARSE, t, d, L, False, False, rp) for nm, t, d, _, rp, L in SPEC]


def _batch(rank):
    rng = np.random.default_rng(700 + rank)
    ids, masks = [], []
    for _, t, d, r, _, L in SPEC:
        if L:
            m = (np.arange(L)[None, :] < rng.integers(0, L + 1, B)[:, None]).astype(np.float32)
            ids.append(np.where(m > 0, rng.integers(1, r, (B, L)), 0))
            masks.append(m)
        else:
            x = rng.integers(0, r, B)
            x[:3] = 0
            x[rng.random(B) < 0.3] = 5 if r > 5 else 1     # a hot row every rank looks up
            ids.append(x)
            masks.append(None)
    return ids, masks


def _upstream(rank, width):
    rng = np.random.default_rng(800 + rank)
    return rng.standard_normal((B, width)).astype(np.float32)


def _step_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import _poison
    _poison.poison()
    try:
        from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
        tabs = _tables()
        feats = _feats()
        rep = {f.table for f in feats if f.replicated}
        arenas = {t: (torch.from_numpy(x).to(DEV) if t in rep else
                      shard_step.make_arena(x.shape[0], x.shape[1], rank, world, DEV, full=torch.from_numpy(x).to(DEV))) for t, x in tabs.items()}
        ids, masks = _batch(rank)
        inputs = [torch.from_numpy(x).to(DEV) for x in ids]
        weights = [None if m is None else torch.from_numpy(m).to(DEV) for m in masks]
        eng = RowShardedEmbedding(rank, world, slack=0.5, host_staged=True, overflow_policy="defer")
        step = shard_step.PreparedShardedStep(eng, feats, inputs, weights, arenas, one_sided=False, replicated_grads=True)
        g_out = torch.from_numpy(_upstream(rank, step.ld)).to(DEV)
        step.bind_backward(g_out, direct_grad=False)
        res = {}
        for it in range(2):
            step.run()
            entries = step.backward()
            torch.cuda.synchronize()
            rep_e = [e for e in entries if e["tables"] is step.rep["tables"]]
            got = {}
            for e in rep_e:
                nu = int(e["counts"][0])
                for k, v in zip(e["uniq"][:nu].cpu().numpy(), e["values"][:nu].cpu().numpy().view(np.int32)):
                    got[(step.rep_names[int(k >> 40)], int(k & MASK))] = v.tolist()
            res[f"entries{it}"] = got
        step.check()
        # two optimizer steps on the replicas from the replicated entries
        sink = ops.SparseGradSink()
        opt = FusedSparseAdam(sink, lr=1e-2)
        for _ in range(2):
            step.run()
            sink.pending.extend([e for e in step.backward() if e["tables"] is step.rep["tables"]])
            opt.step()
        torch.cuda.synchronize()
        res["replicas"] = {t: arenas[t].cpu().numpy().view(np.int32).tolist() for t in sorted(rep)}
        q.put((rank, res))
        dist.barrier()
    except Exception as e:
        import traceback
        q.put((rank, {"error": f"{type(e).__name__}: {e} {traceback.format_exc()}"[:3000]}))
        raise
    finally:
        dist.destroy_process_group()


def _run(world, target, args=()):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            item = q.get(timeout=400)
            res[item[0]] = item[1]
        for p in procs:
            p.join(timeout=120)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    for r in range(world):
        assert "error" not in res[r], (r, res[r].get("error"))
    return res


def _direct_local(rank, feats, tabs, plan_slots, ld):
    """Rank `rank`'s direct-path gradient on the full tables: {(table, row): float32 row}."""
    names = sorted(tabs)
    ids, masks = _batch(rank)
    slots = [dataclasses.replace(s, table=names.index(f.table), flags=0) for s, f in zip(plan_slots, feats)]
    plan = ops.EmbedPlan(slots, out_width=ld)
    full = [torch.from_numpy(tabs[t]).to(DEV) for t in names]
    fwd = ops.PreparedEmbed(plan, full, [torch.from_numpy(x).to(DEV) for x in ids],
                            [None if m is None else torch.from_numpy(m).to(DEV) for m in masks])
    fwd.run()
    groups = ops.PreparedSparseBackward(fwd, torch.from_numpy(_upstream(rank, ld)).to(DEV)).run()
    torch.cuda.synchronize()
    out = {}
    for g in groups:
        nu = int(g["counts"][0])
        for k, v in zip(g["uniq"][:nu].cpu().numpy(), g["values"][:nu].cpu().numpy()):
            out[(names[int(k >> 40)], int(k & MASK))] = v.copy()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_replicated_entries_are_the_rank_order_fold_on_every_rank(world):
    res = _run(world, _step_worker)
    tabs = _tables()
    feats = _feats()
    rep = {f.table for f in feats if f.replicated}
    eng = RowShardedEmbedding(0, world)
    groups, pooled = eng.plan_groups(feats)
    plan = eng._final_plan(feats, groups, pooled)
    locals_ = [_direct_local(r, feats, tabs, plan.slots, plan.out_width) for r in range(world)]
    keys = sorted({k for loc in locals_ for k in loc if k[0] in rep})
    want = {}
    for k in keys:
        s = None
        for loc in locals_:
            g = loc.get(k, np.zeros(tabs[k[0]].shape[1], np.float32))
            s = g.copy() if s is None else (s + g).astype(np.float32)
        want[k] = s.view(np.int32).tolist()
    assert len(want) > 0
    for r in range(world):
        for it in range(2):
            got = res[r][f"entries{it}"]
            assert got.keys() == want.keys(), f"rank {r}"
            assert got == want, f"rank {r} call {it}"
        assert res[r]["replicas"] == res[0]["replicas"]
    assert any(res[0]["replicas"][t] != tabs[t].view(np.int32).tolist() for t in rep)     # (they moved)


# ---------------------------------------------------------------------------------------------- a skewed category at world 2
def _skewed(world):
    from tests.conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "model_fm.npz"), allow_pickle=False))
    rng = np.random.default_rng(31)
    n = 1024 * world
    rows = {"user_id": 97, "item_id": 61, "category": 18, "subcategory": 27, "user_click_category": 18}
    batch = {k: torch.from_numpy(rng.integers(1, r, n)) for k, r in rows.items()}
    cat = rng.integers(1, 18, n)
    cat[rng.random(n) < 0.6] = 5                       # 60 % of the lookups on one odd id: owner 1 at world 2
    batch["category"] = torch.from_numpy(cat)
    batch["label"] = torch.from_numpy(rng.integers(0, 2, (n, 1)).astype(g["batch/label"].dtype))
    return g, batch


def _skew_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import _poison
    _poison.poison()
    res = {}
    try:
        from news_recsys_amd import sharding
        from news_recsys_amd.model.sort.fm.model import FM
        from tests.conftest import CONFIGS
        g, full = _skewed(world)
        n = 1024
        batch = {k: v[rank * n:(rank + 1) * n].contiguous().to(DEV) for k, v in full.items()}

        def make(**kw):
            m = FM(os.path.join(CONFIGS, "cf_fm_small.yaml"))
            m.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
            m = m.to(DEV)
            shard_step.shard_model_step_(m, rank, world, host_staged=True, **kw)       # the default slack (0.05)
            return m, m.configure_optimizers()["optimizer"]

        def train(m, opt):
            opt.zero_grad()
            m.bceLoss(m(batch), batch["label"][:, 0]).backward()
            grads = [p.grad for p in sharding.data_parallel_params(m) if p.grad is not None]
            flat = torch.cat([x.reshape(-1) for x in grads]).cpu()
            dist.all_reduce(flat)
            flat /= world
            off = 0
            for x in grads:
                x.copy_(flat[off:off + x.numel()].view_as(x))
                off += x.numel()
            opt.step()

        m, opt = make()
        try:
            train(m, opt)
            res["raised"] = False
        except RuntimeError as e:
            res["raised"] = "overflowed" in str(e)
        m, opt = make(replicate=("category",))
        res["replicated"] = list(m._replicated_tables)
        for _ in range(2):
            train(m, opt)
        shard_step.check_shard_steps(m)
        torch.cuda.synchronize()
        res["state"] = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        q.put((rank, res))
        dist.barrier()
    except Exception as e:
        import traceback
        q.put((rank, {**res, "error": f"{type(e).__name__}: {e} {traceback.format_exc()}"[:3000]}))
        raise
    finally:
        dist.destroy_process_group()


def test_skewed_category_overflows_row_sharded_and_trains_replicated():
    from news_recsys_amd.model.sort.fm.model import FM
    from tests.conftest import CONFIGS
    world = 2
    res = _run(world, _skew_worker)
    for r in range(world):
        assert res[r]["raised"], f"rank {r}: the all-row-sharded step did not raise the overflow"
        assert res[r]["replicated"] == ["category"]
    g, full = _skewed(world)
    ref = FM(os.path.join(CONFIGS, "cf_fm_small.yaml"))
    ref.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
    ref = ref.to(DEV)
    ref.sparse_grad = "fused"
    batch = {k: v.to(DEV) for k, v in full.items()}
    opt = ref.configure_optimizers()["optimizer"]
    for _ in range(2):
        opt.zero_grad()
        ref.bceLoss(ref(batch), batch["label"][:, 0]).backward()
        opt.step()
    want = {k: v.detach().cpu().numpy() for k, v in ref.state_dict().items()}
    for k, w in want.items():
        for r in range(world):
            got = res[r]["state"][k]
            if k == "embedding_tables.category.weight":
                np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-6, err_msg=f"{k} rank {r}")
                assert np.array_equal(got.view(np.int32), res[0]["state"][k].view(np.int32))      # identical replicas
            elif k.startswith("embedding_tables."):
                np.testing.assert_allclose(got[1:], w[r::world], rtol=1e-5, atol=1e-6, err_msg=f"{k} rank {r}")
            else:
                np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-6, err_msg=f"{k} rank {r}")
