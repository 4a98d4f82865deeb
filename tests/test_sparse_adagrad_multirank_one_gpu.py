"""Row-wise Adagrad through the bound sharded step at world 2: two rank processes on cuda:0, gloo, host-staged exchanges, the BUFFERED forms
(one_sided=False, direct_grad=False; the transport of tests/test_bf16_sharded_step_multirank_one_gpu.py), bf16 arenas, two optimizer steps with
fresh ids each step.

  * The union of the ranks' arenas and of their row-wise state ([1 + local rows] per arena) after two
    FusedSparseAdagrad(row_maps=arena_row_map(rank, world)) steps equals, bit for bit, the UNSHARDED bf16 tables and their [rows] state trained by
    the direct path + FusedSparseAdagrad (same sr_seed) on the rank-major concatenation of the batches: the row-wise sum of squares has one order
    per dim, and the rounding hash takes the global row.
  * The replicated table is updated from the reduced sink entries: the same bits on both ranks after every step."""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from news_recsys_amd import ops, shard_step
from news_recsys_amd._lib import NRX_FEAT_TABLE_BF16, NRX_SPARSE
from news_recsys_amd.model.model_utils.optim import FusedSparseAdagrad
from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
from tests.test_sharding_gloo import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR_SEED, LR, EPS, STEPS, B = 0x5EED0ADA, 5e-2, 1e-10, 2, 600
RANK_TIME_LIMIT = 120          # seconds a rank process gets to deliver its result; then it is killed and the test fails
# (feature, table, dim, rows, replicated)
SPEC = [("a", "a", 16, 3001, False), ("b", "b", 32, 7000, False), ("item_id", "item_id", 16, 900, False), ("last_click", "item_id", 16, 900, False),
        ("cat", "cat", 16, 50, True)]
NAMES = sorted({t for _, t, _, _, _ in SPEC})
REP = {t for _, t, _, _, r in SPEC if r}
WIDTH = sum(d for _, _, d, _, _ in SPEC)


def _full_tables():
    gen = torch.Generator().manual_seed(29)
    tabs = {}
    for _, t, d, r, _ in SPEC:
        if t not in tabs:
            tabs[t] = torch.randn(r, d, generator=gen).to(torch.bfloat16)
            tabs[t][0] = 0
    return tabs


def _ids(rank, it):
    rng = np.random.default_rng([710, rank, it])
    ids = []
    for _, t, d, r, _ in SPEC:
        x = rng.integers(0, r, B)
        x[:4] = 0                                         # padding ids on every rank
        if r > 1000:
            x[rng.random(B) < 0.05] = 17                  # a hot row, looked up by both ranks
        ids.append(x)
    return ids


def _g_out(rank):
    return np.random.default_rng(810 + rank).standard_normal((B, WIDTH)).astype(np.float32)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _worker(rank, world, port, q):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        full = _full_tables()
        a16 = {t: full[t].to(DEV) if t in REP else shard_step.make_arena(*full[t].shape, rank, world, DEV, full=full[t].to(DEV), dtype=torch.bfloat16)
               for t in NAMES}
        feats = [ShardedFeature(nm, NRX_SPARSE, t, d, 0, False, False, rep) for nm, t, d, _, rep in SPEC]
        inputs = [torch.from_numpy(x).to(DEV) for x in _ids(rank, 1)]
        g_out = torch.from_numpy(_g_out(rank)).to(DEV)
        eng = RowShardedEmbedding(rank, world, slack=0.5, host_staged=True, overflow_policy="defer")
        step = shard_step.PreparedShardedStep(eng, feats, inputs, [None] * len(feats), a16, one_sided=False, replicated_grads=True)
        step.bind_backward(g_out, None, direct_grad=False)
        assert step.bf16
        assert all(not g["placed"] for g in step.groups) and all(not b["direct"] for b in step.bwd)      # the buffered forms
        maps = [(1, 0) if t in REP else shard_step.arena_row_map(rank, world) for t in NAMES]
        p16 = [a16[t] for t in NAMES]
        sink = ops.SparseGradSink()
        opt = FusedSparseAdagrad(sink, lr=LR, eps=EPS, rowwise=True, params=p16, sr_seed=SR_SEED, weight_decay=0.01, row_maps=maps)
        rep_bits = []
        for it in range(1, STEPS + 1):
            for x, new in zip(inputs, _ids(rank, it)):
                x.copy_(torch.from_numpy(new))
            step.run()
            entries = step.backward()
            torch.cuda.synchronize()
            dist.barrier()
            sink.pending.extend(entries)
            opt.step()
            torch.cuda.synchronize()
            rep_bits.append({t: _bits(a16[t]) for t in REP})
            dist.barrier()
        assert not step.overflowed()
        arenas = {t: _bits(a16[t]) for t in NAMES if t not in REP}
        sums = {t: opt.sums[k].cpu().numpy() for k, t in enumerate(NAMES)}
        assert all(sums[t].shape == (a16[t].shape[0],) for t in NAMES)
        q.put((rank, rep_bits, arenas, sums))
        dist.barrier()
    except Exception as e:                                # (the parent fails at once instead of waiting for a result that will not come)
        import traceback
        q.put((rank, f"{type(e).__name__}: {e} {traceback.format_exc()}"[:3000]))
        raise
    finally:
        dist.destroy_process_group()


def test_union_of_the_arenas_and_of_the_rowwise_state_is_the_unsharded_run():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            item = q.get(timeout=RANK_TIME_LIMIT)
            assert not isinstance(item[1], str), f"rank {item[0]}: {item[1]}"
            res[item[0]] = item[1:]
        for p in procs:
            p.join(timeout=RANK_TIME_LIMIT)
            assert p.exitcode == 0
    finally:
        for p in procs:                                   # every rank process under its own time limit: what is still running is ended
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    # ---- the unsharded bf16 model on the rank-major concatenation: the direct path + FusedSparseAdagrad, same sr_seed
    full = _full_tables()
    u16 = [full[t].to(DEV) for t in NAMES]
    slots, col = [], 0
    for nm, t, d, _, _ in SPEC:
        slots.append(ops.Slot(nm, NRX_SPARSE, NAMES.index(t), d, 0, col, flags=NRX_FEAT_TABLE_BF16))
        col += d
    plan = ops.EmbedPlan(slots, out_width=col)
    inputs = [torch.from_numpy(np.concatenate([_ids(r, 1)[k] for r in range(world)])).to(DEV) for k in range(len(SPEC))]
    g_out = torch.from_numpy(np.concatenate([_g_out(r) for r in range(world)])).to(DEV)
    fwd = ops.PreparedEmbed(plan, u16, inputs, [None] * len(SPEC))
    bwd = ops.PreparedSparseBackward(fwd, g_out)
    sink = ops.SparseGradSink()
    opt = FusedSparseAdagrad(sink, lr=LR, eps=EPS, rowwise=True, params=u16, sr_seed=SR_SEED, weight_decay=0.01)
    for it in range(1, STEPS + 1):
        for k, x in enumerate(inputs):
            x.copy_(torch.from_numpy(np.concatenate([_ids(r, it)[k] for r in range(world)])))
        fwd.run()
        sink.pending.extend([dict(tables=u16, dim=g["dim"], uniq=g["uniq"], values=g["values"], counts=g["counts"], cap=g["cap"]) for g in bwd.run()])
        opt.step()
        torch.cuda.synchronize()
        for t in REP:                 # replicated tables: the same bits on every rank after every step
            assert np.array_equal(res[1][0][it - 1][t], res[0][0][it - 1][t]), (it, t)
    for t in REP:
        assert not np.array_equal(res[0][0][-1][t], _bits(full[t])), f"{t}: the replicated table did not train"
        assert np.array_equal(res[0][2][t].view(np.int32), res[1][2][t].view(np.int32)) and res[0][2][t].any(), f"{t}: replicated state"
    for k, t in enumerate(NAMES):
        if t in REP:
            continue
        rows, D = full[t].shape
        got = np.zeros((rows, D), np.uint16)
        gs = np.zeros(rows, np.float32)
        for r in range(world):
            a = res[r][1][t]
            assert a.shape[0] == 1 + len(range(r, rows, world)) and not a[0].any()
            got[r::world] = a[1:]
            assert res[r][2][t][0] == 0                   # the dummy row has no state
            gs[r::world] = res[r][2][t][1:]
        want = u16[k].view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), f"{t}: the union of the arenas != the unsharded bf16 table"
        assert (got != _bits(full[t])).any(), f"{t}: nothing trained"
        assert np.array_equal(gs.view(np.int32), opt.sums[k].cpu().numpy().view(np.int32)), f"{t}: the union of the row-wise state != the unsharded state"
        assert gs.any()
