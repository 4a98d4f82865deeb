"""bf16 arenas through the bound sharded step at world 2 and 3 with the product kernels: rank processes on cuda:0, gloo, host-staged exchanges
(the transport of tests/test_shard_step_multirank_one_gpu.py), the buffered and the one-sided / direct-gradient forms, three optimizer steps with
fresh ids each step.

  * The union of the ranks' arenas (and of both moments) after three FusedSparseAdam(row_maps=arena_row_map(rank, world)) steps equals, bit for
    bit, the UNSHARDED bf16 tables trained by the direct path + FusedSparseAdam (same sr_seed) on the rank-major concatenation of the batches.
  * On every rank and step the arenas equal tests/sr_bf16_ref.py's rounding of the fp32 FusedSparseAdam result (widened arena, the returned
    keys and values) with the GLOBAL rows in the hash -- and do NOT equal it with the arenas' local rows (so the test sees the row map).
  * The replicated bf16 table is bit-identical on every rank after every step and equals that restatement fed the reduced gradient the step
    returned (its map is the identity).  Its rank-order fold is not the direct reduction's order, so it is not compared with the unsharded run.
  * `tiny` has 2 rows: at world 3 the last rank's shard is empty (the dummy row alone)."""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from news_recsys_amd import ops, shard_step
from news_recsys_amd._lib import NRX_FEAT_TABLE_BF16, NRX_SPARSE
from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
from tests import sr_bf16_ref as SR
from tests.test_sharding_gloo import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASK = (1 << 40) - 1
SR_SEED, LR, STEPS, B = 0xABCDEF987, 3e-2, 3, 1500
# (feature, table, dim, rows, replicated)
SPEC = [("a", "a", 16, 5000, False), ("b", "b", 32, 70_000, False), ("item_id", "item_id", 16, 9000, False), ("last_click", "item_id", 16, 9000, False),
        ("tiny", "tiny", 32, 2, False), ("cat", "cat", 16, 50, True)]
NAMES = sorted({t for _, t, _, _, _ in SPEC})
REP = {t for _, t, _, _, r in SPEC if r}
WIDTH = sum(d for _, _, d, _, _ in SPEC)


def _full_tables():
    gen = torch.Generator().manual_seed(23)
    tabs = {}
    for _, t, d, r, _ in SPEC:
        if t not in tabs:
            tabs[t] = torch.randn(r, d, generator=gen).to(torch.bfloat16)
            tabs[t][0] = 0
    return tabs


def _ids(rank, it):
    rng = np.random.default_rng([700, rank, it])
    ids = []
    for _, t, d, r, _ in SPEC:
        x = rng.integers(0, r, B)
        x[:4] = 0                                         # padding ids on every rank
        if r > 1000:
            x[rng.random(B) < 0.05] = 17                  # a hot row, looked up by every rank
        ids.append(x)
    return ids


def _g_out(rank):
    return np.random.default_rng(800 + rank).standard_normal((B, WIDTH)).astype(np.float32)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _worker(rank, world, port, q, one_sided, direct_grad):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import _poison
    _poison.poison()
    try:
        full = _full_tables()
        a16 = {t: full[t].to(DEV) if t in REP else shard_step.make_arena(*full[t].shape, rank, world, DEV, full=full[t].to(DEV), dtype=torch.bfloat16)
               for t in NAMES}
        assert a16["tiny"].shape[0] == 1 + (1 if rank < 2 else 0)
        feats = [ShardedFeature(nm, NRX_SPARSE, t, d, 0, False, False, rep) for nm, t, d, _, rep in SPEC]
        inputs = [torch.from_numpy(x).to(DEV) for x in _ids(rank, 1)]
        g_out = torch.from_numpy(_g_out(rank)).to(DEV)
        eng = RowShardedEmbedding(rank, world, slack=0.5, host_staged=True, overflow_policy="defer")
        step = shard_step.PreparedShardedStep(eng, feats, inputs, [None] * len(feats), a16, one_sided=one_sided, replicated_grads=True)
        step.bind_backward(g_out, None, direct_grad=direct_grad)
        assert step.bf16
        assert all(g["placed"] == one_sided for g in step.groups) and all(b["direct"] == direct_grad for b in step.bwd)
        maps = [(1, 0) if t in REP else shard_step.arena_row_map(rank, world) for t in NAMES]
        p16 = [a16[t] for t in NAMES]
        p32 = [torch.empty(a.shape, dtype=torch.float32, device=DEV) for a in p16]
        s16, s32 = ops.SparseGradSink(), ops.SparseGradSink()
        o16 = FusedSparseAdam(s16, lr=LR, params=p16, sr_seed=SR_SEED, weight_decay=0.01, row_maps=maps)
        o32 = FusedSparseAdam(s32, lr=LR, params=p32, weight_decay=0.01)
        for p in p32:
            o32._register(p)
        twin = {id(a): b for a, b in zip(p16, p32)}
        rep_bits, outs, local_hash_differs = [], [], False
        for it in range(1, STEPS + 1):
            for x, new in zip(inputs, _ids(rank, it)):
                x.copy_(torch.from_numpy(new))
            out, _, _ = step.run()
            entries = step.backward()
            torch.cuda.synchronize()
            dist.barrier()                                # (one-sided: every peer's placing launch has finished before anyone reads its buffer)
            outs.append(out.cpu().numpy().copy())
            for a, b in zip(p16, p32):
                b.copy_(a.float())
            before = [_bits(a) for a in p16]
            keyed = [set() for _ in NAMES]
            for e in entries:
                for k in e["uniq"][:int(e["counts"][0])].cpu().numpy():
                    if k & MASK:
                        keyed[next(i for i, a in enumerate(p16) if a is e["tables"][k >> 40])].add(int(k & MASK))
            s16.pending.extend(entries)
            s32.pending.extend([dict(e, tables=[twin[id(t)] for t in e["tables"]], uniq=e["uniq"].clone(), values=e["values"].clone()) for e in entries])
            o16.step()
            o32.step()
            torch.cuda.synchronize()
            for k, t in enumerate(NAMES):
                (m16, v16), (m32, v32) = o16.moments[k], o32.moments[k]
                assert torch.equal(m16, m32) and torch.equal(v16, v32), (it, t)
                got = _bits(p16[k])
                rows = np.array(sorted(keyed[k]), dtype=np.int64)
                rest = np.ones(got.shape[0], bool)
                rest[rows] = False
                assert np.array_equal(got[rest], before[k][rest]) and not got[0].any(), (it, t)
                if not rows.size:
                    continue
                w32 = p32[k][torch.from_numpy(rows).to(DEV)].cpu().numpy()
                mul, add = maps[k]
                cols = np.arange(got.shape[1])
                assert SR.matches(got[rows], SR.sr_round(w32, SR.sr_bits(SR_SEED, it, k, rows * mul + add, cols))), \
                    f"step {it}: {t}: bf16 patterns != the restatement with the global rows"
                if t not in REP:
                    local_hash_differs |= not np.array_equal(got[rows], SR.sr_round(w32, SR.sr_bits(SR_SEED, it, k, rows, cols)))
            rep_bits.append({t: _bits(a16[t]) for t in REP})
            dist.barrier()
        assert not step.overflowed()
        arenas = {t: _bits(a16[t]) for t in NAMES if t not in REP}
        moms = {t: tuple(m.contiguous().cpu().numpy() for m in o16.moments[k]) for k, t in enumerate(NAMES) if t not in REP}
        q.put((rank, outs, rep_bits, arenas, moms, bool(local_hash_differs)))
        dist.barrier()                                    # nobody unmaps a buffer a peer may still be writing
    except Exception as e:                                # (the parent fails at once instead of waiting for a result that will not come)
        import traceback
        q.put((rank, f"{type(e).__name__}: {e} {traceback.format_exc()}"[:3000]))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("one_sided,direct_grad", [(False, False), (True, True)])
def test_union_of_the_arenas_is_the_unsharded_bf16_model(world, one_sided, direct_grad):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, one_sided, direct_grad)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        item = q.get(timeout=300)
        assert not isinstance(item[1], str), f"rank {item[0]}: {item[1]}"
        res[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    # ---- the unsharded bf16 model on the rank-major concatenation: the direct path + FusedSparseAdam, same sr_seed
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
    opt = FusedSparseAdam(sink, lr=LR, params=u16, sr_seed=SR_SEED, weight_decay=0.01)
    routed_cols = [c for sl, (_, t, _, _, rep) in zip(slots, SPEC) if not rep for c in range(sl.out_col, sl.out_col + sl.dim)]
    for it in range(1, STEPS + 1):
        for k, x in enumerate(inputs):
            x.copy_(torch.from_numpy(np.concatenate([_ids(r, it)[k] for r in range(world)])))
        d_out = fwd.run()[0].cpu().numpy()
        for r in range(world):        # the forward of every step: the routed tables' columns are the unsharded model's rows
            assert np.array_equal(res[r][0][it - 1][:, routed_cols].view(np.int32), d_out[r * B:(r + 1) * B][:, routed_cols].view(np.int32)), (it, r)
        sink.pending.extend([dict(tables=u16, dim=g["dim"], uniq=g["uniq"], values=g["values"], counts=g["counts"], cap=g["cap"]) for g in bwd.run()])
        opt.step()
        torch.cuda.synchronize()
        for t in REP:                 # replicated tables: the same bits on every rank after every step
            for r in range(1, world):
                assert np.array_equal(res[r][1][it - 1][t], res[0][1][it - 1][t]), (it, t, r)
    assert any(res[r][4] for r in range(world)), "the restatement with the arenas' LOCAL rows matched too: the test cannot see the row map"
    for k, t in enumerate(NAMES):
        if t in REP:
            continue
        rows, D = full[t].shape
        got = np.zeros((rows, D), np.uint16)
        gm, gv = np.zeros((rows, D), np.float32), np.zeros((rows, D), np.float32)
        for r in range(world):
            a = res[r][2][t]
            assert a.shape[0] == 1 + len(range(r, rows, world)) and not a[0].any()
            got[r::world] = a[1:]
            gm[r::world], gv[r::world] = res[r][3][t][0][1:], res[r][3][t][1][1:]
        want = u16[k].view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), f"{t}: the union of the arenas != the unsharded bf16 table"
        assert (got != full[t].view(torch.int16).numpy().view(np.uint16)).any() or rows <= 2, f"{t}: nothing trained"
        mu, vu = opt.moments[k]
        assert np.array_equal(gm.view(np.int32), mu.contiguous().cpu().numpy().view(np.int32)), f"{t}: exp_avg"
        assert np.array_equal(gv.view(np.int32), vu.contiguous().cpu().numpy().view(np.int32)), f"{t}: exp_avg_sq"


# ---------------------------------------------------------------------------------------------- the converted model at world 2
def _model_worker(rank, world, port, q, cfg_path):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import _poison
    _poison.poison()
    try:
        from news_recsys_amd import sharding
        from news_recsys_amd.model.sort.fm.model import FM
        from tests.test_bf16_tables_gpu import make_batch

        def pack(sd):
            return {k: (v.view(torch.int16) if v.dtype is torch.bfloat16 else v).detach().cpu().numpy() for k, v in sd.items()}

        torch.manual_seed(3)                              # (the same initial model on every rank)
        m = FM(cfg_path).to(DEV)
        init = {k: v.clone() for k, v in m.state_dict().items()}
        batches = [make_batch(m, 256, torch.Generator(device=DEV).manual_seed(100 * it + rank)) for it in range(2)]
        kw = dict(host_staged=True, bf16_tables=True, replicate=("category",), slack=1.0)
        shard_step.shard_model_step_(m, rank, world, **kw)
        full0 = sharding.full_state_dict(m)              # gather-on-save: the bf16 bit patterns through gloo
        assert sorted(full0) == sorted(init)
        for k, v in init.items():
            assert full0[k].dtype is v.dtype and full0[k].shape == v.shape, k
            assert np.array_equal(pack({k: full0[k]})[k], pack({k: v})[k]), f"{k}: gather-on-save changed the table"
        opt = m.configure_optimizers()["optimizer"]
        assert opt._sparse.row_maps == [(1, 0) if n in m._replicated_tables else shard_step.arena_row_map(rank, world) for n in m.embedding_tables]
        for b in batches:
            opt.zero_grad()
            m.bceLoss(m(b), b["label"][:, 0]).backward()
            grads = [p.grad for p in sharding.data_parallel_params(m) if p.grad is not None]
            flat = torch.cat([x.reshape(-1) for x in grads]).cpu()
            dist.all_reduce(flat)
            flat /= world
            off = 0
            for x in grads:
                x.copy_(flat[off:off + x.numel()].view_as(x))
                off += x.numel()
            opt.step()
        shard_step.check_shard_steps(m)
        torch.cuda.synchronize()
        full2 = sharding.full_state_dict(m)
        torch.manual_seed(50 + rank)
        again = FM(cfg_path).to(DEV)
        shard_step.shard_model_step_(again, rank, world, **kw)
        sharding.load_full_state_dict_(again, full2)      # scatter-on-load of the full bf16 tables
        back = pack(sharding.full_state_dict(again))
        for k, v in pack(full2).items():
            assert np.array_equal(back[k], v), f"{k}: scatter-on-load + gather-on-save is not the identity"
        for n, e in again.embedding_tables.items():
            assert torch.equal(e.weight.view(torch.int16), m.embedding_tables[n].weight.view(torch.int16)), n
        q.put((rank, pack(init), pack(full2), [str(v.dtype) for v in full2.values()]))
        dist.barrier()
    except Exception as e:                                # (the parent fails at once instead of waiting for a result that will not come)
        import traceback
        q.put((rank, f"{type(e).__name__}: {e} {traceback.format_exc()}"[:3000], None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_converted_bf16_model_at_world_2_saves_and_loads_full_bf16_tables(tmp_path):
    """shard_model_step_(bf16_tables=True) over gloo (host-staged), one table replicated: gather-on-save right after the conversion returns the
    initial bf16 tables bit for bit; after two training steps both ranks gather the same full state (bf16 tables under the unsharded keys,
    trained); scatter-on-load of it into a freshly converted model reproduces every arena."""
    from tests.test_bf16_tables_gpu import write_cfg
    world = 2
    cfg = write_cfg(tmp_path, "cf_fm_small.yaml", table_dtype="bf16", sparse_grad="fused", sr_seed=9)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_model_worker, args=(r, world, port, q, cfg)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        item = q.get(timeout=300)
        assert not isinstance(item[1], str), f"rank {item[0]}: {item[1]}"
        res[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    init, full, dts = res[0]
    assert any(d == "torch.bfloat16" for d in dts)
    for k, v in full.items():
        assert np.array_equal(v, res[1][1][k]), f"{k}: the ranks gathered different states"
    moved = [k for k in full if k.startswith("embedding_tables.") and not np.array_equal(full[k], init[k])]
    assert moved, "no table trained"
