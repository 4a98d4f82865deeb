"""The replicated tables' gradient exchange of the bound sharded step (shard_step.PreparedShardedStep(replicated_grads=True),
csrc/nrx_replicated.hip) without a GPU:

  * the replication planner of shard_step_model_ (shard_step.replicated_table_names): tables by name, by a feature name (the features that share
    its table follow it), by size threshold; the defaults replicate nothing;
  * the exchange PROTOCOL over real rank processes (gloo, world 2 and 3) with numpy stand-ins for the three kernels -- the definitions the HIP
    kernels are checked against bit for bit on the GPU (tests/test_replicated_grads_gpu.py): pack every local (keys, values) list into the
    dense chunked buffer (shard_step.replicated_layout), equal-split all-to-all, the rank-order sum of a chunk, all-gather, compaction per dim.
    Mixed dims, a table count that does not divide into the chunks, rows no rank touched: every rank ends with the same keys and bits, equal to
    the rank-order fold s = G_0; s = s + G_1; ... of the ranks' dense local gradients over the union of their keys.
No reference counterpart (the reference is single-device: src/model/sort/deep/train.py:38-44)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from news_recsys_amd.shard_step import replicated_layout, replicated_table_names
from tests.test_sharding_gloo import _free_port

MASK = (1 << 40) - 1


# ------------------------------------------------------------------ numpy definitions of the three kernels
def np_pack(lists, lay_t, world, cf, cr):
    """lists: [(keys int64 [n], values float32 [n, dim])]; lay_t: per key table (voff, roff, rows, dim).  The buffer [world * C] as float32 words
    (touch counts stored as int32 bit patterns)."""
    C = cf + cr
    buf = np.zeros(world * C, np.float32)
    words = buf.view(np.int32)
    for keys, vals in lists:
        for k, key in enumerate(keys):
            voff, roff, rows, dim = lay_t[key >> 40]
            row = key & MASK
            assert row < rows and vals.shape[1] == dim
            i = voff + row * dim + np.arange(dim)
            buf[(i // cf) * C + i % cf] = vals[k]
            j = roff + row
            words[(j // cr) * C + cf + j % cr] = 1
    return buf


def np_ordered_sum(recv, world, cf, cr):
    """recv [world * C] -> [C]: floats added in rank order (float32 each step), counts as int32."""
    C = cf + cr
    r = recv.reshape(world, C)
    out = r[0].copy()
    for q in range(1, world):
        out[:cf] = (out[:cf] + r[q, :cf]).astype(np.float32)
    out.view(np.int32)[cf:] = r[:, cf:].view(np.int32).sum(0, dtype=np.int64).astype(np.int32)
    return out


def np_compact(full, world, cf, cr, tabs):
    """tabs: [(key table, voff, roff, rows, dim)] in key order -> (keys, values) of the rows whose count > 0, row order."""
    C = cf + cr
    words = full.view(np.int32)
    keys, vals = [], []
    for kt, voff, roff, rows, dim in tabs:
        for row in range(rows):
            j = roff + row
            if words[(j // cr) * C + cf + j % cr] > 0:
                i = voff + row * dim + np.arange(dim)
                keys.append((kt << 40) | row)
                vals.append(full[(i // cf) * C + i % cf])
    dim = tabs[0][4]
    return np.array(keys, np.int64), (np.stack(vals).astype(np.float32) if vals else np.zeros((0, dim), np.float32))


def dim_groups(dims):
    """Table indices grouped by embedding dim (first appearance), as PreparedShardedStep lays them out."""
    out = {}
    for t, d in enumerate(dims):
        out.setdefault(d, []).append(t)
    return list(out.values())


def layout_of(rows, dims, world):
    groups = dim_groups(dims)
    order = [t for g in groups for t in g]
    lay = replicated_layout([(rows[t], dims[t]) for t in order], world)
    at = {t: k for k, t in enumerate(order)}
    per_t = {t: (lay["voff"][at[t]], lay["roff"][at[t]], rows[t], dims[t]) for t in range(len(rows))}
    return lay, groups, per_t


def local_lists(rank, rows, dims, groups, touch=0.4):
    """Rank `rank`'s local (keys, values) per dim group: a random subset of rows (row 2 of every table: never), random values."""
    rng = np.random.default_rng(900 + rank)
    out = []
    for g in groups:
        keys, vals = [], []
        for t in g:
            sel = np.flatnonzero(rng.random(rows[t]) < touch)
            sel = sel[sel != 2]
            keys += [(t << 40) | int(r) for r in sel]
            vals.append(rng.standard_normal((len(sel), dims[t])).astype(np.float32))
        out.append((np.array(keys, np.int64), np.concatenate(vals) if vals else np.zeros((0, dims[g[0]]), np.float32)))
    return out


def fold(world, rows, dims, groups, touch=0.4):
    """The contract: per dim group, keys = the union of the ranks' keys (sorted), values = the rank-order float32 fold of the dense G_r."""
    res = []
    for gi, g in enumerate(groups):
        dense = {t: np.zeros((rows[t], dims[t]), np.float32) for t in g}
        hit = {t: np.zeros(rows[t], bool) for t in g}
        for r in range(world):
            G = {t: np.zeros((rows[t], dims[t]), np.float32) for t in g}
            keys, vals = local_lists(r, rows, dims, groups, touch)[gi]
            for k, v in zip(keys, vals):
                G[k >> 40][k & MASK] = v
                hit[k >> 40][k & MASK] = True
            for t in g:
                dense[t] = G[t].copy() if r == 0 else (dense[t] + G[t]).astype(np.float32)
        keys = [(t << 40) | int(r_) for t in g for r_ in np.flatnonzero(hit[t])]
        vals = [dense[t][r_] for t in g for r_ in np.flatnonzero(hit[t])]
        res.append((np.array(keys, np.int64), np.stack(vals) if vals else np.zeros((0, dims[g[0]]), np.float32)))
    return res


ROWS = [18, 270, 18, 5, 41, 1]
DIMS = [8, 8, 8, 3, 5, 3]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lay, groups, per_t = layout_of(ROWS, DIMS, world)
        cf, cr, C = lay["cf"], lay["cr"], lay["C"]
        send = np_pack(local_lists(rank, ROWS, DIMS, groups), per_t, world, cf, cr)
        recv = torch.empty(world * C, dtype=torch.float32)
        dist.all_to_all_single(recv, torch.from_numpy(send))                  # equal splits: chunk q of every rank to rank q
        red = np_ordered_sum(recv.numpy(), world, cf, cr)
        full = torch.empty(world * C, dtype=torch.float32)
        dist.all_gather(list(full.view(world, C).unbind(0)), torch.from_numpy(red))
        got = [np_compact(full.numpy(), world, cf, cr, [(t,) + per_t[t][:2] + (ROWS[t], DIMS[t]) for t in g]) for g in groups]
        q.put((rank, [(k.tolist(), v.view(np.int32).tolist()) for k, v in got]))
    except Exception as e:      # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_replicated_exchange_protocol_gives_every_rank_the_rank_order_fold(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(res[r], str), res[r]
    lay, groups, _ = layout_of(ROWS, DIMS, world)
    # (chunks by words: a chunk boundary falls inside some table's rows, so rows are split between two reducing ranks)
    spans = [(lay["voff"][k], lay["voff"][k] + ROWS[t] * DIMS[t]) for k, t in enumerate(t for g in groups for t in g)]
    assert any(lo < q * lay["cf"] < hi for q in range(1, world) for lo, hi in spans)
    want = fold(world, ROWS, DIMS, groups)
    for r in range(world):
        assert res[r] == res[0]                      # same keys, same bits on every rank
    for (k, v), (wk, wv) in zip(res[0], want):
        assert k == wk.tolist()
        assert v == wv.view(np.int32).tolist()
    # rows no rank touched (row 2 of every table) carry no key
    assert all(((np.array(k, np.int64) & MASK) != 2).all() for k, _ in res[0])


def test_layout_chunks_cover_every_table():
    for world in (1, 2, 3, 8):
        lay = replicated_layout([(r, d) for r, d in zip(ROWS, DIMS)], world)
        assert lay["cf"] % 4 == 0 and lay["cr"] % 4 == 0
        assert world * lay["cf"] >= sum(r * d for r, d in zip(ROWS, DIMS)) and world * lay["cr"] >= sum(ROWS)


# ------------------------------------------------------------------ the planner
def _model(cfg):
    from news_recsys_amd.model.sort.widedeep.model import WideDeep
    from news_recsys_amd.model.sort.deep.model import Deep
    from tests.conftest import CONFIGS
    return (WideDeep if "widedeep" in cfg else Deep)(os.path.join(CONFIGS, cfg))


def test_planner_defaults_replicate_nothing():
    m = _model("cf_widedeep_small.yaml")
    assert replicated_table_names(m) == []


def test_planner_by_name_and_by_threshold():
    m = _model("cf_widedeep_small.yaml")
    assert replicated_table_names(m, replicate=("category", "subcategory")) == [n for n in m.embedding_tables if n in ("category", "subcategory")]
    # 18 * 17 * 4 = 1224 bytes (category, user_click_category); 27 * 17 * 4 = 1836 (subcategory); 61 * 32 * 4 = 7808 (item_id)
    assert sorted(replicated_table_names(m, replicate_below_bytes=1224)) == ["category", "user_click_category"]
    assert sorted(replicated_table_names(m, replicate_below_bytes=1836)) == ["category", "subcategory", "user_click_category"]
    assert sorted(replicated_table_names(m, replicate=("item_id",), replicate_below_bytes=1224)) == ["category", "item_id", "user_click_category"]
    with pytest.raises(ValueError):
        replicated_table_names(m, replicate=("no_such_table",))


def test_planner_features_that_share_a_table_follow_it():
    """cf_array_small: user_history (the history bag) reads item_id's table -- naming the feature replicates the shared table."""
    m = _model("cf_array_small.yaml")
    shared = m._get_emb_feature_name("user_history")
    assert shared != "user_history" and shared in m.embedding_tables
    assert replicated_table_names(m, replicate=("user_history",)) == [shared]
