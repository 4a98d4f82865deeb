"""The bound sharded training step (shard_step.PreparedShardedStep) at the FULL baseline sizes bench.py times, against float64 and the direct path.

World 1: the path bench builds (sharding.ShardedBenchPath(wl, dev, seed, 0, 1, 65536, "row") + train_setup(), engine "feat") on the real C2 / C3 /
C4 / C5 tables -- arena element offsets past 2^31 (C3's 100 M x 64 item table, C5's 500 M x 32 one), owner ids near 5e8, C4's 3.3 M-entry
history channel.  One bound step runs uniform -> Zipf(1.05) -> uniform id sets (refilled in place, so the planners' choice follows the previous
batch), each twice; every call is checked:
  * single-valued concat columns == table[ids] and == the direct bound path (PreparedEmbed over the same tables): bit for bit;
  * C4's pooled history columns vs the float64 masked mean (rel 1e-6), all-empty bags exact zeros; C2's FM logit vs float64 (rtol 2e-5) and vs
    the direct path (1e-5: the pass over the finished concat sums in another order);
  * the row-sparse gradient (keys, values) == the direct PreparedSparseBackward bit for bit (keys shifted by the dummy row; C2 with the FM term
    folded in) -- C4 to the per-row bound (the pooled channel sums in another order) -- and every gradient vs a float64 restatement of the
    definition within |v - ref| <= 2e-6 * mass + 1e-6 per row, on exactly the same support (padding row never keyed, every row once per list);
  * no overflow, the same bits twice; C2: the captured-graph replay bench performs leaves the eager keys and values; C2 / C4: two FusedSparseAdam
    steps on the arenas == the same steps on clones of the direct tables (rows not looked up keep their bits, dummy and padding rows stay zero).
World 2 (two rank processes sharing cuda:0 over gloo, host-staged): C2's 26 tables x 1 M rows at B = 32 768 per rank, buffered and default forms,
uniform and Zipf ids; and a block that really overflows through nrx_route_feat.
No reference counterpart (the reference is single-device, src/model/sort/deep/train.py:38-44); the arithmetic is autograd of
src/model/BaseModel/base_model.py:262-308 and the FM logit of src/model/sort/fm/model.py:18-26."""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from news_recsys_amd import ops, shard_step
from news_recsys_amd._lib import NRX_SPARSE
from tests.test_full_size_baseline_shapes import need_free
from tests.test_sharding_gloo import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 65536
ROW = (1 << 40) - 1
FULL_BYTES = {"c2": 26 * 1_000_000 * 16 * 4, "c3": (100_000_000 + 1_000_000 + 306) * 64 * 4,
              "c4": (10_000_000 + 200_000) * 16 * 4, "c5": sum(int(round(1e3 * (5e5) ** (i / 39))) for i in range(40)) * 32 * 4}


# ---------------------------------------------------------------------------------------------- id sets
def _zipf(rng, rows, shape):
    """Zipf(1.05) ranks scattered over the table by a multiplicative hash: the hot rows are real rows (never the padding row) spread over it."""
    z = np.minimum(rng.zipf(1.05, shape), rows - 1).astype(np.int64) - 1
    return 1 + (z * 2654435761) % (rows - 1)


def _fill(path, ins, ws, orig, kind, rng):
    """Refill the bound step's id (and mask) tensors in place: the pool's own ids ("uniform") or Zipf ids, padding and last rows at fixed
    positions, histories padded like DataReader's (random lengths 0..L, id 0 and mask 0 past the length, an all-empty bag)."""
    for f, x, w, o in zip(path.feats, ins, ws, orig):
        rows = path.rows[f.name]
        ids = o.clone() if kind == "uniform" else torch.from_numpy(_zipf(rng, rows, tuple(x.shape))).to(DEV)
        if f.bag_len:
            L = f.bag_len
            lens = torch.from_numpy(rng.integers(0, L + 1, x.shape[0])).to(DEV)
            lens[0], lens[1], lens[2] = L, 0, 1
            m = (torch.arange(L, device=DEV)[None] < lens[:, None]).float()
            ids[0, 0], ids[0, L - 1], ids[2, 0] = rows - 1, rows - 1, 1
            ids = ids * m.long()
            w.copy_(m)
        else:
            flat = ids.view(-1)
            flat[0], flat[1], flat[2] = 0, rows - 1, rows - 1          # padding, last row (largest offset), a duplicate of it
            big = (1 << 31) // f.dim                                    # the first row whose element offset is 2^31
            if big < rows:
                flat[3] = big
        x.copy_(ids)


# ---------------------------------------------------------------------------------------------- references
def _direct(path, ins, ws, tables=None):
    """The direct (unsharded) bound path over path.tables (= the arenas without their dummy row: the same memory; or `tables`) and the same id
    tensors."""
    tables = path.tables if tables is None else tables
    names = sorted(tables)
    slots, col = [], 0
    for f in path.feats:
        slots.append(ops.Slot(f.name, f.kind, names.index(f.table), f.dim, f.bag_len, col, fm_field=int(path.fm)))
        col += f.dim
    plan = ops.EmbedPlan(slots, out_width=col, use_fm=path.fm)
    sums = torch.empty((B, path.feats[0].dim), dtype=torch.float32, device=DEV) if path.fm else None
    fwd = ops.PreparedEmbed(plan, [tables[t] for t in names], ins, [w if f.bag_len else None for f, w in zip(path.feats, ws)], fm_sums=sums)
    return fwd, ops.PreparedSparseBackward(fwd, path._g_out, path._g_fm), names


def _bag_weights(m):
    return m.double() / (m.double().sum(1, keepdim=True) + 1e-8)


def _fm_rows64(path, ins):
    return torch.stack([path.tables[f.table][x].double() for f, x in zip(path.feats, ins)], 1)          # [B, F, D]


def _fm_grad64(v, g_fm):
    """d(FM logit)/d(field rows) times g_fm in float64 ([B, F, D]: column 0 -> 1, columns k >= 1 -> sum_f v[f, k] - v[f, k]), and the L1 mass
    the fp32 form of it is rounded against (the field sum is formed from sum_f |v[f, k]|)."""
    g = g_fm.double()[:, None, None]
    s, sa = v.sum(1, keepdim=True), v.abs().sum(1, keepdim=True)
    one = torch.ones_like(v[:, :, :1])
    return g * torch.cat([one, s[:, :, 1:] - v[:, :, 1:]], 2), g.abs() * torch.cat([one, sa[:, :, 1:] + v[:, :, 1:].abs()], 2)


def _reference_grad(path, ins, ws, cols, names):
    """float64 restatement of the tables' gradient, compact: (sorted global keys name << 40 | row, values [n, D], L1 mass [n, D]).  Padding
    lookups (id 0) never train."""
    g = path._g_out.double()
    fm_term = fm_mass = None
    if path.fm:
        fm_term, fm_mass = _fm_grad64(_fm_rows64(path, ins), path._g_fm)
    keys, vals, mass = [], [], []
    for t in names:
        parts = []
        for i, (f, x, w) in enumerate(zip(path.feats, ins, ws)):
            if f.table != t:
                continue
            D, c = f.dim, cols[i]
            if f.bag_len:
                c_rows = (_bag_weights(w)[..., None] * g[:, None, c:c + D]).reshape(-1, D)
                m_rows = c_rows.abs()
            elif fm_term is not None:
                c_rows = g[:, c:c + D] + fm_term[:, i]
                m_rows = g[:, c:c + D].abs() + fm_mass[:, i]
            else:
                c_rows = g[:, c:c + D]
                m_rows = c_rows.abs()
            parts.append((x.reshape(-1), c_rows, m_rows))
        ids = torch.cat([p[0] for p in parts])
        rows = torch.cat([p[1] for p in parts])
        m_rows = torch.cat([p[2] for p in parts])
        live = ids != 0
        uniq, inv = torch.unique(ids[live], return_inverse=True)
        keys.append((names.index(t) << 40) | uniq)
        vals.append(torch.zeros((uniq.numel(), rows.shape[1]), dtype=torch.float64, device=DEV).index_add_(0, inv, rows[live]))
        mass.append(torch.zeros((uniq.numel(), rows.shape[1]), dtype=torch.float64, device=DEV).index_add_(0, inv, m_rows[live]))
        del ids, rows, m_rows, live, inv
    return torch.cat(keys), torch.cat(vals), torch.cat(mass)


def _global_lists(entries, name_of, names, world=1, rank=0):
    """The sharded step's (keys, values) lists in global terms: [(keys name << 40 | global row, values)] per list.  Checks on the way: every row
    once per list, the arenas' dummy row carries zeros, the global padding row is never keyed."""
    out = []
    for e in entries:
        nu = int(e["counts"][0])
        k, v = e["uniq"][:nu], e["values"][:nu]
        assert torch.unique(k).numel() == nu
        lut = torch.tensor([names.index(name_of[t.data_ptr()]) for t in e["tables"]], dtype=torch.int64, device=DEV)
        row = k & ROW
        dummy = row == 0
        assert not bool(v[dummy].any())
        grow = (row[~dummy] - 1) * world + rank
        assert not bool((grow == 0).any())
        out.append(((lut[k[~dummy] >> 40] << 40) | grow, v[~dummy]))
    return out


def _direct_lists(groups, world=1, rank=None):
    """The direct path's lists in the same terms (its padding row's entry dropped; rank: keep only the rows that rank owns)."""
    out = []
    for gr in groups:
        nu = int(gr["counts"][0])
        k, v = gr["uniq"][:nu], gr["values"][:nu]
        keep = (k & ROW) != 0
        if rank is not None:
            keep &= (k & ROW) % world == rank
        out.append((k[keep], v[keep]))
    return out


def _merge(lists):
    """Sum of the lists per key in float64: (sorted keys, values)."""
    k = torch.cat([x[0] for x in lists])
    v = torch.cat([x[1] for x in lists]).double()
    uniq, inv = torch.unique(k, return_inverse=True)
    return uniq, torch.zeros((uniq.numel(), v.shape[1]), dtype=torch.float64, device=k.device).index_add_(0, inv, v)


def _sorted_cat(lists):
    k = torch.cat([x[0] for x in lists])
    v = torch.cat([x[1] for x in lists])
    o = torch.argsort(k)
    return k[o], v[o]


def _snapshot(entries):
    return [(e["uniq"][:int(e["counts"][0])].clone(), e["values"][:int(e["counts"][0])].clone()) for e in entries]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(ka, kb) and torch.equal(va.view(torch.int32), vb.view(torch.int32)) for (ka, va), (kb, vb) in zip(a, b))


# ---------------------------------------------------------------------------------------------- world 1, the bench path
def _check_call(path, step, direct, ins, ws, cols, names, name_of, exact_grad):
    fwd, bwd, _ = direct
    out, _, fmv = step.run()
    entries = step.backward()
    d_out, _, d_fm = fwd.run()
    d_groups = bwd.run()
    torch.cuda.synchronize()
    for i, (f, x, w) in enumerate(zip(path.feats, ins, ws)):
        c, D = cols[i], f.dim
        got = out[:, c:c + D]
        if f.bag_len:
            rows = path.tables[f.table][x].double()                                       # [B, L, D]
            ref = (rows * w.double()[..., None]).sum(1) / (w.double().sum(1, keepdim=True) + 1e-8)
            del rows
            empty = w.sum(1) == 0
            assert bool(empty.any()) and bool((got[empty] == 0).all())                      # all-empty bags: exact zeros
            rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
            assert rel < 1e-6, f"{f.name}: pooled rel {rel}"
            torch.testing.assert_close(got, d_out[:, c:c + D], rtol=1e-6, atol=1e-6)
        else:
            assert torch.equal(got, path.tables[f.table][x]), f.name                       # the definition: torch indexing
            assert torch.equal(got, d_out[:, c:c + D]), f.name                              # the direct bound path
    if path.fm:
        v = _fm_rows64(path, ins)
        fm64 = v[:, :, 0].sum(1) + 0.5 * (v[:, :, 1:].sum(1).pow(2) - v[:, :, 1:].pow(2).sum(1)).sum(1)
        # (bench's tables are N(0, 1): the logit is a difference of terms ~ 20x its size -- rtol 2e-5 of the terms it is formed from)
        mass = v[:, :, 0].abs().sum(1) + 0.5 * (v[:, :, 1:].sum(1).pow(2) + v[:, :, 1:].pow(2).sum(1)).sum(1)
        del v
        assert bool(((fmv.double() - fm64).abs() <= 2e-5 * mass + 2e-5).all())
        torch.testing.assert_close(fmv, d_fm, rtol=1e-5, atol=1e-5 * float(d_fm.abs().max()))
    # gradients: the direct path, then float64
    lists = _global_lists(entries, name_of, names)
    d_lists = _direct_lists(d_groups)
    r_keys, r_vals, r_mass = _reference_grad(path, ins, ws, cols, names)
    tol = 2e-6 * r_mass + 1e-6
    if exact_grad:
        sk, sv = _sorted_cat(lists)
        dk, dv = _sorted_cat(d_lists)
        assert torch.equal(sk, dk)
        assert torch.equal(sv.view(torch.int32), dv.view(torch.int32))
        mk, mv = sk, sv.double()
    else:
        mk, mv = _merge(lists)
        dk, dv = _merge(d_lists)
        assert torch.equal(mk, dk)
        assert bool(((mv - dv).abs() <= tol).all())
    assert torch.equal(mk, r_keys)                                                           # exactly the looked-up rows
    assert bool(((mv - r_vals).abs() <= tol).all())
    res = (out.clone(), None if fmv is None else fmv.clone(), _snapshot(entries))
    del r_keys, r_vals, r_mass, tol, mk, mv, dk, dv
    return res


def _optimizer_steps(path, step, ins, ws, names, exact):
    """Two FusedSparseAdam steps on the arenas vs the same on clones of the direct tables."""
    from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
    before = {t: path.tables[t].clone() for t in names}
    full = {t: path.tables[t].clone() for t in names}
    fwd, bwd, _ = _direct(path, ins, ws, full)
    sink_a, sink_b = ops.SparseGradSink(), ops.SparseGradSink()
    # (eps 1e-3: Adam's first step is ~ lr * g / |g|, whose slope at |g| ~ eps would turn C4's last-place gradient differences into large ones)
    opt_a, opt_b = FusedSparseAdam(sink_a, lr=0.01, eps=1e-3), FusedSparseAdam(sink_b, lr=0.01, eps=1e-3)
    for _ in range(2):
        step.run()
        step.sink_entries(sink_a)
        opt_a.step()
        fwd.run()
        for g in bwd.run():
            sink_b.pending.append(dict(tables=[full[n] for n in names], dim=g["dim"], uniq=g["uniq"], values=g["values"], counts=g["counts"], cap=g["cap"]))
        opt_b.step()
    torch.cuda.synchronize()
    for t in names:
        touched = torch.zeros(path.tables[t].shape[0], dtype=torch.bool, device=DEV)
        for f, x in zip(path.feats, ins):
            if f.table == t:
                touched[x.reshape(-1)] = True
        got = path.tables[t]
        if exact:
            assert torch.equal(got, full[t]), t
        else:
            torch.testing.assert_close(got, full[t], rtol=1e-5, atol=1e-6, msg=lambda s, t=t: f"{t}: {s}")
        assert torch.equal(got[~touched], before[t][~touched]), t                                    # rows not looked up keep their bits
        assert bool(touched[1:].any()) and not bool((got[touched] == before[t][touched]).all())      # ... and the looked-up ones moved
        a = path.arenas[t]
        assert not bool(a[0].any()) and not bool(a[1].any()), t                                      # dummy row, global padding row
    del before, full


@pytest.mark.parametrize("wl", ["c2", "c3", "c4", "c5"])
def test_world_1_bench_step_at_full_size_against_float64_and_the_direct_path(wl):
    from news_recsys_amd.sharding import ShardedBenchPath
    need_free(FULL_BYTES[wl] * (3 if wl in ("c2", "c4") else 1) + (16 << 30))
    path = None
    try:
        path = ShardedBenchPath(wl, DEV, 1234, 0, 1, B, "row")
        assert path.engine == "feat" and path.train_setup()
        step = path.calls[0]
        ins, ws = path.pool[0]
        orig = [x.clone() for x in ins]
        names = sorted(path.tables)
        name_of = {a.data_ptr(): n for n, a in path.arenas.items()}
        cols = [s.out_col for s in step.plan.slots]
        if wl in ("c3", "c5"):
            assert max(t.numel() for t in path.tables.values()) > 2 ** 31                       # element offsets past 32 bits
        direct = _direct(path, ins, ws)
        policies = [g["policy"] for b in step.bwd if not b["pooled"] for g in b["owner"].groups if g.get("policy") is not None]
        choices = []
        rng = np.random.default_rng({"c2": 2, "c3": 3, "c4": 4, "c5": 5}[wl])
        last = None
        for kind in ("uniform", "zipf", "uniform"):
            _fill(path, ins, ws, orig, kind, rng)
            runs = [_check_call(path, step, direct, ins, ws, cols, names, name_of, exact_grad=wl != "c4")]
            choices.append(tuple(p.use_lds for p in policies))
            out, _, fmv = step.run()                                                              # the same id set again: the same bits
            entries = step.backward()
            torch.cuda.synchronize()
            choices.append(tuple(p.use_lds for p in policies))
            runs.append((out.clone(), None if fmv is None else fmv.clone(), _snapshot(entries)))
            assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
            assert runs[0][1] is None or torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
            assert _same(runs[0][2], runs[1][2])
            assert not path.overflowed()
            last = runs[1]
        if wl == "c2" and any(p.eligible for p in policies):
            assert len(set(choices)) > 1                                                          # the planner changed between calls
        if wl == "c2":
            # bench's captured-graph replay of the bound step (bench.py, sharded_train_leg): the eager keys and values
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out2, _, _ = step.run()
                entries2 = step.backward()
            out2.zero_()
            for e in entries2:
                e["values"].zero_()
                e["counts"].zero_()
            for _ in range(2):
                graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out2.view(torch.int32), last[0].view(torch.int32))
            assert _same(_snapshot(entries2), last[2])
            del graph
        if wl in ("c2", "c4"):                                                                    # (C3 / C5: the moments do not fit next to the tables)
            _optimizer_steps(path, step, ins, ws, names, exact=wl == "c2")
    finally:
        del path
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- world 2, C2's feature count at full size
F2, ROWS2, D2, B2 = 26, 1_000_000, 16, 32768


def _tables2():
    tabs = []
    for t in range(F2):
        x = torch.randn((ROWS2, D2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(700 + t))
        x[0].zero_()
        tabs.append(x)
    return tabs


def _batch2(kind, rank):
    """(ids [F2] int64 numpy arrays, g_out, g_fm) of one rank's batch, rebuilt from seeds on any process."""
    rng = np.random.default_rng(4000 + 10 * rank + {"uniform": 0, "zipf": 1, "overflow": 2}[kind])
    ids = []
    for f in range(F2):
        x = _zipf(rng, ROWS2, B2) if kind == "zipf" else rng.integers(1, ROWS2, B2)
        if kind == "overflow" and f == 3:
            x = 2 * rng.integers(1, ROWS2 // 2, B2)              # every id an even row: all of them owned by rank 0
        x[0], x[1], x[2] = 0, ROWS2 - 1, ROWS2 - 1
        ids.append(x.astype(np.int64))
    gen = torch.Generator(device=DEV).manual_seed(5000 + 10 * rank + len(kind))
    return ids, torch.randn((B2, F2 * D2), device=DEV, generator=gen), torch.randn((B2,), device=DEV, generator=gen)


def _slack_for(batches, world):
    """The smallest slack whose blocks hold the draw's largest (source, owner, feature) count (numpy): no block overflows."""
    worst = max(int(np.bincount(x % world, minlength=world).max()) for ids, _, _ in batches for x in ids)
    return max(0.0, worst * world / B2 - 1.0) + 1e-3


def _world2_compare(step, tabs, batches, rank, world, fm_exact):
    """One bound call of `step` (its id tensors hold batches[rank]) against the direct path and float64 on the rank-major concatenation:
    booleans only."""
    out, _, fmv = step.run()
    entries = step.backward()
    torch.cuda.synchronize()
    dist.barrier()
    res = {}
    ins = [torch.from_numpy(np.concatenate([b[0][f] for b in batches])).to(DEV) for f in range(F2)]
    g_out = torch.cat([b[1] for b in batches])
    g_fm = torch.cat([b[2] for b in batches])
    names = [f"C{i:02d}" for i in range(F2)]
    plan = ops.EmbedPlan([ops.Slot(n, NRX_SPARSE, i, D2, 0, i * D2, fm_field=1) for i, n in enumerate(names)], out_width=F2 * D2, use_fm=True)
    sums = torch.empty((world * B2, D2), dtype=torch.float32, device=DEV)
    fwd = ops.PreparedEmbed(plan, tabs, ins, [None] * F2, fm_sums=sums)
    d_out, _, d_fm = fwd.run()
    d_groups = ops.PreparedSparseBackward(fwd, g_out, g_fm).run()
    torch.cuda.synchronize()
    mine = slice(rank * B2, (rank + 1) * B2)
    res["out"] = torch.equal(out, d_out[mine])
    res["fm"] = bool(torch.allclose(fmv, d_fm[mine], rtol=1e-5, atol=1e-5 * float(d_fm.abs().max()))) and (not fm_exact or torch.equal(fmv, d_fm[mine]))
    name_of = {t.data_ptr(): n for n, t in step.keep[2].items()}
    lists = _global_lists(entries, name_of, names, world, rank)
    sk, sv = _sorted_cat(lists)
    dk, dv = _sorted_cat(_direct_lists(d_groups, world, rank))
    res["keys"] = torch.equal(sk, dk)
    res["values"] = res["keys"] and torch.equal(sv.view(torch.int32), dv.view(torch.int32))
    # float64 on the concatenation, this rank's rows
    fm_term, fm_mass = _fm_grad64(torch.stack([t[x].double() for t, x in zip(tabs, ins)], 1), g_fm)
    ok = True
    for f in range(F2):
        x = ins[f]
        keep = (x != 0) & (x % world == rank)
        c = g_out[:, f * D2:(f + 1) * D2].double() + fm_term[:, f]
        uniq, inv = torch.unique(x[keep], return_inverse=True)
        ref = torch.zeros((uniq.numel(), D2), dtype=torch.float64, device=DEV).index_add_(0, inv, c[keep])
        cm = g_out[:, f * D2:(f + 1) * D2].double().abs() + fm_mass[:, f]
        mass = torch.zeros((uniq.numel(), D2), dtype=torch.float64, device=DEV).index_add_(0, inv, cm[keep])
        sel = (sk >> 40) == f
        ok &= torch.equal(sk[sel] & ROW, uniq) and bool(((sv[sel].double() - ref).abs() <= 2e-6 * mass + 1e-6).all())
    res["float64"] = ok
    res["n_keys"] = int(sk.numel())
    res["overflowed"] = step.overflowed()
    res["_snap"] = (out.clone(), _snapshot(entries))
    return res


def _world2_worker(rank, world, port, q, case, one_sided, direct_grad):
    import os
    from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import _poison
    _poison.poison()          # (NRX_TEST_POISON=1: this rank's buffers start from 0xFF bytes)
    try:
        tabs = _tables2()
        names = [f"C{i:02d}" for i in range(F2)]
        arenas = {n: shard_step.make_arena(ROWS2, D2, rank, world, DEV, full=t) for n, t in zip(names, tabs)}
        feats = [ShardedFeature(n, NRX_SPARSE, n, D2, 0, False, True) for n in names]
        out = {}
        kinds = ("overflow",) if case == "overflow" else ("uniform", "zipf")
        for kind in kinds:                                        # (at most two bound steps per process)
            batches = [_batch2(kind, r) for r in range(world)]
            ids, g_out, g_fm = batches[rank]
            inputs = [torch.from_numpy(x).to(DEV) for x in ids]
            if kind == "overflow":
                # the default slack: rank 0's block of feature 3 receives all B2 lookups of every rank -- more than capf
                eng = RowShardedEmbedding(rank, world, host_staged=True, overflow_policy="defer")
                step = shard_step.PreparedShardedStep(eng, feats, inputs, [None] * F2, arenas, one_sided=one_sided)
                assert step.groups[0]["capf"] < B2
                step.run()
                out["overflowed"] = step.overflowed()
                step.run()
                try:
                    step.check()
                    out["raised"] = False
                except RuntimeError as e:
                    out["raised"] = "overflowed" in str(e)
                dist.barrier()
                slack = 1.0
            else:
                slack = 0.05 if kind == "uniform" else _slack_for(batches, world)
            eng = RowShardedEmbedding(rank, world, slack=slack, host_staged=True, overflow_policy="defer")
            step = shard_step.PreparedShardedStep(eng, feats, inputs, [None] * F2, arenas, one_sided=one_sided).bind_backward(g_out, g_fm, direct_grad=direct_grad)
            r1 = _world2_compare(step, tabs, batches, rank, world, fm_exact=one_sided is False)
            out2, _, _ = step.run()                               # the same batch again: the same bits
            entries2 = step.backward()
            torch.cuda.synchronize()
            dist.barrier()
            same = torch.equal(r1["_snap"][0].view(torch.int32), out2.view(torch.int32)) and _same(r1["_snap"][1], _snapshot(entries2))
            out[kind] = {k: v for k, v in r1.items() if not k.startswith("_")}
            out[kind]["same"] = same
            out[kind]["placed"] = all(g["placed"] for g in step.groups)
            out[kind]["direct"] = all(b["direct"] for b in step.bwd)
            del step
        q.put((rank, out))
        dist.barrier()                                            # nobody unmaps a buffer a peer may still be writing
    except Exception as e:                                        # (reported, not lost: the parent fails with it instead of waiting)
        q.put((rank, {"error": f"{type(e).__name__}: {e}"[:500]}))
        raise
    finally:
        dist.destroy_process_group()


def _spawn2(case, one_sided, direct_grad):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world2_worker, args=(r, world, port, q, case, one_sided, direct_grad)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            item = q.get(timeout=600)
            assert "error" not in item[1], item
            res[item[0]] = item[1]
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:                                            # (a rank that failed leaves its peer waiting in a collective)
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    return res


@pytest.mark.parametrize("form", ["buffered", "default"])
def test_world_2_c2_feature_count_at_full_size_equals_the_direct_path(form):
    """26 tables x 1 M rows x 16, B = 32 768 per rank, uniform ids at the default slack and Zipf ids at the slack their largest block needs: every
    rank's concat bit for bit (the FM logit to 1e-5), the union of the ranks' (key, value) sets == the direct gradient on the concatenation bit
    for bit, the float64 per-row bound, two runs the same bits.  buffered = all-to-all forms; default = one-sided placement + direct gradient pack."""
    need_free(12 << 30)
    one_sided, direct_grad = (False, False) if form == "buffered" else (None, None)
    res = _spawn2("forms", one_sided, direct_grad)
    for r in (0, 1):
        for kind in ("uniform", "zipf"):
            got = res[r][kind]
            assert got["placed"] == (form == "default") and got["direct"] == (form == "default"), (r, kind, got)
            assert not got["overflowed"] and got["same"], (r, kind, got)
            assert got["out"] and got["fm"] and got["keys"] and got["values"] and got["float64"], (r, kind, got)
            assert got["n_keys"] > 0


def test_world_2_a_real_overflow_is_reported_and_a_larger_slack_recovers():
    """One feature's ids all even rows (all owned by rank 0) at the default slack: nrx_route_feat's block overflows, overflowed() says so and check()
    raises RuntimeError on both ranks; the same batch with slack = 1.0 equals the direct path."""
    need_free(12 << 30)
    res = _spawn2("overflow", None, None)
    for r in (0, 1):
        got = res[r]
        assert got["overflowed"] and got["raised"], (r, got)
        o = got["overflow"]
        assert not o["overflowed"] and o["same"] and o["out"] and o["fm"] and o["keys"] and o["values"] and o["float64"], (r, o)
