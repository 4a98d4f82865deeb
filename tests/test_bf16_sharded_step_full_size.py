"""bf16 arenas through the bound sharded step at the FULL baseline sizes (world 1, B = 65 536): the real C2, C4 and C5 tables drawn in bf16
(sharding.ShardedBenchPath(table_dtype=torch.bfloat16): C5 is 112 GB, arena element offsets past 2^31), every default form of the step, uniform
and Zipf(1.05) id sets (refilled in place: padding ids, the last row, the first row past 2^31 elements, padded histories with an all-empty bag).

Truth is the direct bf16 path (PreparedEmbed with NRX_FEAT_TABLE_BF16 over the same memory, PreparedSparseBackward), itself tested against
float64 (tests/test_bf16_tables_gpu.py), in the scope in which the fp32 step is compared with its direct path bit for bit
(tests/test_shard_step_full_size.py):
  * every single-valued column == the widened table row (torch indexing) and == the direct bf16 call, bit for bit; C2's FM logit (the pass over
    the finished concat sums in another order) to that test's rtol 1e-5;
  * C4's pooled history columns: the float64 masked mean of the widened rows to that test's rel 1e-6, all-empty bags exact zeros;
  * C2 / C5 (keys, values) == the direct bf16 path's bit for bit (keys shifted by the dummy row); C4, whose pooled channel sums in another
    order: the same keys, values within that test's per-row bound 2e-6 * mass + 1e-6 (mass = the float64 L1 mass of the row's terms);
  * no overflow; the same bits twice.
The tables are released when a test ends."""
import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from news_recsys_amd._lib import NRX_FEAT_TABLE_BF16
from tests.test_full_size_baseline_shapes import need_free
from tests.test_shard_step_full_size import (B, DEV, FULL_BYTES, _direct_lists, _fill, _global_lists, _merge, _reference_grad, _same, _snapshot,
                                              _sorted_cat)

pytestmark = pytest.mark.gpu


class _Widened:
    """path.tables as the fp32 restatements index them: rows widened on the way out (no fp32 copy of a 112 GB table)."""

    def __init__(self, tables):
        self.tables = tables

    def __getitem__(self, name):
        t = self.tables[name]

        class _T:
            def __getitem__(self, ids):
                return t[ids].float()
        return _T()


def _direct16(path, ins, ws):
    names = sorted(path.tables)
    slots, col = [], 0
    for f in path.feats:
        slots.append(ops.Slot(f.name, f.kind, names.index(f.table), f.dim, f.bag_len, col, fm_field=int(path.fm), flags=NRX_FEAT_TABLE_BF16))
        col += f.dim
    plan = ops.EmbedPlan(slots, out_width=col, use_fm=path.fm)
    sums = torch.empty((B, path.feats[0].dim), dtype=torch.float32, device=DEV) if path.fm else None
    fwd = ops.PreparedEmbed(plan, [path.tables[t] for t in names], ins, [w if f.bag_len else None for f, w in zip(path.feats, ws)], fm_sums=sums)
    return fwd, ops.PreparedSparseBackward(fwd, path._g_out, path._g_fm), names


def _run(wl):
    from news_recsys_amd.sharding import ShardedBenchPath
    path = ShardedBenchPath(wl, DEV, 1234, 0, 1, B, "row", table_dtype=torch.bfloat16)
    assert path.engine == "feat" and path.train_setup()
    assert all(t.dtype is torch.bfloat16 for t in path.arenas.values())
    step = path.calls[0]
    assert step.bf16
    if wl != "c4":
        assert all(g["placed"] for g in step.groups if not g["pooled"]) and all(b["direct"] for b in step.bwd if not b["pooled"])      # the default forms
    ins, ws = path.pool[0]
    orig = [x.clone() for x in ins]
    names = sorted(path.tables)
    name_of = {a.data_ptr(): n for n, a in path.arenas.items()}
    cols = [s.out_col for s in step.plan.slots]
    if wl == "c5":
        assert max(t.numel() for t in path.tables.values()) > 2 ** 31
    fwd, bwd, _ = _direct16(path, ins, ws)
    wide = type("P", (), {})()          # the float64 restatement reads path.tables[t][ids], path.feats, path.fm, path._g_out, path._g_fm
    wide.tables, wide.feats, wide.fm, wide._g_out, wide._g_fm = _Widened(path.tables), path.feats, path.fm, path._g_out, path._g_fm
    rng = np.random.default_rng({"c2": 12, "c4": 14, "c5": 15}[wl])
    for kind in ("uniform", "zipf"):
        _fill(path, ins, ws, orig, kind, rng)
        runs = []
        for _ in range(2):
            out, _, fmv = step.run()
            entries = step.backward()
            torch.cuda.synchronize()
            runs.append((out.clone(), None if fmv is None else fmv.clone(), _snapshot(entries)))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
        assert runs[0][1] is None or torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
        assert _same(runs[0][2], runs[1][2])
        assert not path.overflowed()
        d_out, _, d_fm = fwd.run()
        d_groups = bwd.run()
        torch.cuda.synchronize()
        for i, (f, x, w) in enumerate(zip(path.feats, ins, ws)):
            c, D = cols[i], f.dim
            got = out[:, c:c + D]
            if f.bag_len:
                rows = path.tables[f.table][x].double()
                ref = (rows * w.double()[..., None]).sum(1) / (w.double().sum(1, keepdim=True) + 1e-8)
                del rows
                empty = w.sum(1) == 0
                assert bool(empty.any()) and bool((got[empty] == 0).all())
                rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
                assert rel < 1e-6, f"{f.name}: pooled rel {rel}"
            else:
                assert torch.equal(got, path.tables[f.table][x].float()), f.name
                assert torch.equal(got.view(torch.int32), d_out[:, c:c + D].view(torch.int32)), f.name
        if path.fm:
            torch.testing.assert_close(fmv, d_fm, rtol=1e-5, atol=1e-5 * float(d_fm.abs().max()))
        lists = _global_lists(entries, name_of, names)
        d_lists = _direct_lists(d_groups)
        if wl != "c4":
            sk, sv = _sorted_cat(lists)
            dk, dv = _sorted_cat(d_lists)
            assert torch.equal(sk, dk), "keys != the direct bf16 path"
            assert torch.equal(sv.view(torch.int32), dv.view(torch.int32)), "values != the direct bf16 path"
        else:
            r_keys, r_vals, r_mass = _reference_grad(wide, ins, ws, cols, names)
            tol = 2e-6 * r_mass + 1e-6
            mk, mv = _merge(lists)
            dk, dv = _merge(d_lists)
            assert torch.equal(mk, dk) and torch.equal(mk, r_keys)
            assert bool(((mv - dv).abs() <= tol).all()) and bool(((mv - r_vals).abs() <= tol).all())
            del r_keys, r_vals, r_mass, tol, mk, mv, dk, dv
        del lists, d_lists, d_out, d_groups


@pytest.mark.parametrize("wl", ["c2", "c4", "c5"])
def test_world_1_bf16_bench_step_at_full_size_equals_the_direct_bf16_path(wl):
    need_free(FULL_BYTES[wl] // 2 + (16 << 30))
    try:
        _run(wl)
    finally:            # (every holder of the tables was a local of _run: the memory goes back to the device for the tests after this one)
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
