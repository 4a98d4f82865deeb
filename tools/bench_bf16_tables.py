"""bf16 against fp32 embedding tables on the bench workloads (C2, C3, C4, C5 at B = 65 536), in one process, HIP events around the timed loop.

Per workload and storage type, one after the other (the first set is freed before the second is built, so C5 never holds both):
  fwd        the concat forward (PreparedEmbed: validation and descriptors done once, the launch alone timed); for C2 with the FM epilogue
  fm_only    C2 only: the FM-only inference form (need_out=False: no concat written)
  train      forward + row-sparse backward into a SparseGradSink + FusedSparseAdam step (bf16: nrx_sparse_adam_step_bf16)
  fwd_bwd    the same without the optimizer step (train - fwd_bwd = the optimizer)
Each line records the algorithmic bytes for its storage type (rows at 2 B per element for bf16, 4 B for fp32; ids 8 B; the fp32 concat write
and, for masked-mean bags, the 4-B weights unchanged) and the fraction of 8 TB/s.  The training leg needs fp32 moments for every row of every
table ([rows, 2, D]); where they do not fit next to the tables (C5; C3 on a box with less free memory) the leg runs over the tables of at most
16 M rows and says so (`train_tables`).  C5's own forward likewise keeps the tables of at most 16 M rows when the 224 GB fp32 set does not fit.

    python tools/bench_bf16_tables.py [--workloads c2,c3,c4,c5] [--iters 50] [--train-iters 20] [--out profiles/bf16_tables_lines.jsonl]
    python tools/bench_bf16_tables.py --workloads c2 --dtypes bf16 --legs fwd      # the form profiled under rocprofv3

--sharded: the BOUND SHARDED STEP at world 1 instead (shard_step.PreparedShardedStep over sharding.ShardedBenchPath's tables, the path bench.py's
sharded legs time), per workload:
  sharded_fwd    the bound forward (the forward-only calls of the path, cycling over its id sets)
  sharded_step   forward + backward + FusedSparseAdam on the arenas (bf16: row maps wired, nrx_sparse_adam_step_bf16_rows) -- or, where the
                 fp32 moments of every row do not fit (C5), `sharded_fwd_bwd`: the same without the optimizer
Both storage types are built and warmed up, then timed ALTERNATING, `--rounds` times each, so a drift of the device shows in both; every
round's time is kept and the fp32 leg's own spread stands beside every ratio.  Where the two table sets do not fit together (C5: 224 + 112 GB)
they run one after the other (`alternating: false`).  `allocated_bytes` = torch.cuda.memory_allocated() after the tables are built.

    python tools/bench_bf16_tables.py --sharded [--workloads c2,c3,c4,c5] [--rounds 3] [--out profiles/bf16_sharded_lines.jsonl]
    python tools/bench_bf16_tables.py --sharded --workloads c4 --dtypes bf16 --rounds 1      # the form profiled under rocprofv3
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import workload_spec                       # noqa: E402  (the workload definitions the headline uses)
from news_recsys_amd import ops                       # noqa: E402
from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_FEAT_TABLE_BF16, NRX_SPARSE   # noqa: E402
from news_recsys_amd.model.model_utils.optim import FusedSparseAdam                       # noqa: E402

B = 65536
PEAK = 8.0e12
SMALL_ROWS = 16_000_000


def build_tables(feats, dtype, dev, gen, max_rows=None):
    tabs, slots, col = {}, [], 0
    flag = NRX_FEAT_TABLE_BF16 if dtype is torch.bfloat16 else 0
    names = []
    for f in feats:
        tname = f.get("share", f["name"])
        if max_rows is not None and f["rows"] > max_rows:
            continue
        if tname not in tabs:
            t = torch.empty(f["rows"], f["dim"], dtype=dtype, device=dev)
            step = 1 << 24
            for r0 in range(0, f["rows"], step):             # fp32 N(0, 1) rows, rounded per chunk: no fp32 copy of a whole bf16 table
                t[r0:r0 + step] = torch.randn(min(step, f["rows"] - r0), f["dim"], device=dev, generator=gen).to(dtype)
            t[0] = 0
            tabs[tname] = t
            names.append(tname)
        kind = NRX_BAG_MASKED_MEAN if f["bag"] else NRX_SPARSE
        slots.append(ops.Slot(f["name"], kind, names.index(tname), f["dim"], f["bag"], col, flags=flag))
        col += f["dim"]
    return [tabs[n] for n in names], slots, col


def inputs_for(slots, tables, dev, gen):
    ins, ws = [], []
    for s in slots:
        rows = tables[s.table].shape[0]
        if s.bag_len:
            ins.append(torch.randint(0, rows, (B, s.bag_len), device=dev, generator=gen))
            lens = torch.randint(0, s.bag_len + 1, (B, 1), device=dev, generator=gen)
            ws.append((torch.arange(s.bag_len, device=dev)[None] < lens).float())
        else:
            ins.append(torch.randint(0, rows, (B,), device=dev, generator=gen))
            ws.append(None)
    return ins, ws


def fwd_bytes(slots, elem, concat: bool, fm: bool):
    per = 0
    for s in slots:
        n = max(1, s.bag_len)
        per += n * (8 + elem * s.dim + (4 if s.bag_len else 0)) + (4 * s.dim if concat else 0)
    return B * (per + (4 if fm else 0))


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def line(wl, dtype, leg, ms, nbytes, **extra):
    d = dict(workload=wl, table_dtype="bf16" if dtype is torch.bfloat16 else "fp32", leg=leg, batch=B, ms=round(ms, 5),
             algorithmic_bytes=int(nbytes), achieved_GBps=round(nbytes / ms / 1e6, 1), frac_of_8TBps=round(nbytes / (ms * 1e-3) / PEAK, 4))
    d.update(extra)
    return d


def run_workload(wl, dtype, legs, iters, train_iters, dev):
    feats, _ = workload_spec(wl)
    gen = torch.Generator(device=dev).manual_seed(0)
    free, _ = torch.cuda.mem_get_info(dev)
    fp32_bytes = sum(f["rows"] * f["dim"] * 4 for f in feats if "share" not in f)
    max_rows = SMALL_ROWS if fp32_bytes > 0.8 * free else None          # the same table set for both storage types of a workload
    out = []
    tables, slots, width = build_tables(feats, dtype, dev, gen, max_rows)
    ins, ws = inputs_for(slots, tables, dev, gen)
    elem = tables[0].element_size()
    fm = wl == "c2"
    plan = ops.EmbedPlan([ops.Slot(s.name, s.kind, s.table, s.dim, s.bag_len, s.out_col, fm_field=int(fm), flags=s.flags) for s in slots],
                         out_width=width, use_fm=fm)
    note = {"tables": "rows <= 16M only" if max_rows else "all"}
    if "fwd" in legs:
        call = ops.PreparedEmbed(plan, tables, ins, ws)
        out.append(line(wl, dtype, "fwd", timed(call.run, iters), fwd_bytes(slots, elem, True, fm), **note))
        if fm:
            call = ops.PreparedEmbed(plan, tables, ins, ws, need_out=False)
            out.append(line(wl, dtype, "fm_only", timed(call.run, iters), fwd_bytes(slots, elem, False, True), **note))
        del call
    if "train" in legs:
        free, _ = torch.cuda.mem_get_info(dev)
        mom = sum(t.shape[0] * t.shape[1] * 8 for t in tables)
        keep = list(range(len(tables)))
        if mom > 0.8 * free:                   # moments of every row do not fit: train the tables of <= 16 M rows
            keep = [i for i, t in enumerate(tables) if t.shape[0] <= SMALL_ROWS]
        tslots = [s for s in slots if s.table in keep]
        remap = {k: i for i, k in enumerate(keep)}
        col, ts = 0, []
        for s in tslots:
            ts.append(ops.Slot(s.name, s.kind, remap[s.table], s.dim, s.bag_len, col, flags=s.flags))
            col += s.dim
        tplan = ops.EmbedPlan(ts, out_width=col)
        ttabs = [tables[k].requires_grad_(True) for k in keep]
        tins = [ins[slots.index(s)] for s in tslots]
        tws = [ws[slots.index(s)] for s in tslots]
        sink = ops.SparseGradSink()
        opt = FusedSparseAdam(sink, lr=1e-3, params=ttabs, sr_seed=1)
        g = torch.randn(B, col, device=dev, generator=gen)

        def step():
            o = ops.embed_apply(tplan, ttabs, tins, tws, sparse_grad=sink, index_check="off")[0]
            o.backward(g)
            opt.step()
        def fwd_bwd():                          # the same without the optimizer: train - fwd_bwd = the optimizer step
            o = ops.embed_apply(tplan, ttabs, tins, tws, sparse_grad=sink, index_check="off")[0]
            o.backward(g)
            sink.clear()
        ms = timed(step, train_iters, warm=3)
        ms_fb = timed(fwd_bwd, train_iters, warm=3)
        tb = fwd_bytes(tslots, elem, True, False)
        out.append(line(wl, dtype, "train", ms, tb, train_tables=f"{len(keep)} of {len(tables)}",
                        bytes_note="forward bytes only (the backward's and optimizer's traffic is not counted)", **note))
        out.append(line(wl, dtype, "fwd_bwd", ms_fb, tb, train_tables=f"{len(keep)} of {len(tables)}",
                        bytes_note="forward bytes only; no optimizer step", **note))
        del opt, sink, ttabs, g
    del tables, ins, ws
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


class ShardedLegs:
    """One storage type of one workload through the bound sharded step at world 1."""

    def __init__(self, wl, dtype, dev, with_opt):
        from news_recsys_amd.shard_step import arena_row_map
        from news_recsys_amd.sharding import ShardedBenchPath
        base = torch.cuda.memory_allocated(dev)
        self.path = ShardedBenchPath(wl, dev, 0, 0, 1, B, "row", table_dtype=dtype)
        torch.cuda.synchronize()
        self.allocated = torch.cuda.memory_allocated(dev) - base
        self.table_bytes = sum(a.numel() * a.element_size() for a in self.path.arenas.values())
        assert self.path.train_setup()
        self.with_opt = with_opt
        self.i = 0
        self.sink = self.opt = None
        if with_opt:
            names = sorted(self.path.arenas)
            params = [self.path.arenas[n] for n in names]
            self.sink = ops.SparseGradSink()
            self.opt = FusedSparseAdam(self.sink, lr=1e-3, params=params, sr_seed=1,
                                       row_maps=[arena_row_map(0, 1)] * len(params) if dtype is torch.bfloat16 else None)

    def fwd(self):
        calls = self.path.calls
        self.i += 1
        calls[2 + self.i % (len(calls) - 2)].run()

    def step(self):
        self.i += 1
        entries = self.path.train_step(self.i)
        if self.opt is not None:
            self.sink.pending.extend(entries)
            self.opt.step()


def run_sharded(wl, dtypes, rounds, iters, train_iters, dev):
    feats, _ = workload_spec(wl)
    fp32_bytes = sum(f["rows"] * f["dim"] * 4 for f in feats if "share" not in f)
    free, _ = torch.cuda.mem_get_info(dev)
    with_opt = 3 * fp32_bytes < 0.8 * free                   # one storage type's tables + fp32 moments [rows, 2, D]
    together = len(dtypes) > 1 and (5.5 if with_opt else 1.5) * fp32_bytes < 0.8 * free
    step_leg = "sharded_step" if with_opt else "sharded_fwd_bwd"
    times = {(dn, leg): [] for dn in dtypes for leg in ("sharded_fwd", step_leg)}
    info = {}

    def build(dn):
        s = ShardedLegs(wl, {"fp32": torch.float32, "bf16": torch.bfloat16}[dn], dev, with_opt)
        info[dn] = dict(allocated_bytes=int(s.allocated), table_bytes=int(s.table_bytes))
        timed(s.fwd, 5, warm=5)
        timed(s.step, 3, warm=3)
        return s

    def measure(dn, s):
        times[(dn, "sharded_fwd")].append(timed(s.fwd, iters, warm=2))
        times[(dn, step_leg)].append(timed(s.step, train_iters, warm=2))

    if together:
        legs = {dn: build(dn) for dn in dtypes}
        for _ in range(rounds):
            for dn in dtypes:
                measure(dn, legs[dn])
        del legs
    else:
        for dn in dtypes:
            s = build(dn)
            for _ in range(rounds):
                measure(dn, s)
            del s
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = []
    med = {}
    for (dn, leg), ms in times.items():
        srt = sorted(ms)
        med[(dn, leg)] = srt[len(srt) // 2]
        out.append(dict(workload=wl, table_dtype=dn, leg=leg, world=1, batch=B, ms_rounds=[round(x, 5) for x in ms], ms_median=round(med[(dn, leg)], 5),
                        spread_over_median=round((srt[-1] - srt[0]) / med[(dn, leg)], 4), alternating=bool(together),
                        optimizer=bool(with_opt), **info[dn]))
    if "fp32" in dtypes and "bf16" in dtypes:
        for leg in ("sharded_fwd", step_leg):
            f32 = sorted(times[("fp32", leg)])
            out.append(dict(workload=wl, leg=leg, bf16_over_fp32_time=round(med[("bf16", leg)] / med[("fp32", leg)], 4),
                            fp32_spread_over_median=round((f32[-1] - f32[0]) / med[("fp32", leg)], 4), alternating=bool(together)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3,c4,c5")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--legs", default="fwd,train")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--train-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sharded", action="store_true", help="the bound sharded step at world 1 (see the module docstring)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if a.sharded:
        lines = []
        for wl in a.workloads.split(","):
            for ln in run_sharded(wl, a.dtypes.split(","), a.rounds, a.iters, a.train_iters, dev):
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
        return
    dts = {"fp32": torch.float32, "bf16": torch.bfloat16}
    legs = set(a.legs.split(","))
    lines = []
    for wl in a.workloads.split(","):
        res = {}
        for dn in a.dtypes.split(","):
            for ln in run_workload(wl, dts[dn], legs, a.iters, a.train_iters, dev):
                res[(ln["leg"], dn)] = ln
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        for leg in ("fwd", "fm_only", "train", "fwd_bwd"):
            if (leg, "fp32") in res and (leg, "bf16") in res:
                r = dict(workload=wl, leg=leg, bf16_over_fp32_time=round(res[(leg, "bf16")]["ms"] / res[(leg, "fp32")]["ms"], 3))
                lines.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
