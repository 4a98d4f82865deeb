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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3,c4,c5")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--legs", default="fwd,train")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--train-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
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
