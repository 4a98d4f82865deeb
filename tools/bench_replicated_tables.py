"""Replicated small tables in the bound sharded step (shard_step.PreparedShardedStep(replicated_grads=True)), on one GPU, HIP events around the
timed loops; one JSON line per measurement.

(a) leg "step_w1": the bound step at world 1, forward + backward, B = 65 536, eager (fwd_bwd_us: host launch path included) and replayed from
    a captured HIP graph (fwd_bwd_graph_us), three forms per workload --
      replicated  the small tables held in full, their gradient from the final launch's restricted reduction (no exchange)
      row_sharded every table an arena, every feature routed (the round-6 step)
      direct      ops.PreparedEmbed + ops.PreparedSparseBackward on the full tables (the single-GPU path)
    C3: item_id, user_id, category, subcategory, user_click_category at D = 64; the 18 / 270 / 18-row tables replicated.
    C5: the tables of <= 16 M rows of the 40 (D = 32); the 10 smallest (1 000 - 20 661 rows) replicated and WIDE (WideDeep's column routing:
        column 0 -> wide [B, 10]).  A row-sharded wide feature is refused, so C5's row_sharded form is the plain concat of the same tables.
(b) leg "kernels_w8": nrx_rep_pack (one rank's local lists -> the chunked buffer), nrx_rep_ordered_sum (8 received chunks -> 1) and
    nrx_rep_compact (the gathered buffer -> keys, values per dim) at W = 8 shapes with fabricated partials (C5's 10 tables, C3's three); bytes
    moved over time next to a device-to-device copy of the same buffer.  The collectives between them are not here: nothing measures them on
    one GPU.

    python tools/bench_replicated_tables.py [--legs step_w1,kernels_w8] [--iters 50] [--out profiles/replicated_tables_lines.jsonl]
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import workload_spec                                           # noqa: E402
from news_recsys_amd import _lib, ops, shard_step                         # noqa: E402
from news_recsys_amd._lib import NRX_SPARSE                               # noqa: E402
from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature  # noqa: E402

B = 65536
DEV = "cuda:0"


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def workload(wl):
    feats, _ = workload_spec(wl)
    if wl == "c5":
        feats = [f for f in feats if f["rows"] <= 16_000_000]
        small = sorted(feats, key=lambda f: f["rows"])[:10]
    else:
        small = [f for f in feats if f["rows"] <= 270]
    return feats, {f["name"] for f in small}


def step_leg(wl, iters, gen):
    feats, small = workload(wl)
    wide = wl == "c5"
    arenas, full, ids = {}, {}, []
    for f in feats:
        a = shard_step.make_arena(f["rows"], f["dim"], 0, 1, DEV, generator=gen)     # world 1: arena[1:] IS the full table (row 0 = padding)
        arenas[f["name"]], full[f["name"]] = a, a[1:]
        ids.append(torch.randint(0, f["rows"], (B,), device=DEV, generator=gen))
    lines = []
    eng = RowShardedEmbedding(0, 1, overflow_policy="defer")
    for form in ("replicated", "row_sharded", "direct"):
        rep = form == "replicated"
        sfeats = [ShardedFeature(f["name"], NRX_SPARSE, f["name"], f["dim"], 0, wide and rep and f["name"] in small, False,
                                 rep and f["name"] in small) for f in feats]
        tabs = {f["name"]: (full if (rep and f["name"] in small) else arenas)[f["name"]] for f in feats}
        if form != "direct":
            step = shard_step.PreparedShardedStep(eng, sfeats, ids, [None] * len(feats), tabs, one_sided=False, replicated_grads=rep)
            g_out = torch.randn((B, step.ld), device=DEV, generator=gen)
            g_wide = torch.randn((B, step.plan.wide_width), device=DEV, generator=gen) if step.plan.wide_width else None
        if form == "direct":
            # the direct path: every table read in full with the original ids, the same routing as the replicated form (C5: the wide columns)
            dfeats = [dataclasses.replace(x, replicated=True, wide=wide and x.name in small) for x in sfeats]
            plan = eng._final_plan(dfeats, [], set())
            fwd = ops.PreparedEmbed(plan, [full[t] for t in eng.replicated_tables(dfeats)], ids, [None] * len(feats))
            g_out = torch.randn((B, plan.out_width), device=DEV, generator=gen)
            g_wide = torch.randn((B, plan.wide_width), device=DEV, generator=gen) if plan.wide_width else None
            bwd = ops.PreparedSparseBackward(fwd, g_out, g_wide=g_wide)

            def fn(fwd=fwd, bwd=bwd):
                fwd.run()
                bwd.run()
        else:
            step.bind_backward(g_out, g_wide=g_wide)

            def fn(step=step):
                step.run()
                step.backward()
        us = timed(fn, iters)
        # the same calls captured in a HIP graph and replayed: the device time without the host's launch path
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        gus = timed(graph.replay, iters)
        lines.append(dict(tool="bench_replicated_tables", leg="step_w1", workload=wl, form=form, batch=B, tables=len(feats),
                          replicated=sorted(small) if rep else [], wide=bool(wide and form != "row_sharded"), fwd_bwd_us=round(us, 1),
                          fwd_bwd_graph_us=round(gus, 1)))
        del graph
        print(json.dumps(lines[-1]), flush=True)
        del fn
        step = None
        torch.cuda.empty_cache()
    return lines


def kernels_leg(wl, iters, gen, world=8):
    lib = _lib.load()
    feats, small = workload(wl)
    tabs = [(f["rows"], f["dim"]) for f in feats if f["name"] in small]
    lay = shard_step.replicated_layout(tabs, world)
    cf, cr, Cw = lay["cf"], lay["cr"], lay["C"]
    n, D = len(tabs), tabs[0][1]
    stream = torch.cuda.current_stream().cuda_stream
    # one rank's local list: every table's rows that B uniform lookups touch (expected unique rows), keys ascending, random values
    keys, cap = [], 0
    for t, (rows, _) in enumerate(tabs):
        u = torch.unique(torch.randint(1, rows, (B,), device=DEV, generator=gen))
        keys.append((t << 40) | u)
    keys = torch.cat(keys)
    cap = keys.numel()
    vals = torch.randn((cap, D), device=DEV, generator=gen)
    cnt = torch.tensor([cap, 0], dtype=torch.int64, device=DEV)
    arr64 = lambda xs: (C.c_int64 * len(xs))(*xs)          # noqa: E731
    voff, roff, rws = arr64(lay["voff"]), arr64(lay["roff"]), arr64([r for r, _ in tabs])
    tdims = (C.c_int32 * n)(*[d for _, d in tabs])
    buf = torch.empty(world * Cw, dtype=torch.float32, device=DEV)
    red = torch.empty(Cw, dtype=torch.float32, device=DEV)
    okeys = torch.empty(sum(r for r, _ in tabs), dtype=torch.int64, device=DEV)
    ovals = torch.empty((okeys.numel(), D), dtype=torch.float32, device=DEV)
    ocnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    ws = torch.empty(max(8, lib.nrx_rep_compact_workspace(okeys.numel())), dtype=torch.uint8, device=DEV)
    pk = (C.c_void_p * 1)(keys.data_ptr())
    pv = (C.c_void_p * 1)(vals.data_ptr())
    pn = (C.c_void_p * 1)(cnt.data_ptr())

    def pack():
        ops.check(lib.nrx_rep_pack(pk, pv, pn, arr64([cap]), (C.c_int32 * 1)(D), 1, voff, roff, rws, tdims, n, world, cf, cr, buf.data_ptr(),
                                   stream), "nrx_rep_pack")

    def osum():
        ops.check(lib.nrx_rep_ordered_sum(buf.data_ptr(), world, cf, cr, red.data_ptr(), stream), "nrx_rep_ordered_sum")

    def compact():
        ops.check(lib.nrx_rep_compact(buf.data_ptr(), world, cf, cr, voff, roff, rws, (C.c_int32 * n)(*range(n)), n, D, okeys.data_ptr(),
                                      ovals.data_ptr(), okeys.numel(), ocnt.data_ptr(), ws.data_ptr(), stream), "nrx_rep_compact")

    pack()
    compact()
    torch.cuda.synchronize()
    n_out = int(ocnt[0])
    W4 = world * Cw * 4
    moved = dict(pack=W4 + cap * (D * 4 + 8), ordered_sum=W4 + Cw * 4,
                 compact=lay["rows"] * 4 + n_out * D * 4 * 2 + n_out * 8)      # counts read, touched rows read + written, keys written
    src = torch.empty(W4 // 4, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src), iters)
    lines = []
    for name, fn in (("pack", pack), ("ordered_sum", osum), ("compact", compact)):
        us = timed(fn, iters)
        lines.append(dict(tool="bench_replicated_tables", leg="kernels_w8", workload=wl, world=world, kernel=name, tables=n, dim=D,
                          replicated_bytes=lay["floats"] * 4, buffer_bytes=W4, local_rows=cap, out_rows=n_out, us=round(us, 2),
                          bytes=moved[name], gbps=round(moved[name] / us / 1e3, 1),
                          copy_same_buffer=dict(us=round(copy_us, 2), gbps=round(2 * W4 / copy_us / 1e3, 1))))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="step_w1,kernels_w8")
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(7)
    lines = []
    for wl in a.workloads.split(","):
        if "kernels_w8" in a.legs:
            lines += kernels_leg(wl, a.iters, gen)
        if "step_w1" in a.legs:
            lines += step_leg(wl, a.iters, gen)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
