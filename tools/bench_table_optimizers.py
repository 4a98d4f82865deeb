"""The three row-sparse table optimizers beside each other: FusedSparseAdam's launch (nrx_sparse_adam_step, two fp32 moments per element), element-wise
Adagrad and row-wise Adagrad (nrx_sparse_adagrad_step, one fp32 accumulator per element / per row), in one process, HIP events around the timed loop.

Default: the C2 shape (26 tables x 1 M rows x 16) at B = 65 536.  One batch's (keys, values) list is formed once by the forward + row-sparse backward;
the OPTIMIZER LAUNCH ALONE is then timed on that list, the three optimizers ALTERNATING, `--rounds` times each, so a drift of the device shows in all
three; every round's time is kept, with the median and the (max - min) / median spread, as tools/bench_bf16_tables.py --sharded reports them.
`bytes_per_row` is the algorithmic traffic of one updated row (gradient and weight read, weight written, state read and written, the 8-byte key).

    python tools/bench_table_optimizers.py [--dtypes fp32,bf16] [--rounds 3] [--iters 50] [--out profiles/adagrad_lines.jsonl]
    python tools/bench_table_optimizers.py --only rowwise_adagrad --rounds 1          # the form profiled under rocprofv3

--sharded WL: a world-1 PreparedShardedStep TRAINING step of a bench workload (c5: Wide&Deep, 40 tables, whose Adam moments do not fit one card) WITH
FusedSparseAdagrad(rowwise=True) on the arenas, beside the same step without an optimizer (forward + backward), one storage type after the other.
`allocated_bytes` = torch.cuda.memory_allocated() after the tables and the optimizer state are built; `state_bytes` = the accumulators alone.  A
storage type whose tables + state do not fit the free memory is reported as `fits: false` and not run.

    python tools/bench_table_optimizers.py --sharded c5 [--dtypes fp32,bf16] [--rounds 3] [--out profiles/adagrad_lines.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import workload_spec                       # noqa: E402  (the workload definitions the headline uses)
from news_recsys_amd import _lib, ops                 # noqa: E402
from news_recsys_amd._lib import NRX_ADAGRAD_ROWWISE, NRX_ADAGRAD_TABLE_BF16, NRX_FEAT_TABLE_BF16, NRX_SPARSE   # noqa: E402
from news_recsys_amd.model.model_utils.optim import FusedSparseAdagrad                       # noqa: E402

B = 65536
OPTIMIZERS = ("adam", "adagrad", "rowwise_adagrad")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def timed(fn, iters, warm=3):
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


def summarize(ms):
    srt = sorted(ms)
    med = srt[len(srt) // 2]
    return dict(ms_rounds=[round(x, 5) for x in ms], ms_median=round(med, 5), spread_over_median=round((srt[-1] - srt[0]) / med, 4))


def run_launch_alone(dn, only, rounds, iters, dev):
    """C2: 26 x 1 M x 16.  Returns the result lines of one storage type."""
    dtype = DTYPES[dn]
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    n_tab, rows, D = 26, 1_000_000, 16
    tables = []
    for _ in range(n_tab):
        t = torch.randn(rows, D, device=dev, generator=gen).to(dtype)
        t[0] = 0
        tables.append(t)
    flag = NRX_FEAT_TABLE_BF16 if dtype is torch.bfloat16 else 0
    plan = ops.EmbedPlan([ops.Slot(f"C{i:02d}", NRX_SPARSE, i, D, 0, i * D, flags=flag) for i in range(n_tab)], out_width=n_tab * D)
    ins = [torch.randint(0, rows, (B,), device=dev, generator=gen) for _ in range(n_tab)]
    fwd = ops.PreparedEmbed(plan, tables, ins, [None] * n_tab)
    bwd = ops.PreparedSparseBackward(fwd, torch.randn(B, n_tab * D, device=dev, generator=gen) * 1e-2)
    fwd.run()
    (g,) = bwd.run()                                     # one embedding dim: one (keys, values) list, launch-local table numbers = positions
    torch.cuda.synchronize()
    n_unique = int(g["counts"][0])
    keys = torch.where(torch.arange(g["cap"], device=dev) < g["counts"][0], g["uniq"], torch.full_like(g["uniq"], torch.iinfo(torch.int64).max))
    keys, vals = keys[:n_unique].contiguous(), g["values"][:n_unique].contiguous()
    mv = [torch.zeros(rows, 2, D, device=dev) for _ in range(n_tab)]              # FusedSparseAdam's layout: a row's two moments side by side
    s_el = [torch.zeros(rows, D, device=dev) for _ in range(n_tab)]
    s_row = [torch.zeros(rows, device=dev) for _ in range(n_tab)]
    tp = (C.c_void_p * n_tab)(*[t.data_ptr() for t in tables])
    mp = (C.c_void_p * n_tab)(*[m[:, 0].data_ptr() for m in mv])
    vp = (C.c_void_p * n_tab)(*[m[:, 1].data_ptr() for m in mv])
    ep = (C.c_void_p * n_tab)(*[s.data_ptr() for s in s_el])
    rp = (C.c_void_p * n_tab)(*[s.data_ptr() for s in s_row])
    stream = torch.cuda.current_stream(dev).cuda_stream
    bf = dtype is torch.bfloat16
    step = [0]

    def adam():
        step[0] += 1
        if bf:
            ops.check(lib.nrx_sparse_adam_step_bf16(tp, mp, vp, n_tab, D, keys.data_ptr(), vals.data_ptr(), n_unique, None, 1e-3, None, 0.9, 0.999, 1e-8,
                                                    0.0, 1, step[0], None, stream), "nrx_sparse_adam_step_bf16")
        else:
            ops.check(lib.nrx_sparse_adam_step(tp, mp, vp, n_tab, D, keys.data_ptr(), vals.data_ptr(), n_unique, None, 1e-3, None, 0.9, 0.999, 1e-8, 0.0,
                                               stream), "nrx_sparse_adam_step")

    def adagrad(state, flags):
        def run():
            step[0] += 1
            ops.check(lib.nrx_sparse_adagrad_step(tp, state, n_tab, D, keys.data_ptr(), vals.data_ptr(), n_unique, None, 1e-2, None, 1e-10, 0.0,
                                                  flags | (NRX_ADAGRAD_TABLE_BF16 if bf else 0), 1, step[0], None, None, None, stream),
                      "nrx_sparse_adagrad_step")
        return run

    fns = {"adam": adam, "adagrad": adagrad(ep, 0), "rowwise_adagrad": adagrad(rp, NRX_ADAGRAD_ROWWISE)}
    w = 2 if bf else 4
    per_row = {"adam": 8 + 4 * D + 2 * w * D + 4 * 4 * D, "adagrad": 8 + 4 * D + 2 * w * D + 2 * 4 * D, "rowwise_adagrad": 8 + 4 * D + 2 * w * D + 2 * 4}
    names = [o for o in OPTIMIZERS if only is None or o in only]
    times = {o: [] for o in names}
    for o in names:
        timed(fns[o], 5, warm=5)
    for _ in range(rounds):
        for o in names:                                  # alternating: a drift of the device shows in all three
            times[o].append(timed(fns[o], iters))
    out = []
    for o in names:
        s = summarize(times[o])
        nbytes = per_row[o] * n_unique
        out.append(dict(workload="c2", leg="optimizer_launch", optimizer=o, table_dtype=dn, batch=B, unique_rows=n_unique, bytes_per_row=per_row[o],
                        achieved_GBps=round(nbytes / s["ms_median"] / 1e6, 1), alternating=len(names) > 1, **s))
    if "adam" in times:
        a = summarize(times["adam"])
        for o in names:
            if o != "adam":
                out.append(dict(workload="c2", leg="optimizer_launch", table_dtype=dn, ratio=f"{o}_over_adam_time",
                                value=round(summarize(times[o])["ms_median"] / a["ms_median"], 4), adam_spread_over_median=a["spread_over_median"]))
    return out


def run_sharded(wl, dn, rounds, iters, dev):
    """World-1 PreparedShardedStep training step of workload `wl` with row-wise Adagrad on the arenas, beside forward + backward alone."""
    from news_recsys_amd.shard_step import arena_row_map
    from news_recsys_amd.sharding import ShardedBenchPath
    dtype = DTYPES[dn]
    feats, _ = workload_spec(wl)
    table_bytes = sum(f["rows"] * f["dim"] * (2 if dtype is torch.bfloat16 else 4) for f in feats if "share" not in f)
    state_bytes = sum((f["rows"] + 1) * 4 for f in feats if "share" not in f)
    free, total = torch.cuda.mem_get_info(dev)
    head = dict(workload=wl, world=1, batch=B, table_dtype=dn, optimizer="rowwise_adagrad", table_bytes_expected=int(table_bytes),
                state_bytes_expected=int(state_bytes), free_bytes=int(free), total_bytes=int(total))
    if table_bytes + state_bytes > 0.97 * free:
        return [dict(head, leg="sharded_step", fits=False)]
    base = torch.cuda.memory_allocated(dev)
    path = ShardedBenchPath(wl, dev, 0, 0, 1, B, "row", table_dtype=dtype)
    torch.cuda.synchronize()
    tables_allocated = torch.cuda.memory_allocated(dev) - base
    assert path.train_setup()
    names = sorted(path.arenas)
    params = [path.arenas[n] for n in names]
    sink = ops.SparseGradSink()
    opt = FusedSparseAdagrad(sink, lr=1e-2, rowwise=True, params=params, sr_seed=1,
                             row_maps=[arena_row_map(0, 1)] * len(params) if dtype is torch.bfloat16 else None)
    for p in params:
        opt._register(p)                                 # the accumulators of every arena, before anything is timed
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(dev) - base
    i = [0]

    def fwd_bwd():
        i[0] += 1
        path.train_step(i[0])

    def step():
        i[0] += 1
        sink.pending.extend(path.train_step(i[0]))
        opt.step()

    timed(fwd_bwd, 3, warm=3)
    timed(step, 3, warm=3)
    times = {"sharded_fwd_bwd": [], "sharded_step": []}
    for _ in range(rounds):
        times["sharded_fwd_bwd"].append(timed(fwd_bwd, iters, warm=2))
        times["sharded_step"].append(timed(step, iters, warm=2))
    peak = torch.cuda.max_memory_allocated(dev)
    out = []
    for leg, ms in times.items():
        out.append(dict(head, leg=leg, fits=True, with_optimizer=leg == "sharded_step", tables_allocated_bytes=int(tables_allocated),
                        allocated_bytes=int(allocated), state_bytes=int(sum(s.numel() * 4 for s in opt.sums)), peak_allocated_bytes=int(peak),
                        alternating=True, **summarize(ms)))
    del path, opt, sink, params
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None, help="comma-separated subset of adam,adagrad,rowwise_adagrad")
    ap.add_argument("--sharded", default=None, metavar="WL", help="a bench workload (c2..c5): the world-1 bound training step with row-wise Adagrad")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    only = None if a.only is None else set(a.only.split(","))
    lines = []
    for dn in a.dtypes.split(","):
        res = run_sharded(a.sharded, dn, a.rounds, min(a.iters, 20), dev) if a.sharded else run_launch_alone(dn, only, a.rounds, a.iters, dev)
        for ln in res:
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
