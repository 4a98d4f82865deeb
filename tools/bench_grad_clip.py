"""What global-norm clipping of the row-sparse table gradients costs beside the optimizer step it precedes (nrx_rows_sqnorm + nrx_rows_sqnorm_finish +
nrx_rows_scale, include/nrx_embed.h), in one process, HIP events around the timed loop.

The C2 shape (26 tables x 1 M rows x 16, fp32) at B = 65 536.  One batch's (keys, values) list is formed once by the forward + row-sparse backward;
then, ALTERNATING over `--rounds` rounds so that a drift of the device shows in every leg:

    step              the optimizer launch alone (row-wise Adagrad, nrx_sparse_adagrad_step)
    step_norm         norm launch + finish launch + scale launch with a bound ABOVE the norm (the scale launch returns at once) + the step
    step_norm_scale   the same with a bound below the norm: the scale launch rewrites the list.  The bound starts a hair under the norm and shrinks by
                      0.999 with every call, so every iteration clips by ~0.999 (a fixed bound would clip once and then meet a norm equal to it)
    norm              the norm launch alone
    read              `values.sum()`: a plain read of the same bytes, the yardstick for the norm launch (it moves the list's bytes once)

Every round's time is kept, with the median and the (max - min) / median spread.

    python tools/bench_grad_clip.py [--rounds 3] [--iters 50] [--out profiles/grad_clip_lines.jsonl]
    python tools/bench_grad_clip.py --only norm --rounds 1          # the form profiled under rocprofv3
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

from news_recsys_amd import _lib, ops                 # noqa: E402
from news_recsys_amd._lib import NRX_ADAGRAD_ROWWISE, NRX_SPARSE   # noqa: E402
from tools.bench_table_optimizers import summarize, timed          # noqa: E402

B = 65536
LEGS = ("step", "step_norm", "step_norm_scale", "norm", "read")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(LEGS))
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    n_tab, rows, D = 26, 1_000_000, 16
    tables = []
    for _ in range(n_tab):
        t = torch.randn(rows, D, device=dev, generator=gen)
        t[0] = 0
        tables.append(t)
    plan = ops.EmbedPlan([ops.Slot(f"C{i:02d}", NRX_SPARSE, i, D, 0, i * D) for i in range(n_tab)], out_width=n_tab * D)
    ins = [torch.randint(0, rows, (B,), device=dev, generator=gen) for _ in range(n_tab)]
    fwd = ops.PreparedEmbed(plan, tables, ins, [None] * n_tab)
    bwd = ops.PreparedSparseBackward(fwd, torch.randn(B, n_tab * D, device=dev, generator=gen) * 1e-2)
    fwd.run()
    (g,) = bwd.run()
    torch.cuda.synchronize()
    n_unique = int(g["counts"][0])
    keys = torch.where(torch.arange(g["cap"], device=dev) < g["counts"][0], g["uniq"], torch.full_like(g["uniq"], torch.iinfo(torch.int64).max))
    keys, vals = keys[:n_unique].contiguous(), g["values"][:n_unique].contiguous()
    s_row = [torch.zeros(rows, device=dev) for _ in range(n_tab)]
    tp = (C.c_void_p * n_tab)(*[t.data_ptr() for t in tables])
    rp = (C.c_void_p * n_tab)(*[s.data_ptr() for s in s_row])
    stream = torch.cuda.current_stream(dev).cuda_stream
    bins = torch.zeros(258, dtype=torch.int64, device=dev)
    norm = torch.zeros(1, dtype=torch.float64, device=dev)
    coef = torch.ones(1, dtype=torch.float32, device=dev)
    step_no = [0]
    bound = [1e30]
    shrink = [1.0]

    def step():
        step_no[0] += 1
        ops.check(lib.nrx_sparse_adagrad_step(tp, rp, n_tab, D, keys.data_ptr(), vals.data_ptr(), n_unique, None, 1e-2, None, 1e-10, 0.0,
                                              NRX_ADAGRAD_ROWWISE, 1, step_no[0], None, None, None, stream), "nrx_sparse_adagrad_step")

    def norm_only():
        ops.check(lib.nrx_rows_sqnorm(keys.data_ptr(), vals.data_ptr(), n_unique, None, n_tab, D, 0, bins.data_ptr(), stream), "nrx_rows_sqnorm")

    def clipped():
        bound[0] *= shrink[0]
        norm_only()
        ops.check(lib.nrx_rows_sqnorm_finish(bins.data_ptr(), None, bound[0], norm.data_ptr(), coef.data_ptr(), 1, stream), "nrx_rows_sqnorm_finish")
        ops.check(lib.nrx_rows_scale(vals.data_ptr(), n_unique, D, coef.data_ptr(), stream), "nrx_rows_scale")
        step()

    def read():
        vals.sum()

    def leg(name):
        if name == "step":
            return step
        if name == "norm":
            return norm_only
        if name == "read":
            return read
        return clipped

    def arm(name):
        """The bound of the next timed loop: far above the norm, or the norm itself, shrinking by 0.999 per call."""
        bins.zero_()
        bound[0], shrink[0] = 1e30, 1.0
        if name == "step_norm_scale":
            norm_only()
            ops.check(lib.nrx_rows_sqnorm_finish(bins.data_ptr(), None, 1e30, norm.data_ptr(), coef.data_ptr(), 1, stream), "nrx_rows_sqnorm_finish")
            bound[0], shrink[0] = norm.item(), 0.999

    names = [x for x in LEGS if a.only is None or x in set(a.only.split(","))]
    times = {x: [] for x in names}
    for x in names:
        arm(x)
        timed(leg(x), 5, warm=5)
    for _ in range(a.rounds):
        for x in names:
            arm(x)
            times[x].append(timed(leg(x), a.iters))
    list_bytes = n_unique * (8 + 4 * D)
    lines = []
    for x in names:
        s = summarize(times[x])
        ln = dict(workload="c2", leg=x, table_dtype="fp32", optimizer="rowwise_adagrad", batch=B, unique_rows=n_unique, alternating=len(names) > 1, **s)
        if x in ("norm", "read"):
            nbytes = list_bytes if x == "norm" else n_unique * 4 * D
            ln.update(bytes_moved=nbytes, achieved_GBps=round(nbytes / s["ms_median"] / 1e6, 1))
        lines.append(ln)
    med = {x: summarize(times[x])["ms_median"] for x in names}
    for num, den in (("step_norm", "step"), ("step_norm_scale", "step"), ("norm", "read")):
        if num in med and den in med:
            lines.append(dict(workload="c2", ratio=f"{num}_over_{den}_time", value=round(med[num] / med[den], 4)))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
