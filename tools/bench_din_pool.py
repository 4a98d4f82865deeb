#!/usr/bin/env python3
"""Time and peak memory of the fused target-attention pooling (ops.din_pool) beside what it replaces, on one GPU, in one process:
  fused  ops.din_pool on the table, the [B, N] ids and the [B, D] query;
  math   ops.din_pool_math over the materialised rows of a one-slot gather (what BaseModel.get_feature_embedding does): the way to this
         result without the operator;
  mean   the masked-mean bag slot of the fused embedding launch at the same shape (embed_apply, NRX_BAG_MASKED_MEAN): the same row traffic,
         the floor of the forward.
Shapes: N = 50 (the history length), D = 16 and 64, B = 65 536 and 512, a 200 000-row fp32 table, int64 ids.  Legs: forward (no autograd graph)
and forward + backward (ends with the gradients of the query and of the table in the default dense mode; `mean` has no query).  Legs are
warmed, then timed alternately (leg after leg within a round) over --rounds rounds of --iters calls each between two device events; a line
holds each leg's median over the rounds and its spread (max - min) / median.  Algorithmic bytes of the pooling itself: forward
B N (8 + 4 + 4 D) + B (8 D + 4) (ids, mask -- counted with or without one --, rows; query read, out written, lse), backward the forward's
plus 4 B N D + 8 B D (g_rows written;
g_out read, g_query written) -- the table gradient's reduction behind g_rows is the embedding backward's and is not counted; `hbm_frac` is
those bytes over the time at the 8 TB/s HBM peak.  Peak memory is the rise of the allocator's peak over one call of the leg.  One JSON line
per shape on stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEQ = 50
ROWS = 200_000
SHAPES = ((65536, 16), (65536, 64), (512, 16), (512, 64))
HBM_PEAK = 8.0e12


def run_shape(B, D, rounds, iters, masked):
    import torch
    from news_recsys_amd import ops
    from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_SPARSE

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + D)
    table = torch.randn(ROWS, D, device=dev, generator=gen).requires_grad_(True)
    with torch.no_grad():
        table[0] = 0
    ids = torch.randint(1, ROWS, (B, SEQ), device=dev, generator=gen)
    query = torch.randn(B, D, device=dev, generator=gen).requires_grad_(True)
    g = torch.randn(B, D, device=dev, generator=gen)
    mask = torch.ones(B, SEQ, device=dev)          # (the mean slot always takes one; the pooling legs take None when nothing is masked)
    if masked:
        lens = torch.randint(1, SEQ + 1, (B,), device=dev, generator=gen)
        mask = (torch.arange(SEQ, device=dev)[None, :] < lens[:, None]).float()
        ids = ids * mask.long()
    gather = ops.EmbedPlan([ops.Slot("user_history", NRX_SPARSE, 0, D, 0, 0)], out_width=D)
    bag = ops.EmbedPlan([ops.Slot("user_history", NRX_BAG_MASKED_MEAN, 0, D, SEQ, 0)], out_width=D)
    flat = ids.view(-1)
    pmask = mask if masked else None

    def fused(t, q):
        return ops.din_pool(t, ids, q, pmask, index_check="off")

    def math(t, q):
        rows = ops.embed_apply(gather, [t], [flat], [None], index_check="off")[0].view(B, SEQ, D)
        return ops.din_pool_math(None, None, q, pmask, rows=rows)

    def mean(t, q):
        return ops.embed_apply(bag, [t], [ids], [mask], index_check="off")[0]

    def leg(fn, backward, with_query):
        if backward:
            return lambda: torch.autograd.grad(fn(table, query), (table, query) if with_query else (table,), g)
        td, qd = table.detach(), query.detach()

        def fwd():
            with torch.no_grad():
                return fn(td, qd)
        return fwd

    legs = {f"{name}_{'fwdbwd' if bwd else 'fwd'}": leg(fn, bwd, name != "mean")
            for bwd in (False, True) for name, fn in (("fused", fused), ("math", math), ("mean", mean))}
    # results agree before anything is timed (fp32, summation orders differ)
    want = math(table.detach(), query.detach())
    err = float((fused(table.detach(), query.detach()) - want).abs().max())
    assert err <= 1e-4 * float(want.abs().max()), err
    gt_w, gq_w = torch.autograd.grad(math(table, query), (table, query), g)
    gt_f, gq_f = torch.autograd.grad(fused(table, query), (table, query), g)
    assert float((gq_f - gq_w).abs().max()) <= 1e-4 * float(gq_w.abs().max())
    assert float((gt_f[1:] - gt_w[1:]).abs().max()) <= 1e-4 * float(gt_w.abs().max())
    del want, gt_w, gq_w, gt_f, gq_f
    peak = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - before
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    fwd_bytes = B * SEQ * (8 + 4 + 4 * D) + B * (8 * D + 4)
    bwd_bytes = fwd_bytes + 4 * B * SEQ * D + 8 * B * D
    line = {"B": B, "N": SEQ, "D": D, "rows": ROWS, "masked": bool(masked), "rounds": rounds, "iters": iters}
    for name in legs:
        med = statistics.median(times[name])
        nbytes = fwd_bytes + bwd_bytes if name.endswith("fwdbwd") else fwd_bytes
        line[name] = {"us": round(med, 2), "spread": round((max(times[name]) - min(times[name])) / med, 3), "alg_bytes": nbytes,
                      "hbm_frac": round(nbytes / HBM_PEAK / (med * 1e-6), 4), "peak_mb": round(peak[name] / 1e6, 1)}
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (0: 10 at B = 65536, 100 below)")
    ap.add_argument("--masked", action="store_true", help="prefix masks of random length 1..N instead of an all-ones mask")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_din_pool.py measures on the GPU: none is visible")
    for B, D in SHAPES:
        line = run_shape(B, D, args.rounds, args.iters or (10 if B >= 65536 else 100), args.masked)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
