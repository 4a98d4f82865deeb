#!/usr/bin/env python3
"""Time and peak memory of the fused pairwise dot-product interaction (ops.dot_interaction, ops.dot_interaction_cat_) beside what it replaces,
on one GPU, in one process:
  fused  ops.dot_interaction on the [B, F D] concat: z [B, P] in a buffer of its own;
  cat    ops.dot_interaction_cat_ on a [B, ld] buffer that holds the concat: z next to it, torch.cat([x, z]) without the pass (the form the PNN
         model runs); its backward returns the gradient of the whole buffer, the upstream gradient of the concat columns included;
  math   ops.dot_interaction_math (bmm + tril_indices + index) followed by torch.cat([x, z]): the way to the model's input without the operator.
Shapes: B = 65 536 with (F, D) in {(26, 16), (40, 32), (8, 64)} and B = 512 with (26, 16).  Legs: forward (no autograd graph) and forward +
backward (ends with the gradient of x; for `cat` and `math` the upstream gradient covers the concat columns too).  Legs are warmed, then timed
alternately (leg after leg within a round) over --rounds rounds of --iters calls each between two device events; a line holds each leg's median
over the rounds and its spread (max - min) / median.  Algorithmic bytes of the interaction itself: forward 4 B (F D + P) (fields read, pairs
written), backward 4 B (P + F D) more (g_z read, g_x written); `hbm_frac` is those bytes over the time at the 8 TB/s HBM peak (the figure
DESIGN 7h quotes for the DIN forward).  Peak memory is the rise of the allocator's peak over one call of the leg.  One JSON line per shape on
stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((65536, 26, 16), (65536, 40, 32), (65536, 8, 64), (512, 26, 16))
HBM_PEAK = 8.0e12


def run_shape(B, F, D, rounds, iters):
    import torch
    from news_recsys_amd import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + 100 * F + D)
    W, P = F * D, ops.dot_interaction_pairs(F)
    ld = (W + P + 3) // 4 * 4
    x = torch.randn(B, W, device=dev, generator=gen).requires_grad_(True)
    base = torch.zeros(B, ld, device=dev)
    base[:, :W] = x.detach()
    base.requires_grad_(True)
    g_z = torch.randn(B, P, device=dev, generator=gen)
    g_all = torch.randn(B, ld, device=dev, generator=gen)
    g_cat = g_all[:, :W + P].contiguous()

    def fused(t):
        return ops.dot_interaction(t, F, D)

    def cat(t):
        # (the model's buffer comes out of the embedding launch; here a copy stands in for it, outside the timed op in the forward leg)
        return ops.dot_interaction_cat_(t, W, F, D)

    def math(t):
        return torch.cat([t, ops.dot_interaction_math(t, F, D)], dim=1)

    work = base.detach().clone()

    def fused_fwd():
        with torch.no_grad():
            return fused(x.detach())

    def cat_fwd():
        with torch.no_grad():
            return cat(work)

    def math_fwd():
        with torch.no_grad():
            return math(x.detach())

    def fused_fwdbwd():
        return torch.autograd.grad(fused(x), (x,), g_z)

    def cat_fwdbwd():
        # base * 1 makes the non-leaf buffer the in-place op needs (one extra pass each way that the model does not pay: its buffer is
        # the embedding launch's own output)
        return torch.autograd.grad(cat(base * 1.0), (base,), g_all)

    def math_fwdbwd():
        return torch.autograd.grad(math(x), (x,), g_cat)

    legs = {"fused_fwd": fused_fwd, "cat_fwd": cat_fwd, "math_fwd": math_fwd, "fused_fwdbwd": fused_fwdbwd, "cat_fwdbwd": cat_fwdbwd,
            "math_fwdbwd": math_fwdbwd}
    # results agree before anything is timed (fp32, summation orders differ)
    want = math_fwd()
    got = fused_fwd()
    assert float((got - want[:, W:]).abs().max()) <= 1e-4 * float(want[:, W:].abs().max())
    assert torch.equal(cat_fwd()[:, W:W + P], got)
    gw, = math_fwdbwd()
    gc, = cat_fwdbwd()
    assert float((gc[:, :W] - gw).abs().max()) <= 1e-4 * float(gw.abs().max())
    del want, got, gw, gc
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
    fwd_bytes = 4 * B * (W + P)
    line = {"B": B, "F": F, "D": D, "P": P, "rounds": rounds, "iters": iters}
    for name in legs:
        med = statistics.median(times[name])
        nbytes = 2 * fwd_bytes if name.endswith("fwdbwd") else fwd_bytes
        line[name] = {"us": round(med, 2), "spread": round((max(times[name]) - min(times[name])) / med, 3), "alg_bytes": nbytes,
                      "hbm_frac": round(nbytes / HBM_PEAK / (med * 1e-6), 4), "peak_mb": round(peak[name] / 1e6, 1)}
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (0: 10 at B = 65536, 100 below)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dot_interact.py measures on the GPU: none is visible")
    for B, F, D in SHAPES:
        line = run_shape(B, F, D, args.rounds, args.iters or (10 if B >= 65536 else 100))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
