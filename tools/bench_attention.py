#!/usr/bin/env python3
"""Time and peak memory of the fused short-sequence self-attention (ops.seq_attention) beside what it replaces, on one GPU, in one process:
  fused  ops.seq_attention on the [B, N, 3 C] projection output;
  math   the modules' torch path (model_utils.utils.attention_math: the reference's arithmetic, [B, H, N, N] scores materialised);
  sdpa   torch.nn.functional.scaled_dot_product_attention in fp32 on the permuted views, its output brought back to [B, N, C].
Shapes: N = 50 (the history length), (C, H) = (16, 2) and (64, 4), B = 65 536 and 512.  Legs: forward (no autograd graph) and forward + backward
(ends with the gradient of qkv).  Every leg starts from the same qkv tensor.  Legs are warmed, then timed alternately (path after path
within a round) over --rounds rounds of --iters calls each between two device events; a line holds each leg's median over the rounds and
its spread (max - min) / median.  Algorithmic bytes: forward 16 B N C (qkv read, out written), forward + backward 48 B N C (the forward's,
plus the backward's 32 B N C: qkv, out, g_out read, g_qkv written); `hbm_frac` is those bytes over the time at the 8 TB/s HBM peak.  Peak
memory is the rise of the allocator's peak over one call of the leg.  One JSON line per shape on stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEQ = 50
SHAPES = ((65536, 16, 2), (65536, 64, 4), (512, 16, 2), (512, 64, 4))
HBM_PEAK = 8.0e12


def run_shape(B, C, H, rounds, iters, masked):
    import torch
    import torch.nn.functional as F
    from news_recsys_amd import ops
    from news_recsys_amd.model.model_utils.utils import attention_math

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + C)
    x = torch.randn(B, SEQ, 3 * C, device=dev, generator=gen).requires_grad_(True)
    g = torch.randn(B, SEQ, C, device=dev, generator=gen)
    mask = None
    if masked:
        lens = torch.randint(1, SEQ + 1, (B,), device=dev, generator=gen)
        mask = (torch.arange(SEQ, device=dev)[None, :] < lens[:, None]).float()
    hd = C // H

    def fused(t):
        return ops.seq_attention(t, H, key_mask=mask)

    def math(t):
        return attention_math(t, H, mask)

    def sdpa(t):
        q, k, v = t.reshape(B, SEQ, 3, H, hd).permute(2, 0, 3, 1, 4)
        am = None if mask is None else (mask != 0)[:, None, None, :]
        return F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(B, SEQ, C)

    def leg(fn, backward):
        if backward:
            return lambda: torch.autograd.grad(fn(x), x, g)
        xd = x.detach()

        def fwd():
            with torch.no_grad():
                return fn(xd)
        return fwd

    legs = {f"{name}_{'fwdbwd' if bwd else 'fwd'}": leg(fn, bwd) for bwd in (False, True) for name, fn in (("fused", fused), ("math", math), ("sdpa", sdpa))}
    # results agree before anything is timed (fp32, summation orders differ)
    want = math(x.detach())
    for name, fn in (("fused", fused), ("sdpa", sdpa)):
        err = float((fn(x.detach()) - want).abs().max())
        assert err <= 1e-4 * float(want.abs().max()), (name, err)
    del want
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
    line = {"B": B, "N": SEQ, "C": C, "H": H, "masked": bool(masked), "rounds": rounds, "iters": iters}
    for name in legs:
        med = statistics.median(times[name])
        nbytes = (48 if name.endswith("fwdbwd") else 16) * B * SEQ * C
        line[name] = {"us": round(med, 2), "spread": round((max(times[name]) - min(times[name])) / med, 3), "alg_bytes": nbytes,
                      "hbm_frac": round(nbytes / HBM_PEAK / (med * 1e-6), 4), "peak_mb": round(peak[name] / 1e6, 1)}
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (0: 10 at B = 65536, 200 below)")
    ap.add_argument("--masked", action="store_true", help="prefix key masks of random length 1..N instead of no mask")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_attention.py measures on the GPU: none is visible")
    for B, C, H in SHAPES:
        line = run_shape(B, C, H, args.rounds, args.iters or (10 if B >= 65536 else 200), args.masked)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
