#!/usr/bin/env python3
"""Time and peak memory of the fused attentional pooling of pair interactions (ops.afm_pool) beside the same arithmetic in stock torch, on one
GPU, in one process:
  fused  ops.afm_pool on the [B, F D] concat: one nrx_afm_fwd, one nrx_afm_bwd in the backward;
  math   ops.afm_pool_math: the gathered pair products, two matmuls, softmax, the weighted sum -- stock PyTorch fp32, the yardstick; it
         materialises [B, P, D] and [B, P, A] and keeps them for the backward.
Shapes: B = 65 536, F = 26, D = 16, A = 16 (the package's batch) and B = 8 192, F = 26, D = 64, A = 64.  Legs: forward (no autograd graph) and
forward + backward (ends with the gradients of x, w1, b1 and w2); the two entry points are timed alone through the C ABI too (`capi_us`).  Legs
are warmed, then timed alternately (leg after leg within a round) over --rounds rounds of --iters calls each between two device events; a line
holds each leg's median over the rounds and its spread (max - min) / median.  `mfma_frac`: the leg's matrix FLOP -- 2 B P D A per score GEMM,
one in the forward and three in the backward, plus 2 B F^2 D per S E product (the pooling; the backward's reduction onto the fields) -- over the
time at the 157 TFLOP/s fp32 matrix peak.  Peak memory is the rise of the allocator's peak over one call of the leg.  One JSON line per shape
on stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((65536, 26, 16, 16), (8192, 26, 64, 64))
MFMA_F32_PEAK = 157e12


def timed(legs, rounds, iters):
    import torch
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
    return times


def run_shape(B, F, D, A, rounds, iters):
    import torch
    from news_recsys_amd import _lib, ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + 100 * F + D)
    x = torch.randn(B, F * D, device=dev, generator=gen).requires_grad_(True)
    ps = [(torch.randn(A, D, device=dev, generator=gen) / D ** 0.5).requires_grad_(True), torch.zeros(A, device=dev, requires_grad=True),
          (torch.randn(A, device=dev, generator=gen) / A ** 0.5).requires_grad_(True)]
    g = torch.randn(B, D, device=dev, generator=gen)
    det = [p.detach() for p in ps]

    def fused_fwd():
        with torch.no_grad():
            return ops.afm_pool(x.detach(), F, D, *det)

    def math_fwd():
        with torch.no_grad():
            return ops.afm_pool_math(x.detach(), F, D, *det)

    def fused_fwdbwd():
        return torch.autograd.grad(ops.afm_pool(x, F, D, *ps), [x] + ps, g)

    def math_fwdbwd():
        return torch.autograd.grad(ops.afm_pool_math(x, F, D, *ps), [x] + ps, g)

    legs = {"fused_fwd": fused_fwd, "math_fwd": math_fwd, "fused_fwdbwd": fused_fwdbwd, "math_fwdbwd": math_fwdbwd}
    # results agree before anything is timed: forward and every gradient against the float64 form of the same definition, in batch chunks.
    # The forward is held to 1e-5 of the largest value.  The gradients are not continuous: a pre-activation within fp32 rounding of 0 switches
    # one attention unit's gradient on or off, and among the batch's B P A pre-activations (3.4e8 at the first shape) some are; so they are
    # held to 1e-2 only here (tests/test_afm_gpu.py holds them to derived bounds on inputs that stay clear of the kink).
    got, grads = fused_fwd(), fused_fwdbwd()
    want, wgrads = [], None
    for c in range(0, B, 8192):
        xs = x.detach()[c:c + 8192].double().requires_grad_(True)
        pd = [p.detach().double().requires_grad_(True) for p in ps]
        o = ops.afm_pool_math(xs, F, D, *pd)
        gr = torch.autograd.grad(o, [xs] + pd, g[c:c + 8192].double())
        want.append((o.detach(), gr[0]))
        wgrads = list(gr[1:]) if wgrads is None else [a + b for a, b in zip(wgrads, gr[1:])]
    pairs = [(got, torch.cat([w[0] for w in want])), (grads[0], torch.cat([w[1] for w in want]))] + list(zip(grads[1:], wgrads))
    agree = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in pairs]
    assert agree[0] <= 1e-5 and max(agree[1:]) <= 1e-2, agree
    del got, grads, want, wgrads, pairs
    peak = {}
    for name, fn in legs.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - before
    times = timed(legs, rounds, iters)
    P = F * (F - 1) // 2
    score, se = 2.0 * B * P * D * A, 2.0 * B * F * F * D
    line = {"B": B, "F": F, "D": D, "A": A, "rounds": rounds, "iters": iters, "score_gemm_gflop": round(score / 1e9, 2), "se_gflop": round(se / 1e9, 2),
            "max_err_vs_float64": [float(f"{e:.2e}") for e in agree]}
    for name in legs:
        med = statistics.median(times[name])
        flop = (4 * score + 2 * se) if name.endswith("fwdbwd") else (score + se)
        line[name] = {"us": round(med, 1), "spread": round((max(times[name]) - min(times[name])) / med, 3), "peak_mb": round(peak[name] / 1e6, 1)}
        if name.startswith("fused"):
            line[name]["mfma_frac"] = round(flop / MFMA_F32_PEAK / (med * 1e-6), 4)
    # the two entry points alone through the C ABI
    import ctypes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    off = (ctypes.c_int32 * F)(*range(0, F * D, D))
    xd = x.detach()
    out, lse, gx = torch.empty(B, D, device=dev), torch.empty(B, device=dev), torch.empty(B, F * D, device=dev)
    gs = [torch.empty_like(p) for p in det]
    wsp = torch.empty(lib.nrx_afm_bwd_workspace(B, F, D, A) // 4, device=dev)

    def fwd():
        _lib.check(lib.nrx_afm_fwd(xd.data_ptr(), F * D, off, F, D, det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr(), A, B, out.data_ptr(), D,
                                   lse.data_ptr(), st), "nrx_afm_fwd")

    def bwd():
        _lib.check(lib.nrx_afm_bwd(xd.data_ptr(), F * D, off, F, D, det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr(), A, B, out.data_ptr(), D,
                                   lse.data_ptr(), g.data_ptr(), D, gx.data_ptr(), F * D, gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(),
                                   wsp.data_ptr(), st), "nrx_afm_bwd")
    capi = {"fwd": fwd, "bwd": bwd}
    for fn in capi.values():
        fn()
    ct = timed(capi, rounds, iters)
    line["capi_us"] = {}
    for leg, flop in (("fwd", score + se), ("bwd", 3 * score + se)):
        med = statistics.median(ct[leg])
        line["capi_us"][leg] = {"us": round(med, 1), "mfma_frac": round(flop / MFMA_F32_PEAK / (med * 1e-6), 4)}
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_afm.py measures on the GPU: none is visible")
    for B, F, D, A in SHAPES:
        line = run_shape(B, F, D, A, args.rounds, args.iters)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
