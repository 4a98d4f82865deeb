#!/usr/bin/env python3
"""Time and peak memory of the fused Compressed Interaction Network (ops.cin) beside the same arithmetic in stock torch, on one GPU, in one process:
  fused  ops.cin on the [B, m D] concat: one nrx_cin_layer_fwd per layer, one nrx_cin_layer_bwd per layer in the backward;
  math   ops.cin_math: einsum('bid,bjd->bijd'), the 1x1 convolution as an einsum, sum pooling -- stock PyTorch fp32, the yardstick; it
         materialises [B, Hp, m, D] per layer and keeps it for the backward.
Shapes: B = 65 536, m = 26, D = 16, layers [32, 32] (the package's batch) and B = 8 192, m = 26, D = 64, layers [64, 64].  Legs: forward (no
autograd graph) and forward + backward (ends with the gradients of x and of every W_k); the single layers' forward and backward are timed through
the C ABI too (`layers`).  Legs are warmed, then timed alternately (leg after leg within a round) over --rounds rounds of --iters calls each
between two device events; a line holds each leg's median over the rounds and its spread (max - min) / median.  `mfma_frac`: the leg's GEMM
FLOP -- 2 B D Hp m H per layer and GEMM; the forward is one GEMM per layer, the backward three -- over the time at the 157 TFLOP/s fp32 matrix
peak.  Peak memory is the rise of the allocator's peak over one call of the leg.  One JSON line per shape on stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((65536, 26, 16, (32, 32)), (8192, 26, 64, (64, 64)))
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


def run_shape(B, m, D, sizes, rounds, iters):
    import torch
    from news_recsys_amd import _lib, ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + 100 * m + D)
    x = torch.randn(B, m * D, device=dev, generator=gen).requires_grad_(True)
    ws, shapes, Hp = [], [], m
    for H in sizes:
        ws.append((torch.randn(H, Hp, m, device=dev, generator=gen) / (Hp * m) ** 0.5).requires_grad_(True))
        shapes.append((Hp, H))
        Hp = H
    g = torch.randn(B, sum(sizes), device=dev, generator=gen)
    offs = tuple(range(0, m * D, D))

    def fused_fwd():
        with torch.no_grad():
            return ops.cin(x.detach(), m, D, [w.detach() for w in ws])

    def math_fwd():
        with torch.no_grad():
            return ops.cin_math(x.detach(), m, D, [w.detach() for w in ws])

    def fused_fwdbwd():
        return torch.autograd.grad(ops.cin(x, m, D, ws), [x] + ws, g)

    def math_fwdbwd():
        return torch.autograd.grad(ops.cin_math(x, m, D, ws), [x] + ws, g)

    legs = {"fused_fwd": fused_fwd, "math_fwd": math_fwd, "fused_fwdbwd": fused_fwdbwd, "math_fwdbwd": math_fwdbwd}
    # results agree before anything is timed (fp32, summation orders differ)
    want, got = math_fwd(), fused_fwd()
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
    for a, b in zip(fused_fwdbwd(), math_fwdbwd()):
        assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max())
    del want, got, a, b
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
    flop = [2.0 * B * D * hp * m * h for hp, h in shapes]
    line = {"B": B, "m": m, "D": D, "layers": list(sizes), "rounds": rounds, "iters": iters, "gemm_gflop": [round(f / 1e9, 2) for f in flop]}
    for name in legs:
        med = statistics.median(times[name])
        gemms = sum(flop) * (4 if name.endswith("fwdbwd") else 1)
        line[name] = {"us": round(med, 1), "spread": round((max(times[name]) - min(times[name])) / med, 3), "peak_mb": round(peak[name] / 1e6, 1)}
        if name.startswith("fused"):
            line[name]["mfma_frac"] = round(gemms / MFMA_F32_PEAK / (med * 1e-6), 4)
    # the single layers through the C ABI: forward (1 GEMM) and backward (3 GEMMs + the ordered sum of the weight gradient's partials)
    import ctypes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    off = (ctypes.c_int32 * m)(*offs)
    xd = x.detach()
    pbuf = torch.empty(B, sum(sizes), device=dev)
    gx = torch.empty(B, m * D, device=dev)
    layer_legs, keep = {}, []
    xprev, col = None, 0
    for k, ((hp, h), w) in enumerate(zip(shapes, ws)):
        xk = torch.empty(B, h * D, device=dev)
        gxk = torch.randn(B, h * D, device=dev, generator=gen)
        gxp = None if xprev is None else torch.empty(B, hp * D, device=dev)
        gw = torch.empty_like(w)
        wsp = torch.empty(lib.nrx_cin_layer_bwd_workspace(B, m, hp, h, D) // 4, device=dev)
        keep += [xk, gxk, gxp, gw, wsp]
        ptr = lambda t: None if t is None else t.data_ptr()

        def fwd(xprev=xprev, hp=hp, h=h, w=w, xk=xk, col=col):
            _lib.check(lib.nrx_cin_layer_fwd(xd.data_ptr(), m * D, off, m, D, ptr(xprev), hp * D, hp, w.data_ptr(), h, B, xk.data_ptr(), h * D,
                                             pbuf.data_ptr() + 4 * col, pbuf.shape[1], st), "nrx_cin_layer_fwd")

        def bwd(xprev=xprev, hp=hp, h=h, w=w, gxk=gxk, gxp=gxp, gw=gw, wsp=wsp, col=col):
            _lib.check(lib.nrx_cin_layer_bwd(xd.data_ptr(), m * D, off, m, D, ptr(xprev), hp * D, hp, w.data_ptr(), h, B, g.data_ptr() + 4 * col,
                                             g.shape[1], gxk.data_ptr(), h * D, ptr(gxp), hp * D, gx.data_ptr(), m * D, 0, gw.data_ptr(), wsp.data_ptr(),
                                             st), "nrx_cin_layer_bwd")
        fwd()
        layer_legs[f"layer{k + 1}_fwd"], layer_legs[f"layer{k + 1}_bwd"] = fwd, bwd
        xprev, col = xk, col + h
    for fn in layer_legs.values():
        fn()
    lt = timed(layer_legs, rounds, iters)
    line["layers_us"] = {}
    for k, f in enumerate(flop):
        for leg, gemms in (("fwd", 1), ("bwd", 3)):
            med = statistics.median(lt[f"layer{k + 1}_{leg}"])
            line["layers_us"][f"layer{k + 1}_{leg}"] = {"us": round(med, 1), "mfma_frac": round(gemms * f / MFMA_F32_PEAK / (med * 1e-6), 4)}
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cin.py measures on the GPU: none is visible")
    for B, m, D, sizes in SHAPES:
        line = run_shape(B, m, D, sizes, args.rounds, args.iters)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
