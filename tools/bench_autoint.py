#!/usr/bin/env python3
"""Time and peak memory of AutoInt's fused interacting layer (ops.interacting_layer) beside the same arithmetic composed from existing code,
on one GPU, in one process:
  fused    ops.interacting_layer: one nrx_autoint_layer_fwd per layer, one nrx_autoint_layer_bwd in the backward;
  math     ops.interacting_layer_math: stock PyTorch fp32 -- (a); it materialises q, k, v, r [B, F, C] and the weights [B, H, F, F];
  compose  one projection x W4^T with W4 = (Wq | Wk | Wv | Wres) [4 C, din] held as ONE parameter (nn.Linear(din, 4 C, bias=False)), ops.seq_attention on
           the q | k | v columns of its output read in place, the add and the ReLU -- (b), the bar;
  sdpa     the same with torch.nn.functional.scaled_dot_product_attention in fp32 -- (c).
Shapes: B = 65 536, F = 26, D = 16, 2 heads of 16 (the package's batch) and B = 8 192, F = 26, D = 64, 2 heads of 32; one layer and the stack of
three (din = D, then C), unscaled scores, the residual on.  Legs: forward (no autograd graph) and forward + backward (ends with the gradients
of x and of every weight).  Legs are warmed, then timed alternately (leg after leg within a round) over --rounds rounds of --iters calls each
between two device events; a line holds each leg's median over the rounds and its spread (max - min) / median.  For the fused legs,
`mfma_frac`: the matrix FLOP the kernels issue on useful elements -- per sample and layer 2 F din 4 C for the projections and 2 F^2 C per
attention GEMM (2 in the forward; the backward recomputes 3 projections and runs 7 attention GEMMs and 2 F 4 C din twice, for g_W and g_x) --
over the time at the 157 TFLOP/s fp32 matrix peak; `hbm_frac`: the bytes a layer must move (x and out in the forward; x, out, g_out, g_x in
the backward; row_lse in both) over the time at 8 TB/s.  Peak memory is the rise of the allocator's peak over one call of the leg.  One JSON
line per (shape, layers) on stdout, appended to --out if given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((65536, 26, 16, 2, 16), (8192, 26, 64, 2, 32))
MFMA_F32_PEAK = 157e12
HBM_PEAK = 8e12


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


def run_shape(B, F, D, H, hd, layers, rounds, iters):
    import torch
    from news_recsys_amd import ops

    dev = torch.device("cuda:0")
    C = H * hd
    gen = torch.Generator(device=dev).manual_seed(B + 100 * F + D + layers)
    x = (torch.randn(B, F * D, device=dev, generator=gen) * 0.5).requires_grad_(True)
    dins = [D] + [C] * (layers - 1)
    ws = [[(torch.randn(C, din, device=dev, generator=gen) / din ** 0.5).requires_grad_(True) for _ in range(4)] for din in dins]
    flat = [w for lw in ws for w in lw]
    w4 = [torch.cat([w.detach() for w in lw]).requires_grad_(True) for lw in ws]     # (b), (c): nn.Linear(din, 4 C).weight, one leaf per layer
    g = torch.randn(B, F * C, device=dev, generator=gen)

    def stack(layer, xin, wsets):
        h, din = xin, D
        for lw in wsets:
            h = layer(h, din, lw)
            din = C
        return h

    def fused(h, din, lw):
        return ops.interacting_layer(h, F, din, *lw, heads=H, scale=1.0)

    def math(h, din, lw):
        return ops.interacting_layer_math(h, F, din, *lw, heads=H, scale=1.0)

    def compose(h, din, w):
        y = h.view(B, F, din) @ w.t()                                    # [B, F, 4 C]: q | k | v | r
        return torch.relu(ops.seq_attention(y[..., :3 * C], H, scale=1.0) + y[..., 3 * C:]).reshape(B, F * C)

    def sdpa(h, din, w):
        y = h.view(B, F, din) @ w.t()
        q, k, v = y[..., :3 * C].view(B, F, 3, H, hd).permute(2, 0, 3, 1, 4)
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=1.0).transpose(1, 2).reshape(B, F, C)
        return torch.relu(o + y[..., 3 * C:]).reshape(B, F * C)

    forms = {"fused": fused, "math": math, "compose": compose, "sdpa": sdpa}
    legs = {}
    for name, layer in forms.items():
        params = w4 if name in ("compose", "sdpa") else ws               # the yardsticks' weights are ONE [4 C, din] parameter per layer
        leaves = w4 if name in ("compose", "sdpa") else flat
        frozen = [p.detach() if torch.is_tensor(p) else [w.detach() for w in p] for p in params]

        def fwd(layer=layer, frozen=frozen):
            with torch.no_grad():
                return stack(layer, x.detach(), frozen)

        def fwdbwd(layer=layer, params=params, leaves=leaves):
            return torch.autograd.grad(stack(layer, x, params), [x] + leaves, g)
        legs[name + "_fwd"], legs[name + "_fwdbwd"] = fwd, fwdbwd
    # results agree before anything is timed: forward and every gradient of every form against the float64 math form, in batch chunks.  The
    # forward is held to 1e-5 of the largest value.  The gradients are not continuous: a pre-activation within fp32 rounding of 0 switches one
    # element's gradient on or off, and among the batch's B F C pre-activations per layer some are -- in a stack the switched element's whole
    # contribution then reaches the sample's g_x through the layers below --; so the gradients are held in the Frobenius norm, to 1e-2 of the
    # reference's (tests/test_autoint_gpu.py holds every element to derived bounds under the kernel's own mask).
    want, wgrads = [], None
    for c in range(0, B, 8192):
        xs = x.detach()[c:c + 8192].double().requires_grad_(True)
        wd = [[w.detach().double().requires_grad_(True) for w in lw] for lw in ws]
        o = stack(lambda h, din, lw: ops.interacting_layer_math(h, F, din, *lw, heads=H, scale=1.0), xs, wd)
        gr = torch.autograd.grad(o, [xs] + [w for lw in wd for w in lw], g[c:c + 8192].double())
        want.append((o.detach(), gr[0]))
        wgrads = list(gr[1:]) if wgrads is None else [a + b for a, b in zip(wgrads, gr[1:])]
    ref = [torch.cat([w[0] for w in want]), torch.cat([w[1] for w in want])] + wgrads
    agree = {}
    skipped = {}
    for name in list(forms):
        try:
            got = [legs[name + "_fwd"]()] + list(legs[name + "_fwdbwd"]())
            if name in ("compose", "sdpa"):                               # (their one gradient per layer, split for the comparison only)
                got = got[:2] + [part for gw in got[2:] for part in gw.split(C)]
        except RuntimeError as e:                                         # a yardstick that does not take the shape is reported, not timed
            if name == "fused":
                raise
            skipped[name] = str(e).splitlines()[0][:200]
            del legs[name + "_fwd"], legs[name + "_fwdbwd"]
            continue
        agree[name] = [float((got[0].double() - ref[0]).abs().max() / ref[0].abs().max())]
        agree[name] += [float((a.double() - b).norm() / b.norm()) for a, b in zip(got[1:], ref[1:])]
        assert agree[name][0] <= 1e-5 and max(agree[name][1:]) <= 1e-2, (name, agree[name])
        del got
    del want, wgrads, ref
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
    att = 2.0 * F * F * C
    flop_f = sum(2.0 * F * din * 4 * C + 2 * att for din in dins) * B
    flop_b = sum(2.0 * F * din * 3 * C + 7 * att + 2 * 2.0 * F * 4 * C * din for din in dins) * B
    bytes_f = sum(4.0 * (F * din + F * C + H * F) for din in dins) * B
    bytes_b = sum(4.0 * (2 * F * din + 2 * F * C + H * F) for din in dins) * B
    line = {"B": B, "F": F, "D": D, "heads": H, "head_dim": hd, "layers": layers, "rounds": rounds, "iters": iters,
            "max_err_vs_float64": {k: [float(f"{e:.2e}") for e in (v[0], max(v[1:]))] for k, v in agree.items()}}
    if skipped:
        line["skipped"] = skipped
    for name in legs:
        med = statistics.median(times[name])
        line[name] ={"us": round(med, 1), "spread": round((max(times[name]) - min(times[name])) / med, 3), "peak_mb": round(peak[name] / 1e6, 1)}
        if name.startswith("fused"):
            both = name.endswith("fwdbwd")
            line[name]["mfma_frac"] = round((flop_f + flop_b if both else flop_f) / MFMA_F32_PEAK / (med * 1e-6), 4)
            line[name]["hbm_frac"] = round((bytes_f + bytes_b if both else bytes_f) / HBM_PEAK / (med * 1e-6), 4)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_autoint.py measures on the GPU: none is visible")
    for B, F, D, H, hd in SHAPES:
        for layers in (1, 3):
            line = run_shape(B, F, D, H, hd, layers, args.rounds, args.iters)
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
