#!/usr/bin/env python3
"""Forward + backward time of the fused in-batch softmax loss (ops.inbatch_softmax) beside what it replaces, at B in {4096, 16384, 65536}, d = 16:
  (a) the reference's sampled infoNCE loss in torch (DSSM.forward's gather of negative_sample_rate permutations + DSSM.infoNCE_loss), rates 1 and 4;
  (b) torch's materialised in-batch form ([B, B] logits, masked logsumexp) where it fits, with its peak memory beside it.
Every leg starts from the two L2-normalised [B, 16] tower outputs (requires_grad) and ends with their gradients; the fused op's forward, its
backward and each gradient launch alone are timed as legs of their own (fused_fwd, fused_bwd, fused_bwd_du, fused_bwd_dv).  Legs are warmed, then timed
alternately over >= 3 rounds; a line holds each leg's median and (max - min) / median.  One JSON line per size, appended to --out.

Without --size the tool runs each size in a fresh child process under a time limit of its own and stops at the first one that fails:
    python tools/bench_inbatch_softmax.py --out profiles/inbatch_softmax_lines.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (4096, 16384, 65536)
DIM = 16
TEMPERATURE = 0.1


def run_size(B, rounds, iters, out_path):
    import torch
    import torch.nn.functional as F
    from news_recsys_amd import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B)
    u = F.normalize(torch.randn(B, DIM, device=dev, generator=gen), dim=1).requires_grad_(True)
    v = F.normalize(torch.randn(B, DIM, device=dev, generator=gen), dim=1).requires_grad_(True)
    ids = torch.randint(0, max(2, B // 4), (B,), device=dev, generator=gen)
    mask = (torch.rand(B, device=dev, generator=gen) < 0.9).float()

    def fused():
        loss = (ops.inbatch_softmax(u, v, temperature=TEMPERATURE, item_ids=ids) * mask).mean()
        return torch.autograd.grad(loss, (u, v))

    def sampled(n_neg):
        def leg():
            neg = F.normalize(torch.stack([v[torch.randperm(B, device=dev)] for _ in range(n_neg)], dim=1), p=2, dim=-1)
            pos = torch.sum(u * v, dim=1) / TEMPERATURE
            ng = torch.bmm(u.unsqueeze(1), neg.permute(0, 2, 1)).squeeze(1) / TEMPERATURE
            logits = torch.cat([pos.unsqueeze(1), ng], dim=1)
            losses = F.cross_entropy(logits, torch.zeros(B, dtype=torch.long, device=dev), reduction="none")
            return torch.autograd.grad((losses * mask).mean(), (u, v))
        return leg

    def materialised():
        s = u @ v.t() / TEMPERATURE
        excl = (ids[:, None] == ids[None, :]) & ~torch.eye(B, dtype=torch.bool, device=dev)
        rows = torch.logsumexp(s.masked_fill(excl, float("-inf")), dim=1) - (u * v).sum(dim=1) / TEMPERATURE
        return torch.autograd.grad((rows * mask).mean(), (u, v))

    # the fused op's launches apart: the forward alone, and the backward of a kept graph -- both gradients (two launches of the one kernel),
    # dU alone (v needs no gradient: the dV launch is skipped) and dV alone
    g_rows = mask / B
    kept = {"both": ops.inbatch_softmax(u, v, temperature=TEMPERATURE, item_ids=ids),
            "du": ops.inbatch_softmax(u, v.detach(), temperature=TEMPERATURE, item_ids=ids),
            "dv": ops.inbatch_softmax(u.detach(), v, temperature=TEMPERATURE, item_ids=ids)}

    def fused_fwd():
        with torch.no_grad():
            return ops.inbatch_softmax(u, v, temperature=TEMPERATURE, item_ids=ids)

    def fused_bwd(which, wrt):
        return lambda: torch.autograd.grad(kept[which], wrt, g_rows, retain_graph=True)

    legs = {"fused": fused, "fused_fwd": fused_fwd, "fused_bwd": fused_bwd("both", (u, v)), "fused_bwd_du": fused_bwd("du", (u,)),
            "fused_bwd_dv": fused_bwd("dv", (v,)), "sampled_1": sampled(1), "sampled_4": sampled(4)}
    free, _ = torch.cuda.mem_get_info()
    need = 6 * B * B * 4                        # logits, masked copy, softmax, its gradient, the mask and slack
    if need < free // 2:
        legs["materialised"] = materialised
    peak = {}
    for name, leg in legs.items():              # warm every leg (code objects, allocator pools), and record its peak memory
        leg()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        leg()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    times = {name: [] for name in legs}
    for _ in range(rounds):                     # alternate the legs inside every round
        for name, leg in legs.items():
            n = iters if name != "materialised" else max(2, iters // 4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                leg()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / n)
    # the fused and the materialised form are the same function: say how far apart they are
    agree = None
    if "materialised" in legs:
        gf, gm = fused(), materialised()
        agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, gm))
    line = {"tool": "bench_inbatch_softmax", "batch": B, "dim": DIM, "temperature": TEMPERATURE, "rounds": rounds, "iters": iters,
            "device": torch.cuda.get_device_name(0), "materialised_skipped": "materialised" not in legs,
            "fused_vs_materialised_max_rel_grad_diff": agree}
    for name, ts in times.items():
        med = statistics.median(ts)
        line[name + "_ms"] = round(med, 4)
        line[name + "_spread"] = round((max(ts) - min(ts)) / med, 4)
        line[name + "_peak_bytes"] = int(peak[name])
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=None, help="run this batch size in this process")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one size's child process, seconds")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.size is not None:
        run_size(args.size, args.rounds, args.iters, args.out)
        return 0
    for B in SIZES:                             # a fresh process per size, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--size", str(B),
               "--rounds", str(args.rounds), "--iters", str(args.iters)] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"size {B} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
