#!/usr/bin/env python3
"""Forward + backward time of the fused candidate softmax loss (ops.candidate_softmax: B rows against N = B + E candidates with a column
bias) at d = 16, in two cases:
  flagship      B = 65 536: the new op with E in {0, 8 192, 65 536}, with and without a bias, and ops.inbatch_softmax in the same run.  The
                E = 0, no-bias leg is meant to be the in-batch op's own instruction stream: the line says whether it is slower than the old op
                by more than the larger of the two legs' spreads.  Every leg also reports its time per 32 x 32 tile of the three passes.
  materialised  B = 4 096, E = 8 192: the new op beside torch's materialised [B, N] form (logits + bias, masked logsumexp), with peak memory.
Every leg starts from L2-normalised tower outputs (requires_grad) and ends with their gradients.  Legs are warmed, then timed alternately over
>= 3 rounds; a line holds each leg's median and (max - min) / median.  One JSON line per case, appended to --out.

Without --case the tool runs each case in a fresh child process under a time limit of its own and stops at the first one that fails:
    python tools/bench_candidate_softmax.py --out profiles/candidate_softmax_lines.jsonl
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

CASES = ("flagship", "materialised")
DIM = 16
TEMPERATURE = 0.1


def _inputs(B, E, dev):
    import torch
    import torch.nn.functional as F
    N = B + E
    gen = torch.Generator(device=dev).manual_seed(B + E)
    u = F.normalize(torch.randn(B, DIM, device=dev, generator=gen), dim=1).requires_grad_(True)
    v = F.normalize(torch.randn(N, DIM, device=dev, generator=gen), dim=1).requires_grad_(True)
    ids = torch.randint(0, max(2, N // 4), (N,), device=dev, generator=gen)
    # a logQ-shaped bias: -log of Zipf frequencies, some +-10 wide
    bias = -torch.log(1.0 / (1.0 + torch.randint(0, 20000, (N,), device=dev, generator=gen).float()))
    bias = (bias - bias.mean()).contiguous()
    mask = (torch.rand(B, device=dev, generator=gen) < 0.9).float()
    return u, v, ids, bias, mask


def _time_legs(legs, rounds, iters, slow=()):
    import torch
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
            n = iters if name not in slow else max(2, iters // 4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                leg()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / n)
    out = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = (med, (max(ts) - min(ts)) / med, int(peak[name]))
    return out


def run_flagship(rounds, iters, batch):
    import torch
    from news_recsys_amd import ops
    dev = torch.device("cuda:0")
    B = batch
    legs, shapes = {}, {}
    keep = []
    for E in (0, B // 8, B):
        u, v, ids, bias, mask = _inputs(B, E, dev)
        keep.append((u, v, ids, bias, mask))

        def leg(u=u, v=v, ids=ids, mask=mask, b=None):
            loss = (ops.candidate_softmax(u, v, temperature=TEMPERATURE, ids=ids, col_bias=b) * mask).mean()
            return torch.autograd.grad(loss, (u, v))

        legs[f"cand_e{E}"] = leg
        legs[f"cand_e{E}_bias"] = (lambda leg=leg, bias=bias: leg(b=bias))
        shapes[f"cand_e{E}"] = shapes[f"cand_e{E}_bias"] = B + E
        if E == 0:
            def old(u=u, v=v, ids=ids, mask=mask):
                loss = (ops.inbatch_softmax(u, v, temperature=TEMPERATURE, item_ids=ids) * mask).mean()
                return torch.autograd.grad(loss, (u, v))
            legs["inbatch"] = old
            shapes["inbatch"] = B
            same = all(torch.equal(a, b) for a, b in zip(leg(), old()))
    res = _time_legs(legs, rounds, iters)
    line = {"tool": "bench_candidate_softmax", "case": "flagship", "batch": B, "dim": DIM, "temperature": TEMPERATURE, "rounds": rounds,
            "iters": iters, "device": torch.cuda.get_device_name(0), "cand_e0_equals_inbatch_bits": bool(same)}
    for name, (med, spread, peak) in res.items():
        tiles = 3 * ((B + 31) // 32) * ((shapes[name] + 31) // 32)          # forward, dU and dV each visit every tile once
        line[name + "_ms"] = round(med, 4)
        line[name + "_spread"] = round(spread, 4)
        line[name + "_ns_per_tile"] = round(med * 1e6 / tiles, 4)
        line[name + "_peak_bytes"] = peak
    allowed = max(res["cand_e0"][1], res["inbatch"][1])
    line["cand_e0_over_inbatch"] = round(res["cand_e0"][0] / res["inbatch"][0], 4)
    line["allowed_excess"] = round(allowed, 4)
    line["cand_e0_within_spread_of_inbatch"] = bool(res["cand_e0"][0] <= res["inbatch"][0] * (1.0 + allowed))
    for name in shapes:
        if name not in ("cand_e0", "inbatch"):
            line[name + "_tile_time_over_e0"] = round(line[name + "_ns_per_tile"] / line["cand_e0_ns_per_tile"], 4)
    return line


def run_materialised(rounds, iters, batch):
    import torch
    from news_recsys_amd import ops
    dev = torch.device("cuda:0")
    B, E = batch, 2 * batch
    N = B + E
    u, v, ids, bias, mask = _inputs(B, E, dev)

    def fused():
        loss = (ops.candidate_softmax(u, v, temperature=TEMPERATURE, ids=ids, col_bias=bias) * mask).mean()
        return torch.autograd.grad(loss, (u, v))

    def materialised():
        z = u @ v.t() / TEMPERATURE + bias[None, :]
        excl = (ids[:B, None] == ids[None, :]) & ~torch.eye(B, N, dtype=torch.bool, device=dev)
        z = z.masked_fill(excl, float("-inf"))
        rows = torch.logsumexp(z, dim=1) - z.diagonal()
        return torch.autograd.grad((rows * mask).mean(), (u, v))

    res = _time_legs({"fused": fused, "materialised": materialised}, rounds, iters, slow=("materialised",))
    agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused(), materialised()))
    line = {"tool": "bench_candidate_softmax", "case": "materialised", "batch": B, "extra": E, "dim": DIM, "temperature": TEMPERATURE,
            "rounds": rounds, "iters": iters, "device": torch.cuda.get_device_name(0), "fused_vs_materialised_max_rel_grad_diff": agree,
            "one_b_by_n_fp32_bytes": B * N * 4}
    for name, (med, spread, peak) in res.items():
        line[name + "_ms"] = round(med, 4)
        line[name + "_spread"] = round(spread, 4)
        line[name + "_peak_bytes"] = peak
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=CASES, default=None, help="run this case in this process")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None, help="B of the case (default: 65536 flagship, 4096 materialised)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one case's child process, seconds")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.case is not None:
        line = (run_flagship(args.rounds, args.iters, args.batch or 65536) if args.case == "flagship"
                else run_materialised(args.rounds, args.iters, args.batch or 4096))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        return 0
    for case in CASES:                          # a fresh process per case, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case,
               "--rounds", str(args.rounds), "--iters", str(args.iters)] + (["--out", args.out] if args.out else []) \
              + (["--batch", str(args.batch)] if args.batch else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"case {case} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
