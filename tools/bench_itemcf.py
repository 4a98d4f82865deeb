#!/usr/bin/env python3
"""Time of the two ItemCF ops (ops.itemcf_similarity, ops.itemcf_recall; csrc/nrx_itemcf.hip) on two synthetic shapes:
  reference   the reference's data size: 6 040 users, 3 706 items, about 0.9 M interactions, Zipf item popularity; recall of every user,
              k = 10.  In the same run, on the same GPU, the stock-PyTorch form: a dense 0/1 A, A.T @ A, the elementwise normalisation, and
              torch.topk(H @ S) with the history masked.
  news        50 000 users, 65 536 items, histories of about 30 (a 17 GB sim); recall of the first 8 192 users.  The dense form cannot run it.
Per op the line holds the kernel-only time (the bare launch over prepared buffers) and the whole op (with its torch plumbing: sort,
de-duplication, CSC, allocation), and what the algorithm needs, computed from the shapes: sum_u L_u^2 LDS adds and 4 I^2 bytes of sim written
for the similarity, 4 I sum_q L_q bytes of sim read for the recall, each over the kernel time and against the 8 TB/s HBM peak.  Legs are
warmed, then timed alternately over >= 3 rounds; a line holds each leg's median and (max - min) / median.  One JSON line per case.

Without --case the tool runs each case in a fresh child process under a time limit of its own and stops at the first one that fails:
    python tools/bench_itemcf.py --out profiles/itemcf_bench.jsonl
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

CASES = ("reference", "news")
HBM_PEAK = 8.0e12
K = 10


def _histories(n_users, n_items, mean_len, zipf, seed, dev):
    """CSR of synthetic histories: lengths log-normal around mean_len (at least 3), items drawn by Zipf popularity with replacement
    (the op de-duplicates; the numbers reported are those of the de-duplicated data)."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    lens = torch.exp(torch.randn(n_users, device=dev, generator=gen) * 0.9 - 0.405).mul_(mean_len).clamp_(3, n_items // 2).long()
    off = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    pop = 1.0 / (torch.arange(n_items, device=dev, dtype=torch.float64) + 1.0) ** zipf
    cdf = torch.cumsum(pop / pop.sum(), 0)
    draws = torch.rand(int(off[-1]), device=dev, generator=gen, dtype=torch.float64)
    rank = torch.searchsorted(cdf, draws).clamp_(max=n_items - 1)
    names = torch.randperm(n_items, device=dev, generator=gen)                 # popularity rank -> item index
    return off, names[rank]


def _time_legs(legs, rounds, iters):
    import torch
    for leg in legs.values():                   # warm every leg (code objects, allocator pools)
        leg()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(rounds):                     # alternate the legs inside every round
        for name, leg in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                leg()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / iters)
    return {name: (statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts)) for name, ts in times.items()}


def run_case(case, rounds, iters):
    import torch
    from news_recsys_amd import ops
    dev = torch.device("cuda:0")
    if case == "reference":
        U, I, mean_len, zipf, Q = 6040, 3706, 190, 0.9, 6040
    else:
        U, I, mean_len, zipf, Q = 50000, 65536, 32, 0.9, 8192
    raw_off, raw_items = _histories(U, I, mean_len, zipf, 1234 + U, dev)
    u_off, u_items, owner = ops._csr_pair((raw_off, raw_items), None, I, "bench")
    item_off, users, item_count = ops._itemcf_csc(u_items, owner, I)
    lens = (u_off[1:] - u_off[:-1]).double()
    sim = torch.empty((I, I), dtype=torch.float32, device=dev)
    h_off = u_off[:Q + 1].clone()
    h_items = u_items[:int(h_off[-1])].clone()
    out_idx = torch.empty((Q, K), dtype=torch.int64, device=dev)
    out_score = torch.empty((Q, K), dtype=torch.float32, device=dev)
    ws = torch.empty(ops.itemcf_recall_workspace(I, Q, K, 0), dtype=torch.uint8, device=dev)
    ops._itemcf_similarity_launch(u_off, u_items, item_off, users, I, sim)

    legs = {
        "similarity_kernel": lambda: ops._itemcf_similarity_launch(u_off, u_items, item_off, users, I, sim),
        "similarity_op": lambda: ops.itemcf_similarity(raw_off, raw_items, I),
        "recall_kernel": lambda: ops._itemcf_recall_launch(sim, h_off, h_items, h_off, h_items, K, 0, out_idx, out_score, ws),
        "recall_op": lambda: ops.itemcf_recall(sim, (h_off, h_items), K),
    }
    line = {"tool": "bench_itemcf", "case": case, "users": U, "items": I, "interactions": int(u_items.numel()), "queries": Q, "k": K,
            "rounds": rounds, "iters": iters, "device": torch.cuda.get_device_name(0),
            "density": round(u_items.numel() / (U * I), 6), "max_item_users": int(item_count.max()), "max_user_items": int(lens.max())}
    if case == "reference":
        A = torch.zeros((U, I), dtype=torch.float32, device=dev)
        A[owner, u_items] = 1.0
        H = A[:Q]

        def torch_similarity():
            C = A.t() @ A
            n = torch.diagonal(C).clone()
            S = C / torch.sqrt(n[:, None] * n[None, :]).clamp_(min=1.0)
            S.fill_diagonal_(0.0)
            return S

        S = torch_similarity()

        def torch_recall():
            scores = (H @ S).masked_fill_(H != 0, float("-inf"))
            return torch.topk(scores, K, dim=1)

        legs["torch_similarity"] = torch_similarity
        legs["torch_recall"] = torch_recall
        line["torch_sim_max_rel_diff"] = float(((S - sim).abs() / sim.clamp(min=1e-30)).max())
    res = _time_legs(legs, rounds, iters)
    if case == "reference":
        # agreement of the two recall forms: the share of (query, slot) entries that name the same item (fp32 sums in another order: ties
        # and last-bit neighbours may swap)
        legs["recall_kernel"]()
        ti = torch_recall().indices
        line["torch_recall_same_items"] = round(float((ti == out_idx).double().mean()), 6)
    for name, (med, spread) in res.items():
        line[name + "_ms"] = round(med, 4)
        line[name + "_spread"] = round(spread, 4)
    adds = float((lens * lens).sum())
    sim_bytes = 4.0 * I * I
    read_bytes = 4.0 * I * float(lens[:Q].sum())
    ts, tr = res["similarity_kernel"][0] * 1e-3, res["recall_kernel"][0] * 1e-3
    line.update({"sum_len_sq": adds, "lds_adds_per_s": round(adds / ts, 1), "sim_bytes_written": sim_bytes,
                 "similarity_write_bytes_per_s": round(sim_bytes / ts, 1), "similarity_write_share_of_hbm_peak": round(sim_bytes / ts / HBM_PEAK, 4),
                 "recall_sim_bytes_read": read_bytes, "recall_read_bytes_per_s": round(read_bytes / tr, 1),
                 "recall_read_over_hbm_peak": round(read_bytes / tr / HBM_PEAK, 4)})
    if case == "reference":
        line["similarity_kernel_over_torch"] = round(res["similarity_kernel"][0] / res["torch_similarity"][0], 4)
        line["recall_kernel_over_torch"] = round(res["recall_kernel"][0] / res["torch_recall"][0], 4)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=CASES, default=None, help="run this case in this process")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one case's child process, seconds")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.case is not None:
        text = json.dumps(run_case(args.case, args.rounds, args.iters))
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        return 0
    for case in CASES:                          # a fresh process per case, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case,
               "--rounds", str(args.rounds), "--iters", str(args.iters)] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"case {case} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
