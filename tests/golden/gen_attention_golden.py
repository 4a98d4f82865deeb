#!/usr/bin/env python3
"""Regenerates the attention fixture from the reference's own Python (src/model/model_utils/utils.py of the checkout named by
NRX_REFERENCE_DIR, loaded by path: the file needs nothing but torch; the suite never runs this script and needs no checkout):

    NRX_REFERENCE_DIR=<checkout> python tests/golden/gen_attention_golden.py          # rewrites tests/golden/data/attention.npz
    NRX_REFERENCE_DIR=<checkout> python tests/golden/gen_attention_golden.py --check  # regenerates into a temp dir, compares bit for bit

Four cases (CASES below): the reference's MultiHeadSelfAttention and TransformerBlock at two sizes each, fp32 on the CPU, one thread.
Per case `<name>`:
    <name>/sd/<key>     every entry of the module's state_dict (default initialisation under torch.manual_seed(seed))
    <name>/x            the input [B, N, embed_dim] (standard normal)
    <name>/out          module(x)
    <name>/g            a random upstream gradient of out's shape
    <name>/grad_x       d sum(out * g) / d x
    <name>/grad/<key>   the same for every parameter
Data only.  (The npz sits under data/: gen_golden.py --check treats every npz directly under tests/golden/ as its own.)"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NRX_REFERENCE_DIR", "")
FILE = "attention.npz"
# name, class, embed_dim, heads, ff_dim, B, N, seed
CASES = (("mhsa_16x2", "MultiHeadSelfAttention", 16, 2, None, 3, 7, 101),
         ("mhsa_32x4", "MultiHeadSelfAttention", 32, 4, None, 2, 50, 102),
         ("block_16x2", "TransformerBlock", 16, 2, 32, 3, 7, 103),
         ("block_32x4", "TransformerBlock", 32, 4, 64, 2, 50, 104))


def reference_module():
    path = os.path.join(REF, "src", "model", "model_utils", "utils.py")
    spec = importlib.util.spec_from_file_location("reference_model_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def generate(out_dir):
    ref = reference_module()
    torch.set_num_threads(1)
    arrays = {}
    for name, cls, dim, heads, ff, B, N, seed in CASES:
        torch.manual_seed(seed)
        module = getattr(ref, cls)(dim, heads) if ff is None else getattr(ref, cls)(dim, heads, ff)
        module.eval()
        x = torch.randn(B, N, dim, requires_grad=True)
        g = torch.randn(B, N, dim)
        out = module(x)
        (out * g).sum().backward()
        for key, value in module.state_dict().items():
            arrays[f"{name}/sd/{key}"] = value.detach().numpy().copy()
        for key, p in module.named_parameters():
            arrays[f"{name}/grad/{key}"] = p.grad.numpy().copy()
        arrays[f"{name}/x"] = x.detach().numpy().copy()
        arrays[f"{name}/out"] = out.detach().numpy().copy()
        arrays[f"{name}/g"] = g.numpy().copy()
        arrays[f"{name}/grad_x"] = x.grad.numpy().copy()
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, FILE), **arrays)


def differences(a_dir, b_dir):
    a, b = np.load(os.path.join(a_dir, FILE)), np.load(os.path.join(b_dir, FILE))
    if sorted(a.files) != sorted(b.files):
        return [FILE + ": key sets differ"]
    return [f"{FILE}:{k}" for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]


if __name__ == "__main__":
    if not REF or not os.path.isdir(REF):
        sys.exit("set NRX_REFERENCE_DIR to a checkout of the reference project")
    data = os.path.join(HERE, "data")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            generate(tmp)
            bad = differences(data, tmp)
        if bad:
            sys.exit("the attention fixture differs from a regeneration:\n  " + "\n  ".join(bad))
        print("OK: a regeneration reproduces the committed attention fixture bit for bit")
    else:
        generate(data)
        print("attention fixture written")
