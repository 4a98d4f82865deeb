"""The shapes and masks the target-attention pooling is checked at: one list, shared by the CPU check of ops.din_pool_math and
the GPU check of ops.din_pool, so both are held to the same float64 reference (tests/din_pool_ref.py) at the same inputs.

A case crosses one value of each line (not the full product); every value of every line occurs:
    L in {1, 2, 3, 15, 16, 17, 50, 63, 64, 65, 255, 256}     -- around the rows in flight per step (64 / 32 / 16 / 8 / 4) and the 64-entry id words
    D in {4, 8, 12, 16, 20, 32, 64}                          -- every lane group (1, 2, 4, 8, 16 lanes per row) and the padded ones (12, 20)
    B in {1, 2, 5, 67}                                       -- less than a workgroup's 4 waves, more than one workgroup
    int32 / int64 ids, fp32 / bf16 table of 97 rows (rows repeat inside a sample and across samples)
    mask: none | prefix lengths 0, 1 and L in one batch | holes | non-binary weights | kept entries with id 0"""
import numpy as np
import torch

LS = (1, 2, 3, 15, 16, 17, 50, 63, 64, 65, 255, 256)
DS = (4, 8, 12, 16, 20, 32, 64)
BS = (1, 2, 5, 67)
MASKS = ("none", "prefix", "holes", "weights", "zero_ids")
ROWS = 97
N_CASES = 24


def case_params(i):
    return dict(L=LS[i % 12], D=DS[i % 7], B=BS[(i + i // 12) % 4], idx64=bool(i % 2), bf16=bool((i // 2) % 2), mask=MASKS[i % 5])


def case_id(i):
    c = case_params(i)
    return f"L{c['L']}-D{c['D']}-B{c['B']}-{'i64' if c['idx64'] else 'i32'}-{'bf16' if c['bf16'] else 'fp32'}-{c['mask']}"


def bf16_round(a):
    """fp32 array rounded to bf16 and widened again (what a bf16 table holds)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def make_case(i, amp=1.0, **over):
    """Numpy inputs of case i: table [97, D] fp32 (bf16-representable when the case's table is bf16; row 0 zero), ids [B, L], mask or None,
    query and g_out [B, D], scale.  over: parameters of case_params to replace (B=..., bf16=..., mask=...): the same generator at another
    batch size or crossing."""
    c = case_params(i)
    assert set(over) <= set(c), over
    c.update(over)
    L, D, B = c["L"], c["D"], c["B"]
    rng = np.random.default_rng(1000 + i)
    table = (rng.standard_normal((ROWS, D)) * amp).astype(np.float32)
    table[0] = 0
    if c["bf16"]:
        table = bf16_round(table)
    ids = rng.integers(1, ROWS, (B, L))
    mask = None
    if c["mask"] == "prefix":
        lens = np.array([(0, 1, L)[(b + i) % 3] if b < 3 else rng.integers(0, L + 1) for b in range(B)])
        mask = (np.arange(L)[None] < lens[:, None]).astype(np.float32)
        ids = ids * mask.astype(np.int64)                          # padding ids are 0, as the loader leaves them
    elif c["mask"] == "holes":
        mask = (rng.random((B, L)) < 0.6).astype(np.float32)       # masked entries keep their (ignored) ids
    elif c["mask"] == "weights":
        mask = np.where(rng.random((B, L)) < 0.7, rng.choice([0.5, -2.0, 1e-30, 3.0], (B, L)), 0.0).astype(np.float32)
    elif c["mask"] == "zero_ids":
        mask = np.ones((B, L), dtype=np.float32)
        ids = np.where(rng.random((B, L)) < 0.4, 0, ids)
    query = (rng.standard_normal((B, D)) * amp).astype(np.float32)
    g_out = rng.standard_normal((B, D)).astype(np.float32)
    c.update(table=table, ids=ids.astype(np.int64 if c["idx64"] else np.int32), mask_arr=mask, query=query, g_out=g_out, scale=float(D) ** -0.5)
    return c
