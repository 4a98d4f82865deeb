"""float64 restatement of the pairwise dot-product interaction (include/nrx_embed.h, nrx_dot_interact_fwd / _bwd), its derived error
bounds, and the launch-shape cases the CPU and GPU tests share.  numpy only; held to torch float64 autograd by tests/test_dot_interact_ref.py.

Bounds (u = 2^-24; both results are ONE fp32 fma chain from 0, so n terms give at most n roundings, each of relative size u on a partial sum that
the sum of the terms' magnitudes bounds; 2^-126 per term covers a product that leaves the normal range):
  forward : |z_ij - ref| <= D u sum_k |e_ik e_jk| + 2^-126 D
  backward: |g_e_f[c] - ref| <= (F + 2) u sum_j |S_fj e_j[c]| + 2^-126 F      (F + 1 chain terms when F is odd, one more for S = 2 g on the
            diagonal, which is exact -- so F + 2 is generous by one); accumulating adds one rounding of the sum: + u |up + ref|"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


def n_pairs(F, self_i=False):
    return F * (F + 1) // 2 if self_i else F * (F - 1) // 2


def pair_index(F, self_i=False):
    """(i, j) of every pair column, in the order of the definition: z[i (i - 1) / 2 + j], j < i (with the diagonal: i (i + 1) / 2 + j, j <= i)."""
    ii, jj = [], []
    for i in range(F):
        for j in range(i + 1 if self_i else i):
            ii.append(i)
            jj.append(j)
    return np.asarray(ii, np.int64), np.asarray(jj, np.int64)


def fields(x, offs, dim):
    """x [B, W] -> E [B, F, dim] float64."""
    x = np.asarray(x, np.float64)
    return np.stack([x[:, o:o + dim] for o in offs], axis=1)


def fwd(x, offs, dim, self_i=False):
    """(z [B, P] float64, its bound [B, P])."""
    E = fields(x, offs, dim)
    i, j = pair_index(len(offs), self_i)
    prod = E[:, i, :] * E[:, j, :]
    return prod.sum(-1), dim * U * np.abs(prod).sum(-1) + TINY * dim


def s_matrix(g_z, F, self_i=False):
    """S = G + G^T [B, F, F] float64, G the lower triangle of g_z (the diagonal counts twice)."""
    g_z = np.asarray(g_z, np.float64)
    i, j = pair_index(F, self_i)
    G = np.zeros((g_z.shape[0], F, F))
    G[:, i, j] = g_z
    return G + G.transpose(0, 2, 1)


def bwd(x, offs, dim, g_z, self_i=False, up=None):
    """(g_e [B, F, dim] float64 -- plus `up` [B, F, dim] when accumulating --, its bound)."""
    E = fields(x, offs, dim)
    F = len(offs)
    S = s_matrix(g_z, F, self_i)
    g = np.einsum("bfj,bjc->bfc", S, E)
    mag = np.einsum("bfj,bjc->bfc", np.abs(S), np.abs(E))
    bound = (F + 2) * U * mag + TINY * F
    if up is not None:
        g = g + np.asarray(up, np.float64)
        bound = bound + U * np.abs(g)
    return g, bound


# ---------------------------------------------------------------------------------------------------------- the launch-shape cases
# F: 2 (one pair), 3, 15 / 16 / 17 (around half a tile), 26 (the DeepFM shape), 31 / 32 (one tile, full), 33 (first field of the second tile row),
#    40, 63 / 64 (three tiles, full).  D: 4 and 12, 20 (8-byte loads, 1 / 3 / 5 of them), 8, 16, 32, 64 (16-byte loads, 1 / 2 / 4 / 8), 64 = two
#    column tiles in the backward.  Every F at D = 16, every D at F in {3, 26, 33}, and the corners.
FS = [2, 3, 15, 16, 17, 26, 31, 32, 33, 40, 63, 64]
DS = [4, 8, 12, 16, 20, 32, 64]
SHAPES = [(F, 16) for F in FS] + [(F, D) for F in (3, 26, 33) for D in DS if D != 16] + [(2, 4), (2, 64), (64, 4), (64, 64)]
BATCHES = [1, 2, 5, 67]
FIELD_LAYOUTS = ["adjacent", "permuted", "interleaved", "padded"]
Z_LAYOUTS = ["own", "odd", "cat", "wide"]
WRAP_BATCH = 4 * 2048 + 3          # one batch just past the launch's resident waves (2048 workgroups of 4): the sample loop wraps


def layout(F, D, kind, seed=0):
    """(offs, width): the fields' column offsets and the columns they span.  adjacent: f D.  permuted: the same columns in a shuffled order.
    interleaved: 4 or 8 foreign columns in front of every field (they hold sentinels), shuffled too.  padded: adjacent, 8 columns of row padding."""
    rng = np.random.default_rng(1000 + seed)
    if kind in ("adjacent", "padded"):
        return [f * D for f in range(F)], F * D + (8 if kind == "padded" else 0)
    if kind == "permuted":
        return [int(f) * D for f in rng.permutation(F)], F * D
    assert kind == "interleaved"
    offs, col = [], 0
    for f in range(F):
        col += 4 * int(rng.integers(1, 3))
        offs.append(col)
        col += D
    return [offs[int(f)] for f in rng.permutation(F)], col


def cases():
    """One dict per launch-shape case: every (F, D) of SHAPES once, the batch, field layout, z layout and flag cycling with co-prime periods so
    that every value of each meets many of the others; then every field layout x z layout x flag at one small shape."""
    out = []
    for n, (F, D) in enumerate(SHAPES):
        out.append(dict(F=F, D=D, B=BATCHES[n % 4], fields=FIELD_LAYOUTS[(n // 2 + n) % 4], z=Z_LAYOUTS[(n // 3 + 2 * n) % 4], self_i=bool((n // 5 + n) % 2)))
    for fl in FIELD_LAYOUTS:
        for zl in Z_LAYOUTS:
            for self_i in (False, True):
                out.append(dict(F=5, D=8, B=3, fields=fl, z=zl, self_i=self_i))
    return out


def case_id(c):
    return f"F{c['F']}-D{c['D']}-B{c['B']}-{c['fields']}-z{c['z']}-{'self' if c['self_i'] else 'strict'}"


def case_data(c, seed=0, scale=1.0):
    """(offs, width, e [B, F, D] fp32, g_z [B, P] fp32, up [B, F, D] fp32) of a case, from its own seed."""
    rng = np.random.default_rng(seed + 7 * c["F"] + 131 * c["D"] + 1009 * c["B"])
    offs, width = layout(c["F"], c["D"], c["fields"], seed)
    e = (rng.standard_normal((c["B"], c["F"], c["D"])) * scale).astype(np.float32)
    g_z = rng.standard_normal((c["B"], n_pairs(c["F"], c["self_i"]))).astype(np.float32)
    up = rng.standard_normal((c["B"], c["F"], c["D"])).astype(np.float32)
    return offs, width, e, g_z, up


def place(e, offs, width, fill=np.nan):
    """x [B, width] fp32: field f of e at columns offs[f] .., `fill` everywhere else."""
    B, F, D = e.shape
    x = np.full((B, width), fill, np.float32)
    for f, o in enumerate(offs):
        x[:, o:o + D] = e[:, f]
    return x


# ---------------------------------------------------------------------------------------------------------- the header's fp32 chains, bit for bit
def _round_f32(fr):
    """An exact rational -> the nearest fp32 (ties to even; subnormals kept), as a Python float."""
    if fr == 0:
        return 0.0
    sign, fr = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()          # 2^(e - 1) <= fr < 2^(e + 1)
    if fr < Fraction(2) ** e:
        e -= 1                                                            # 2^e <= fr < 2^(e + 1)
    e = max(e, -126)
    q = fr / Fraction(2) ** (e - 23)                                      # the fp32 grid at this exponent has spacing 2^(e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * float(Fraction(n) * Fraction(2) ** (e - 23))


def fmaf(a, b, c):
    """fp32 fma: a * b + c exactly, rounded once."""
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fwd_chain(x, offs, dim, self_i=False):
    """z [B, P] fp32 by the chain include/nrx_embed.h spells out: acc = 0; for s < H = dim / 2: acc = fmaf(u[s], v[s], acc);
    acc = fmaf(u[H + s], v[H + s], acc).  Exact rational arithmetic, one rounding per fmaf (slow: for small shapes)."""
    x = np.asarray(x, np.float32)
    H = dim // 2
    ii, jj = pair_index(len(offs), self_i)
    z = np.zeros((x.shape[0], len(ii)), np.float32)
    for b in range(x.shape[0]):
        for p, (i, j) in enumerate(zip(ii, jj)):
            u, v = x[b, offs[i]:offs[i] + dim], x[b, offs[j]:offs[j] + dim]
            acc = 0.0
            for s in range(H):
                acc = fmaf(u[s], v[s], acc)
                acc = fmaf(u[H + s], v[H + s], acc)
            z[b, p] = acc
    return z


def bwd_chain(x, offs, dim, g_z, self_i=False, up=None):
    """g_e [B, F, dim] fp32 by the header's chain: acc = 0; for j = 0 .. F - 1: acc = fmaf(S[f][j], e_j[c], acc), S = G + G^T with the diagonal
    doubled (2 g is exact); accumulating: up + acc, rounded once."""
    x, g_z = np.asarray(x, np.float32), np.asarray(g_z, np.float32)
    F = len(offs)
    ii, jj = pair_index(F, self_i)
    out = np.zeros((x.shape[0], F, dim), np.float32)
    for b in range(x.shape[0]):
        S = np.zeros((F, F), np.float32)
        for p, (i, j) in enumerate(zip(ii, jj)):
            S[i, j] = S[j, i] = 2 * g_z[b, p] if i == j else g_z[b, p]
        for f in range(F):
            for c in range(dim):
                acc = 0.0
                for j in range(F):
                    acc = fmaf(S[f, j], x[b, offs[j] + c], acc)
                if up is not None:
                    acc = _round_f32(Fraction(float(up[b, f, c])) + Fraction(acc))
                out[b, f, c] = acc
    return out
