"""float64 restatement of the short-sequence self-attention (include/nrx_embed.h, nrx_attn_fwd / _bwd) and the error bounds its fp32
implementation is held to.  Not a test module: tests/test_attention*.py import it.

    qkv [B, N, 3 C], C = H hd: q of head h at columns h hd, k at C + h hd, v at 2 C + h hd;  key j of sample b is kept iff mask[b, j] != 0
    s_ij = dot(q_i, k_j) scale;  p_ij = softmax over the kept j;  out_i = sum_j p_ij v_j;  lse_i = log sum_kept exp(s_ij)
    a sample with no kept key: out = 0, lse = -inf, zero gradients
    delta_i = dot(g_i, out_i);  dV = P^T g;  dP = g V^T;  dS = P o (dP - delta);  dQ = scale dS K;  dK = scale dS^T Q

Bounds (EPS = 2^-24; per (sample, head)):  E_s = (hd + 2) EPS max|q_i| max|k_j| scale  -- what the fp32 chain of hd products and the scale
perturb a score by;  unit = E_s + (N + hd) EPS  -- the relative perturbation of one term of a sum of N products formed from such scores.
    |out - out64| <= unit (P |V|)                 |dV - dV64| <= unit (P^T |g|)
    T_ij = p_ij (|g_i| . |v_j| + |g_i| . (P |V|)_i):    |dQ - dQ64| <= unit scale (T |K|)        |dK - dK64| <= unit scale (T^T |Q|)
    |lse - lse64| <= 4 E_s + 8 EPS max(1, |lse|)
A sample with no kept key has bound 0: exact.
A relative bound holds only for what fp32 can hold: a p_ij below 2^-126 (s_ij - lse_i < -87: most pairs once scores reach +-1e4) is 0 in ANY
fp32 evaluation while float64 keeps it down to 1e-308, so a dK or dV row of a key no query attends to is, say, 8e-88 in float64 and 0 in fp32
-- off by all of its own magnitude, which no multiple of unit covers (fp32 torch itself sits at 70 times the relative bound there).  Each term
may therefore be off by 2^-126 times its weight as well: the bounds carry FLT_MIN (cap + 1), cap being the same sum of |terms| with every
p_ij replaced by 1 -- some 1e-33 absolute at the shapes tested, far below anything fp32 resolves (tests/inbatch_softmax_ref.py does the
same).  It is 0 for a sample with no kept key."""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
FLT_MIN = 2.0 ** -126          # smallest normal fp32: exp() below it flushes to zero


def attention_ref(qkv, heads, mask=None, scale=None, g_out=None):
    """All in float64 on the values handed in (fp32 inputs are widened exactly).  qkv [B, N, 3 C]; mask None or [B, N]; g_out None or
    [B, N, C].  Returns a namespace: out [B, N, C], lse [B, H, N], tol_out, tol_lse; with g_out also g_qkv [B, N, 3 C] (dQ | dK | dV in
    qkv's layout) and tol_g_qkv.  The tol_* arrays are the bounds of the module docstring, element for element."""
    qkv = np.asarray(qkv, dtype=np.float64)
    B, N, W = qkv.shape
    C = W // 3
    hd = C // heads
    scale = float(hd) ** -0.5 if scale is None else float(scale)
    keep = np.ones((B, N), dtype=bool) if mask is None else np.asarray(mask) != 0
    split = qkv.reshape(B, N, 3, heads, hd).transpose(2, 0, 3, 1, 4)        # [3, B, H, N, hd]
    q, k, v = split[0], split[1], split[2]
    s = np.einsum("bhie,bhje->bhij", q, k) * scale
    kj = keep[:, None, None, :]
    some = keep.any(axis=1)[:, None, None]                                    # [B, 1, 1]
    sm = np.where(kj, s, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(some, sm.max(axis=-1), 0.0)                              # [B, H, N]
        e = np.where(kj, np.exp(sm - m[..., None]), 0.0)
        den = e.sum(axis=-1)
        lse = np.where(some, m + np.log(den), -np.inf)
        p = np.where(some[..., None], e / np.where(den > 0, den, 1.0)[..., None], 0.0)
    o = p @ v                                                                  # [B, H, N, hd]
    abs_o = p @ np.abs(v)

    def merge(t):                                                              # [B, H, N, hd] -> [B, N, C]
        return t.transpose(0, 2, 1, 3).reshape(B, N, C)

    nq = np.sqrt((q ** 2).sum(axis=-1)).max(axis=-1)                           # [B, H]
    nk = np.sqrt((k ** 2).sum(axis=-1)).max(axis=-1)
    e_s = ((hd + 2) * EPS * nq * nk * abs(scale))[..., None]                   # [B, H, 1]
    unit = (e_s + (N + hd) * EPS)[..., None]                                   # [B, H, 1, 1]
    with np.errstate(invalid="ignore"):
        tol_lse = np.where(some, 4.0 * e_s + 8.0 * EPS * np.maximum(1.0, np.abs(lse)), 0.0)
    floor = FLT_MIN * some[..., None]                                           # [B, 1, 1, 1]: nothing for a sample with no kept key
    ones = np.ones_like(p)
    tol_out = unit * abs_o + floor * (ones @ np.abs(v) + 1.0)
    ref = SimpleNamespace(out=merge(o), lse=lse, tol_out=merge(tol_out), tol_lse=tol_lse, scale=scale, head_dim=hd)
    if g_out is not None:
        g = np.asarray(g_out, dtype=np.float64).reshape(B, N, heads, hd).transpose(0, 2, 1, 3)      # [B, H, N, hd]
        delta = (g * o).sum(axis=-1, keepdims=True)
        dp = np.einsum("bhie,bhje->bhij", g, v)
        ds = p * (dp - delta)
        dq = scale * (ds @ k)
        dk = scale * (ds.transpose(0, 1, 3, 2) @ q)
        dv = p.transpose(0, 1, 3, 2) @ g
        ag = np.abs(g)
        t = p * (np.einsum("bhie,bhje->bhij", ag, np.abs(v)) + (ag * abs_o).sum(axis=-1, keepdims=True))
        cap = np.einsum("bhie,bhje->bhij", ag, np.abs(v)) + (ag * (ones @ np.abs(v))).sum(axis=-1, keepdims=True)      # T with p = 1 throughout
        tol_dq = unit * abs(scale) * (t @ np.abs(k)) + floor * (abs(scale) * (cap @ np.abs(k)) + 1.0)
        tol_dk = unit * abs(scale) * (t.transpose(0, 1, 3, 2) @ np.abs(q)) + floor * (abs(scale) * (cap.transpose(0, 1, 3, 2) @ np.abs(q)) + 1.0)
        tol_dv = unit * (p.transpose(0, 1, 3, 2) @ ag) + floor * (ones.transpose(0, 1, 3, 2) @ ag + 1.0)
        ref.g_qkv = np.concatenate([merge(dq), merge(dk), merge(dv)], axis=-1)
        ref.tol_g_qkv = np.concatenate([merge(tol_dq), merge(tol_dk), merge(tol_dv)], axis=-1)
    return ref


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (an element of bound 0 must be exact: it counts as 0 when it is, inf when it is not)."""
    got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want))          # (-inf == -inf: exact)
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(np.where(np.isnan(r), np.inf, r).max()) if r.size else 0.0


def make_case(seed, B, N, H, hd, mask_kind="none", in_scale=1.0):
    """Seeded fp32 inputs of a case: qkv [B, N, 3 H hd] (standard normal times in_scale), g_out [B, N, H hd], mask (None or fp32 [B, N]).
    mask_kind: "none"; "prefix" -- prefix lengths N, 0, 1 for the first three samples, then random ones; "holes" -- random keys dropped in the middle,
    first and last kept; "weights" -- a prefix mask whose kept entries are non-binary weights (0.5, 2, -1: all count as kept)."""
    rng = np.random.default_rng(seed)
    C = H * hd
    qkv = (rng.standard_normal((B, N, 3 * C)) * in_scale).astype(np.float32)
    g_out = rng.standard_normal((B, N, C)).astype(np.float32)
    mask = None
    if mask_kind in ("prefix", "weights"):
        lens = np.array([(N, 0, 1)[b] if b < 3 else int(rng.integers(0, N + 1)) for b in range(B)])
        mask = (np.arange(N)[None, :] < lens[:, None]).astype(np.float32)
        if mask_kind == "weights":
            mask = mask * rng.choice(np.array([0.5, 2.0, -1.0], dtype=np.float32), size=(B, N))
    elif mask_kind == "holes":
        mask = (rng.random((B, N)) < 0.6).astype(np.float32)
        mask[:, 0] = 1.0
        mask[:, -1] = 1.0
    elif mask_kind != "none":
        raise ValueError(mask_kind)
    return qkv, g_out, mask


# (B, N, H, hd, mask_kind, in_scale): every shape tests/test_attention_gpu.py checks against the bounds; tests/test_attention_ref.py holds
# the fp32 torch restatement to 0.25 of the bound on each
_N_SWEEP = [(3, n, 2, 8, mk, 1.0) for n in (1, 2, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 127, 128) for mk in ("none", "prefix")]
_HD_SWEEP = [(3, 50, 2, hd, mk, 1.0) for hd in (4, 8, 12, 16, 32, 64) for mk in ("none", "prefix")]
_H_SWEEP = [(3, 33, h, 8, "holes", 1.0) for h in (1, 3, 4)]
_B_SWEEP = [(b, 17, 2, 8, "weights", 1.0) for b in (1, 2, 5, 67)]
_MASKS = [(4, 50, 2, 8, mk, 1.0) for mk in ("holes", "weights")] + [(4, 33, 3, 12, "prefix", 3.0), (2, 128, 1, 64, "holes", 1.0),
                                                                   (2, 64, 4, 4, "weights", 1.0), (2, 100, 2, 20, "prefix", 1.0)]
GPU_CASES = _N_SWEEP + _HD_SWEEP + _H_SWEEP + _B_SWEEP + _MASKS
# scores that reach +-1e4: |q| |k| scale ~ (60 * 60) * 8 * 8^-0.5
BIG_CASE = (3, 50, 2, 8, "prefix", 60.0)


def case_id(c):
    B, N, H, hd, mk, sc = c
    return f"B{B}-N{N}-H{H}-hd{hd}-{mk}" + ("" if sc == 1.0 else f"-x{sc:g}")
