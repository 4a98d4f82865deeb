"""float64 restatement of AutoInt's interacting layer (include/nrx_embed.h, nrx_autoint_layer_fwd / _bwd) with hand-written gradients
that take the ReLU mask as a parameter, its derived error bounds, and the launch-shape cases the CPU and GPU tests share.  numpy only; held to
torch float64 autograd of ops.interacting_layer_math by tests/test_autoint_ref.py.

Notation: x [B, F, din], W* [C, din], C = heads hd, FT = ceil(F / 32); u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability,
lemma 3.1: a chain of n roundings stays within gamma(n) of the sum of its terms' magnitudes).  Every bound below is a running error analysis:
the error of each intermediate is carried, as an array, into the next; a chain of n terms also gets n 2^-126 for products that underflow.

Forward.
  q, k, v, r : chains of din fmas                                    eq = gamma(din) |x| |Wq|^T, ...
  t_ij       : chain of hd fmas over computed q, k                   et = sum_c (eq |k| + |q| ek + eq ek) + gamma(hd) sum_c (|q| + eq) (|k| + ek)
  s_ij       : fl(scale t)                                           es = |scale| et + u |scale| (|t| + et)
  E_ij       : softmax is shift invariant, so the computed maximum m is a shift, not an error (it lies within max_j es of the true one).  The
               argument fl(s - m) carries es and one rounding (none if the compiler fuses scale t - m; the bound keeps it); expf of the device
               library is within 1 ulp, a relative 2^-23 = EXP_REL:
                                                                      eps_ij = expm1(es + u (|s - m| + 2 max_j es)) (1 + EXP_REL) + EXP_REL
  l_i        : positive terms, two half sums of 16 FT adds and one add: nl = 16 FT + 1
                                                                      eps_l = sum_j p eps + gamma(nl) (1 + sum_j p eps)
  o_i        : chain of 32 FT fmas of v_j E_ij, then fl(a / l) (the division within 1 ulp = 2 u):
               e_p = p ((1 + eps) (1 + 2 u) / (1 - eps_l) - 1);       e_o = sum_j (e_p |v| + (p + e_p) ev) + gamma(32 FT) sum_j (p + e_p) (|v| + ev)
  pre, out   : fl(o + r); relu is 1-Lipschitz                         e_pre = e_o + er + u (|pre| + e_o + er)
  row_lse    : fl(m + logf(l)), logf within 1 ulp                     e_lse = -log1p(-eps_l) + EXP_REL (|log l| + mes) + u (|lse| + |m| + |log l| + 2 mes),
               mes = max_j es (the shift the kernel used is within mes of the float64 one).
Backward (the mask is a parameter: dO = g_out where mask, exact; e_lse_in is the error of the row_lse buffer handed in).
  p_ij       : expf(fl(s - lse_in))                                   eps_b = expm1(es + e_lse_in + u (|s - lse| + es + e_lse_in)) (1 + EXP_REL) + EXP_REL,  e_p = p eps_b
  dP_ij      : chain of hd fmas of computed v and exact dO            e_dP = sum_c ev |dO| + gamma(hd) sum_c (|v| + ev) |dO|
  delta_i    : two half chains of 16 FT fmas and one add              e_dl = sum_j (e_p |dP| + p e_dP + e_p e_dP) + gamma(16 FT + 1) sum_j (p + e_p) (|dP| + e_dP)
  dS_ij      : fl(p fl(dP - delta)): the product rule, one rounding each
  dq, dk     : fl(scale chain of 32 FT fmas of dS and computed k (q)); dv: chain of 32 FT fmas of p and exact dO
  g_x        : one chain of nm C fmas of exact W and computed dM (nm = 4 with Wres, else 3)
  g_W        : slice s is one chain over its n_s = (samples in it) 2 ceil(F / 2) fmas of dM and exact x; the S partials are added in order:
               e_s = sum e_dM |x| + gamma(n_s) sum (|dM| + e_dM) |x|;   |err| <= sum_s e_s + gamma(S) sum_s (|part_s| + e_s)."""
import numpy as np

from tests.dot_interact_ref import layout, place  # noqa: F401  (the field layouts are shared)

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_REL = 2.0 ** -23
MAX_BLOCKS = 1024       # the bounded grid of the backward: one slice per workgroup (the forward's: 2048 workgroups of one sample)


def gamma(n):
    return n * U / (1.0 - n * U)


def wgrad_slice(F, din, heads, hd):
    """nrx_autoint_wgrad_slice: asserted by the GPU test."""
    return 16 if heads * hd * din > 1024 else 64


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _heads(a, heads):
    """[B, F, C] -> [B, heads, F, hd]"""
    B, F, C = a.shape
    return a.reshape(B, F, heads, C // heads).transpose(0, 2, 1, 3)


def _merge(a):
    """[B, heads, F, hd] -> [B, F, C]"""
    B, H, F, hd = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B, F, H * hd)


def forward(x, Wq, Wk, Wv, Wres, heads, scale, exp_rel=EXP_REL):
    """dict of the float64 forward and its bounds: q, k, v [B, H, F, hd] (+ eq, ek, ev), s, p [B, H, F, F], pre, out [B, F, C], lse [B, H, F], ..."""
    x, Wq, Wk, Wv, Wres = _f64(x), _f64(Wq), _f64(Wk), _f64(Wv), _f64(Wres)
    B, F, din = x.shape
    C = Wq.shape[0]
    hd = C // heads
    FT = -(-F // 32)
    ax = np.abs(x)
    proj = lambda W: (_heads(x @ W.T, heads), _heads(gamma(din) * (ax @ np.abs(W).T) + TINY * din, heads))  # noqa: E731
    (q, eq), (k, ek), (v, ev) = proj(Wq), proj(Wk), proj(Wv)
    aq, ak, av = np.abs(q), np.abs(k), np.abs(v)
    t = q @ k.transpose(0, 1, 3, 2)
    et = (eq @ ak.transpose(0, 1, 3, 2) + aq @ ek.transpose(0, 1, 3, 2) + eq @ ek.transpose(0, 1, 3, 2)
          + gamma(hd) * ((aq + eq) @ (ak + ek).transpose(0, 1, 3, 2)) + TINY * hd)
    s = scale * t
    es = abs(scale) * et + U * abs(scale) * (np.abs(t) + et) + TINY
    m = s.max(-1, keepdims=True)
    mes = es.max(-1, keepdims=True)
    E = np.exp(s - m)
    l = E.sum(-1, keepdims=True)
    p = E / l
    eps = np.expm1(es + U * (np.abs(s - m) + 2 * mes)) * (1 + exp_rel) + exp_rel
    mean_eps = (p * eps).sum(-1, keepdims=True)
    eps_l = mean_eps + gamma(16 * FT + 1) * (1 + mean_eps)
    e_p = p * ((1 + eps) * (1 + 2 * U) / (1 - eps_l) - 1)
    o = p @ v
    e_o = e_p @ av + (p + e_p) @ ev + gamma(32 * FT) * ((p + e_p) @ (av + ev)) + TINY * 32 * FT
    pre, e_pre = _merge(o), _merge(e_o)
    if Wres is not None:
        r, er = x @ Wres.T, gamma(din) * (ax @ np.abs(Wres).T) + TINY * din
        pre = pre + r
        e_pre = e_pre + er + U * (np.abs(pre) + e_pre + er) + TINY
    logl = np.log(l[..., 0])
    lse = m[..., 0] + logl
    e_lse = (-np.log1p(-eps_l[..., 0]) + exp_rel * (np.abs(logl) + mes[..., 0])
             + U * (np.abs(lse) + np.abs(m[..., 0]) + np.abs(logl) + 2 * mes[..., 0]))
    return dict(q=q, k=k, v=v, eq=eq, ek=ek, ev=ev, s=s, es=es, p=p, pre=pre, e_pre=e_pre, out=np.maximum(pre, 0.0), lse=lse, e_lse=e_lse)


def backward(x, Wq, Wk, Wv, Wres, heads, scale, g_out, mask=None, e_lse_in=None, slice_samples=None, exp_rel=EXP_REL):
    """((g_x [B, F, din], g_Wq, g_Wk, g_Wv, g_Wres or None) float64 by hand-written gradients under the ReLU mask `mask` [B, F, C] (None: the
    float64 pre-activation's own), (their bounds), the forward dict).  e_lse_in [B, H, F]: the error of the row_lse the kernel is handed
    (None: the forward's e_lse, the kernel's own buffer)."""
    f = forward(x, Wq, Wk, Wv, Wres, heads, scale, exp_rel)
    x, Wq, Wk, Wv, Wres = _f64(x), _f64(Wq), _f64(Wk), _f64(Wv), _f64(Wres)
    B, F, din = x.shape
    C = Wq.shape[0]
    hd = C // heads
    FT = -(-F // 32)
    SL = slice_samples or wgrad_slice(F, din, heads, hd)
    mask = (f["pre"] > 0) if mask is None else np.asarray(mask, bool).reshape(B, F, C)
    e_in = f["e_lse"] if e_lse_in is None else _f64(e_lse_in)
    dOm = _f64(g_out).reshape(B, F, C) * mask
    dO = _heads(dOm, heads)
    adO = np.abs(dO)
    q, k, v, eq, ek, ev, s, es, p = (f[n] for n in ("q", "k", "v", "eq", "ek", "ev", "s", "es", "p"))
    aq, ak, av = np.abs(q), np.abs(k), np.abs(v)
    lse = f["lse"][..., None]
    eps_b = np.expm1(es + e_in[..., None] + U * (np.abs(s - lse) + es + e_in[..., None])) * (1 + exp_rel) + exp_rel
    e_p = p * eps_b
    T = lambda a: a.transpose(0, 1, 3, 2)  # noqa: E731
    dP = dO @ T(v)
    e_dP = adO @ T(ev) + gamma(hd) * (adO @ T(av + ev)) + TINY * hd
    delta = (p * dP).sum(-1, keepdims=True)
    e_dl = ((e_p * np.abs(dP) + p * e_dP + e_p * e_dP).sum(-1, keepdims=True)
            + gamma(16 * FT + 1) * ((p + e_p) * (np.abs(dP) + e_dP)).sum(-1, keepdims=True) + TINY * 32 * FT)
    diff = dP - delta
    e_diff = e_dP + e_dl + U * (np.abs(diff) + e_dP + e_dl) + TINY
    dS = p * diff
    e_dS = e_p * (np.abs(diff) + e_diff) + p * e_diff + U * (p + e_p) * (np.abs(diff) + e_diff) + TINY
    adS = np.abs(dS)
    n = 32 * FT

    def scaled(inner, e_inner):
        return scale * inner, abs(scale) * e_inner + U * abs(scale) * (np.abs(inner) + e_inner) + TINY

    dq, e_dq = scaled(dS @ k, e_dS @ ak + adS @ ek + e_dS @ ek + gamma(n) * ((adS + e_dS) @ (ak + ek)) + TINY * n)
    dk, e_dk = scaled(T(dS) @ q, T(e_dS) @ aq + T(adS) @ eq + T(e_dS) @ eq + gamma(n) * (T(adS + e_dS) @ (aq + eq)) + TINY * n)
    dv = T(p) @ dO
    e_dv = T(e_p) @ adO + gamma(n) * (T(p + e_p) @ adO) + TINY * n
    dMs = [(_merge(dq), _merge(e_dq), Wq), (_merge(dk), _merge(e_dk), Wk), (_merge(dv), _merge(e_dv), Wv)]
    if Wres is not None:
        dMs.append((dOm, np.zeros_like(dOm), Wres))
    nm = len(dMs)
    gx = sum(dM @ W for dM, _, W in dMs)
    e_gx = (sum(e @ np.abs(W) for _, e, W in dMs) + gamma(nm * C) * sum((np.abs(dM) + e) @ np.abs(W) for dM, e, W in dMs) + TINY * nm * C)
    ax = np.abs(x)
    gW, eW = [], []
    for dM, e, _ in dMs:
        tot, esum, psum, S = np.zeros((C, din)), np.zeros((C, din)), np.zeros((C, din)), 0
        for b0 in range(0, B, SL):
            sl = slice(b0, min(b0 + SL, B))
            ns = (sl.stop - sl.start) * 2 * ((F + 1) // 2)
            part = np.einsum("bic,bid->cd", dM[sl], x[sl])
            err = np.einsum("bic,bid->cd", e[sl], ax[sl]) + gamma(ns) * np.einsum("bic,bid->cd", np.abs(dM[sl]) + e[sl], ax[sl]) + TINY * ns
            tot += part
            esum += err
            psum += np.abs(part) + err
            S += 1
        gW.append(tot)
        eW.append(esum + gamma(S) * psum)
    if Wres is None:
        gW.append(None)
        eW.append(None)
    return (gx, *gW), (e_gx, *eW), f


# ---------------------------------------------------------------------------------------------------------- the launch-shape cases
# (F, din, heads, hd, B).  F over {2, 3, 31, 32, 33, 64} (around the 32-row tile) and 26; din over {4, 12, 16, 64}; heads x hd over 1x4, 3x4, 2x12,
# 2x16, 1x64, 4x16 (one head, an odd count, a width that does not divide 64, the widest head, the largest C); B over {1, 2, 3, 5, 67} and the
# weight-gradient slices (64 samples, 16 where C din > 1024): exactly one, one + 1 sample, several.  A workgroup owns one sample at a time, so
# "samples per workgroup +- 1" is B = 1 and 2.
SHAPES = [
    (2, 4, 1, 4, 1), (2, 12, 3, 4, 2), (2, 16, 2, 12, 67), (2, 64, 1, 64, 16), (2, 64, 4, 16, 17), (2, 4, 2, 16, 64),
    (3, 4, 3, 4, 65), (3, 12, 2, 12, 1), (3, 16, 2, 16, 2), (3, 64, 2, 16, 3), (3, 16, 1, 64, 64),
    (31, 4, 1, 4, 2), (31, 12, 2, 16, 3), (31, 16, 4, 16, 1), (31, 64, 3, 4, 5),
    (32, 4, 2, 12, 3), (32, 16, 2, 16, 67), (32, 12, 1, 64, 2), (32, 64, 1, 4, 1),
    (33, 4, 4, 16, 2), (33, 16, 3, 4, 5), (33, 12, 2, 12, 1), (33, 64, 2, 16, 17),
    (64, 4, 1, 4, 3), (64, 16, 2, 16, 2), (64, 12, 3, 4, 1), (64, 64, 4, 16, 2), (64, 64, 1, 64, 1), (26, 16, 2, 16, 67),
]
FIELD_LAYOUTS = ["adjacent", "permuted", "interleaved"]
# one batch just past what the bounded grid holds at once, in the forward (one sample per workgroup) and in the backward (one slice per
# workgroup), at the smallest shape
WRAP = dict(F=2, din=4, heads=1, hd=4, B=MAX_BLOCKS * 64 + 3, fields="interleaved", pad=1, res=True, scaled=False)


def cases():
    """One dict per case: every shape once with the field layout, the padding of the out / g_out / g_x strides, Wres present or not and the
    scale (1 or hd ** -0.5) cycling at co-prime periods."""
    return [dict(F=F, din=din, heads=H, hd=hd, B=B, fields=FIELD_LAYOUTS[n % 3], pad=(0, 4, 3, 8)[n % 4], res=n % 5 != 3, scaled=n % 2 == 1)
            for n, (F, din, H, hd, B) in enumerate(SHAPES)]


def case_id(c):
    return (f"F{c['F']}-din{c['din']}-{c['heads']}x{c['hd']}-B{c['B']}-{c['fields']}-pad{c['pad']}-{'res' if c['res'] else 'nores'}"
            f"-{'scaled' if c['scaled'] else 'unscaled'}")


def case_scale(c):
    return float(np.float32(c["hd"] ** -0.5)) if c["scaled"] else 1.0


def case_data(c, seed=0):
    """dict of a case's fp32 data from its own seed: offs, width, x [B, F, din] standard normal, Wq, Wk, Wv, Wres (or None) normal / sqrt(din),
    g [B, F * C] standard normal, scale."""
    F, din, H, hd, B = c["F"], c["din"], c["heads"], c["hd"], c["B"]
    C = H * hd
    rng = np.random.default_rng(seed + 7 * F + 131 * din + 1009 * B + 17 * C + H)
    offs, width = layout(F, din, c["fields"], seed)
    x = rng.standard_normal((B, F, din)).astype(np.float32)
    Ws = [(rng.standard_normal((C, din)) / np.sqrt(din)).astype(np.float32) for _ in range(4)]
    g = rng.standard_normal((B, F * C)).astype(np.float32)
    return dict(offs=offs, width=width, x=x, Wq=Ws[0], Wk=Ws[1], Wv=Ws[2], Wres=Ws[3] if c["res"] else None, g=g, scale=case_scale(c))
