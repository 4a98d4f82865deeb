"""float64 restatement of the attentional pooling of pair interactions (include/nrx_embed.h, nrx_afm_fwd / _bwd) with hand-written
gradients, its derived error bounds, an exact emulation of the header's score chains, and the launch-shape cases the CPU and GPU tests share.
numpy only; held to torch float64 autograd of ops.afm_pool_math by tests/test_afm_ref.py.

Notation: e [B, F, D], pairs p = (i, j), j < i, in tril order, h_p = e_i * e_j, W1 [A, D], b1 [A], w2 [A]; u = 2^-24, gamma(n) = n u / (1 - n u)
(Higham, Accuracy and Stability, lemma 3.1: a chain of n roundings stays within gamma(n) of the sum of its terms' magnitudes).  Every bound
below is a running error analysis: the error of each intermediate is carried, as an array, into the next.

Forward.
  h       : one rounding, folded into the chains that consume it (their "+ 1").
  z_t     : chain from b1 over D fmas                                 ez = gamma(D + 1) (|b1| + sum_d |W1 h|)
  a       : relu is 1-Lipschitz; two half chains of at most A real terms (a term of a padded row is fma(0, 0, s) = s, exact) and one add
                                                                      ea = sum_t |w2| ez + gamma(A + 1) sum_t |w2| (relu z + ez)
  E_p     : softmax is shift invariant, so the computed maximum is a shift, not an error.  The argument fl(a - m) carries ea and one rounding
            u |a - m|; expf of the device library is within 1 ulp, a relative 2^-23 = EXP_REL (its documented bound; the fast exp2 form the
            kernel does NOT use would add the rounding of a * log2(e), relative to |a|):
                                                                      eps_p = expm1(ea + u |a_p - m|) (1 + EXP_REL) + EXP_REL
  l       : positive terms: a lane's ascending partial sum and the 6-step butterfly, nl = ceil(P / 64) + 6 roundings
                                                                      eps_l = sum_p alpha_p eps_p + gamma(nl) (1 + sum_p alpha_p eps_p)
  alpha   : fl(E_p / l)                                               e_alpha = alpha ((1 + eps_p) (1 + u) / (1 - eps_l) - 1)
  out     : G = 64 // D chains of at most ceil(P / G) fmas and G - 1 adds, h's rounding: n_o = ceil(P / G) + G
                                                                      e_out = sum_p e_alpha |h| + gamma(n_o) sum_p (alpha + e_alpha) |h| + 2^-126 P
  lse     : fl(m + logf(l)), logf within 1 ulp                        e_lse = -log1p(-eps_l) + EXP_REL |log l| + u (|lse| + |m| + |log l|)
  `exp_rel=0` gives the exp-free part (uniform weights: every argument is 0 and expf(0) = 1 exactly).
Backward (the activation pattern [z > 0] is taken as the float64 one: the tests assert that it is, or keep |z| far above ez).
  alpha   : expf(fl(a - lse)), lse the saved fp32 value                eps_b = expm1(ea + e_lse + u |a - lse|) (1 + EXP_REL) + EXP_REL
  dalpha  : two half chains of D / 2 fmas, one add, h's rounding       e_dal = gamma(D / 2 + 2) sum_d |g h|
  delta   : chain of D fmas over the saved fp32 out                    e_del = sum_d |g| e_out + gamma(D) sum_d |g| (|out| + e_out)
  da      : fl(alpha fl(dalpha - delta)): product rule with one rounding each
  u_t     : fl(da w2_t) where z_t > 0                                  e_u = |w2| e_da + u |w2| (|da| + e_da)
  g_h     : chain from fl(alpha g) over at most A real fmas            e_gh = e_al |g| + sum_t |W1| e_u + gamma(A + 1) ((alpha + e_al) |g| + sum_t |W1| (|u| + e_u))
  g_e_i   : fl(g_h e_j) added over at most F - 1 non-zero terms        e_ge = sum_j e_gh |e_j| + gamma(F) sum_j (|g_h| + e_gh) |e_j|
  g_W1    : slice s is one chain over its n_s = (samples in it) P fmas of u h (h's rounding: + 1); the S partials are added in order:
            e_s = sum e_u |h| + gamma(n_s + 1) sum (|u| + e_u) |h|;    |err| <= sum_s e_s + gamma(S) sum_s (|part_s| + e_s)
  g_b1    : the same with h = 1;  g_w2: the terms are da relu(z): e = e_da (relu z + ez) + |da| ez, magnitude (|da| + e_da) (relu z + ez)."""
from fractions import Fraction

import numpy as np

from tests.dot_interact_ref import _round_f32, fmaf, layout, pair_index, place  # noqa: F401  (the exact fp32 fma and the field layouts are shared)

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_REL = 2.0 ** -23
SLICE = 16          # nrx_afm_wgrad_slice: asserted by the GPU test
GRID_WAVES = 1024 * 4   # the bounded grid: workgroups x waves


def gamma(n):
    return n * U / (1.0 - n * U)


def _f64(a):
    return np.asarray(a, np.float64)


def forward(e, W1, b1, w2, exp_rel=EXP_REL):
    """dict of the float64 forward and its bounds: h [B, P, D], z [B, P, A], a, alpha [B, P], out [B, D], lse [B]; ez, ea, e_out, e_lse, ..."""
    e, W1, b1, w2 = _f64(e), _f64(W1), _f64(b1), _f64(w2)
    B, F, D = e.shape
    A = W1.shape[0]
    ii, jj = pair_index(F)
    P = len(ii)
    h = e[:, ii] * e[:, jj]
    z = h @ W1.T + b1
    ez = gamma(D + 1) * (np.abs(h) @ np.abs(W1).T + np.abs(b1))
    rz = np.maximum(z, 0.0)
    a = rz @ w2
    ea = ez @ np.abs(w2) + gamma(A + 1) * ((rz + ez) @ np.abs(w2))
    m = a.max(1, keepdims=True)
    E = np.exp(a - m)
    l = E.sum(1, keepdims=True)
    alpha = E / l
    eps_p = np.expm1(ea + U * np.abs(a - m)) * (1 + exp_rel) + exp_rel
    mean_eps = (alpha * eps_p).sum(1, keepdims=True)
    nl = -(-P // 64) + 6
    eps_l = mean_eps + gamma(nl) * (1 + mean_eps)
    e_alpha = alpha * ((1 + eps_p) * (1 + U) / (1 - eps_l) - 1)
    out = np.einsum("bp,bpd->bd", alpha, h)
    G = 64 // D
    n_o = -(-P // G) + G
    e_out = np.einsum("bp,bpd->bd", e_alpha, np.abs(h)) + gamma(n_o) * np.einsum("bp,bpd->bd", alpha + e_alpha, np.abs(h)) + TINY * P
    logl = np.log(l[:, 0])
    lse = m[:, 0] + logl
    e_lse = -np.log1p(-eps_l[:, 0]) + exp_rel * np.abs(logl) + U * (np.abs(lse) + np.abs(m[:, 0]) + np.abs(logl))
    return dict(ii=ii, jj=jj, h=h, z=z, ez=ez, rz=rz, a=a, ea=ea, alpha=alpha, e_alpha=e_alpha, out=out, e_out=e_out, lse=lse, e_lse=e_lse)


def backward(e, W1, b1, w2, g_out, slice_samples=SLICE, exp_rel=EXP_REL):
    """((g_e [B, F, D], g_W1, g_b1, g_w2) float64 by hand-written gradients, (their bounds))."""
    e, W1, b1, w2, g = _f64(e), _f64(W1), _f64(b1), _f64(w2), _f64(g_out)
    B, F, D = e.shape
    A = W1.shape[0]
    f = forward(e, W1, b1, w2, exp_rel)
    ii, jj, h, z, ez, rz, a, ea, alpha = f["ii"], f["jj"], f["h"], f["z"], f["ez"], f["rz"], f["a"], f["ea"], f["alpha"]
    P = len(ii)
    lse, e_lse, out, e_out = f["lse"][:, None], f["e_lse"][:, None], f["out"], f["e_out"]
    eps_b = np.expm1(ea + e_lse + U * np.abs(a - lse)) * (1 + exp_rel) + exp_rel
    e_al = alpha * eps_b
    ah = np.abs(h)
    dal = np.einsum("bd,bpd->bp", g, h)
    e_dal = gamma(D // 2 + 2) * np.einsum("bd,bpd->bp", np.abs(g), ah)
    delta = (g * out).sum(1, keepdims=True)
    e_del = (np.abs(g) * e_out).sum(1, keepdims=True) + gamma(D) * (np.abs(g) * (np.abs(out) + e_out)).sum(1, keepdims=True)
    diff = dal - delta
    e_diff = e_dal + e_del + U * (np.abs(diff) + e_dal + e_del)
    da = alpha * diff
    e_da = e_al * (np.abs(diff) + e_diff) + alpha * e_diff + U * (alpha + e_al) * (np.abs(diff) + e_diff)
    on = (z > 0).astype(np.float64)
    u = on * da[:, :, None] * w2
    e_u = on * (np.abs(w2) * e_da[:, :, None] + U * np.abs(w2) * (np.abs(da) + e_da)[:, :, None])
    gh = alpha[:, :, None] * g[:, None, :] + u @ W1
    e_gh = (e_al[:, :, None] * np.abs(g)[:, None, :] + e_u @ np.abs(W1)
            + gamma(A + 1) * ((alpha + e_al)[:, :, None] * np.abs(g)[:, None, :] + (np.abs(u) + e_u) @ np.abs(W1)))
    ge, e_ge, m_ge = np.zeros_like(e), np.zeros_like(e), np.zeros_like(e)
    bi = np.arange(B)[:, None]
    for dst, src in ((ii, jj), (jj, ii)):
        np.add.at(ge, (bi, dst[None, :]), gh * e[:, src])
        np.add.at(e_ge, (bi, dst[None, :]), e_gh * np.abs(e[:, src]))
        np.add.at(m_ge, (bi, dst[None, :]), (np.abs(gh) + e_gh) * np.abs(e[:, src]))
    e_ge = e_ge + gamma(F) * m_ge
    # the parameter gradients, slice by slice
    terms_w2, err_w2, mag_w2 = da[:, :, None] * rz, e_da[:, :, None] * (rz + ez) + np.abs(da)[:, :, None] * ez, (np.abs(da) + e_da)[:, :, None] * (rz + ez)
    tot = [np.zeros((A, D)), np.zeros(A), np.zeros(A)]
    esum = [np.zeros((A, D)), np.zeros(A), np.zeros(A)]
    psum = [np.zeros((A, D)), np.zeros(A), np.zeros(A)]
    S = 0
    for b0 in range(0, B, slice_samples):
        sl = slice(b0, min(b0 + slice_samples, B))
        n = (sl.stop - sl.start) * P
        parts = [np.einsum("bpt,bpd->td", u[sl], h[sl]), u[sl].sum((0, 1)), terms_w2[sl].sum((0, 1))]
        errs = [np.einsum("bpt,bpd->td", e_u[sl], ah[sl]) + gamma(n + 1) * np.einsum("bpt,bpd->td", np.abs(u[sl]) + e_u[sl], ah[sl]),
                e_u[sl].sum((0, 1)) + gamma(n + 1) * (np.abs(u[sl]) + e_u[sl]).sum((0, 1)),
                err_w2[sl].sum((0, 1)) + gamma(n + 1) * mag_w2[sl].sum((0, 1))]
        for k in range(3):
            tot[k] += parts[k]
            esum[k] += errs[k] + TINY * n
            psum[k] += np.abs(parts[k]) + errs[k]
        S += 1
    bounds = [esum[k] + gamma(S) * psum[k] for k in range(3)]
    return (ge, tot[0], tot[1], tot[2]), (e_ge, bounds[0], bounds[1], bounds[2]), f


def min_margin(f):
    """min over every (b, p, t) of |z| / ez of a forward() dict: how many of its own fp32 bounds the nearest pre-activation is from the kink."""
    return float((np.abs(f["z"]) / f["ez"]).min())


def effective_pairs(f):
    """exp(entropy) of each sample's attention weights."""
    al = f["alpha"]
    return np.exp(-(al * np.log(np.maximum(al, 1e-300))).sum(1))


def keeps_pairs(f, P):
    """Every sample keeps exp(entropy) >= min(P, 8) pairs.  Up to 8 pairs that asks for uniform weights, which this float64 evaluation of the
    entropy reproduces only to its own rounding (2.9999999999999996 for three equal weights): a relative 1e-9 is allowed for it."""
    return bool(effective_pairs(f).min() >= min(P, 8) * (1 - 1e-9))


# ---------------------------------------------------------------------------------------------------------- the header's score chains, bit for bit
def score_chain(ei, ej, W1, b1, w2):
    """(z [A], a) fp32 of one pair by the header's chains: z_t from b1[t] over d ascending of fmaf(W1[t, d], fl(e_i[d] e_j[d]), .); a = fl(s_0 +
    s_1), s_k the chain from 0 over the t with ((t >> 2) & 1) == k ascending of fmaf(w2[t], max(z_t, 0), .)."""
    ei, ej, W1, b1, w2 = (np.asarray(v, np.float32) for v in (ei, ej, W1, b1, w2))
    A, D = W1.shape
    h = [np.float32(ei[d]) * np.float32(ej[d]) for d in range(D)]          # (numpy fp32 multiply: rounded once)
    z = np.zeros(A, np.float32)
    for t in range(A):
        acc = float(b1[t])
        for d in range(D):
            acc = fmaf(W1[t, d], h[d], acc)
        z[t] = acc
    s = [0.0, 0.0]
    for t in range(A):
        k = (t >> 2) & 1
        s[k] = fmaf(w2[t], max(float(z[t]), 0.0), s[k])
    return z, np.float32(_round_f32(Fraction(s[0]) + Fraction(s[1])))


# ---------------------------------------------------------------------------------------------------------- the launch-shape cases
# (F, D, A, B).  F over {2, 3, 8, 9, 26, 32, 33, 64}: P = 1, 3, 28, 36 (the first crossing of a 32-pair tile), 325, 496, 528 (half a tile over), 2016
# (whole tiles); D over {4, 12, 16, 20, 32, 36, 64} (divides 64, does not, one column tile, two); A over {1, 5, 16, 31, 32, 33, 64} (one row tile,
# its edge, two); B over {1, 2, 3, 5, 67} and the weight-gradient slices: 16 = exactly one, 17 = one + 1 sample, 67 = several.
SHAPES = [
    (2, 4, 1, 1), (2, 12, 5, 2), (2, 16, 16, 3), (2, 20, 31, 5), (2, 32, 32, 67), (2, 36, 33, 16), (2, 64, 64, 17),
    (3, 4, 5, 67), (3, 12, 16, 1), (3, 16, 31, 2), (3, 64, 1, 3), (3, 36, 64, 5),
    (8, 4, 16, 2), (8, 12, 31, 3), (8, 16, 32, 5), (8, 32, 64, 1), (8, 20, 1, 17),
    (9, 4, 31, 3), (9, 12, 32, 5), (9, 16, 33, 67), (9, 36, 5, 1), (9, 64, 16, 2),
    (26, 4, 32, 5), (26, 12, 33, 1), (26, 16, 16, 67), (26, 20, 5, 2), (26, 64, 31, 3), (26, 32, 1, 16),
    (32, 4, 33, 1), (32, 16, 64, 2), (32, 20, 16, 3), (32, 36, 31, 5), (32, 12, 1, 17),
    (33, 4, 64, 2), (33, 16, 1, 3), (33, 20, 33, 5), (33, 32, 5, 1), (33, 64, 32, 2),
    (64, 12, 64, 1), (64, 16, 5, 2), (64, 32, 16, 3), (64, 4, 1, 5), (64, 64, 64, 3),
]
FIELD_LAYOUTS = ["adjacent", "permuted", "interleaved"]
# one batch just past what the bounded grid holds at once -- in the forward (one sample per wave) and in the backward (one slice per wave) --, at
# the smallest shape
WRAP = dict(F=2, D=4, A=1, B=GRID_WAVES * SLICE + 3, fields="interleaved", pad=1)
# general-valued forward + backward: shapes small enough that the float64 min |z| stays 100 bounds clear of the kink (asserted)
GAUSS_BWD = [(2, 4, 1, 3), (3, 4, 5, 5), (3, 12, 5, 17), (8, 4, 1, 2), (2, 16, 16, 67)]
# z and a bit for bit (F = 2: P = 1, alpha = 1 and lse = fl(a + logf(1)) = a)
EXACT = [(4, 1), (12, 5), (16, 16), (20, 33), (64, 64)]


def cases():
    """One dict per case: every shape once with the field layout and the padding of the out / g_out / g_x strides cycling at co-prime periods."""
    return [dict(F=F, D=D, A=A, B=B, fields=FIELD_LAYOUTS[n % 3], pad=(0, 4, 3, 8)[n % 4]) for n, (F, D, A, B) in enumerate(SHAPES)]


def case_id(c):
    return f"F{c['F']}-D{c['D']}-A{c['A']}-B{c['B']}-{c['fields']}-pad{c['pad']}"


def case_data(c, seed=0, kind="dyadic"):
    """dict of a case's fp32 data from its own seed: offs, width, e [B, F, D], W1, b1, w2, g.
    dyadic: field values multiples of 2^-2 in [-2, 2], W1 multiples of 2^-3 in [-1, 1], b1 odd multiples of 2^-8 in (-1/8, 1/8): every z is a
    multiple of 2^-8 below 2^9 in magnitude -- exact in fp32 in any order -- and odd, so |z| >= 2^-8.  w2 is real-valued, scaled (by halving)
    until the float64 softmax of every sample keeps exp(entropy) >= min(P, 8) pairs.
    gauss: standard normal fields, W1 / sqrt(D), b1 / 10, w2 / sqrt(A)."""
    F, D, A, B = c["F"], c["D"], c["A"], c["B"]
    rng = np.random.default_rng(seed + 7 * F + 131 * D + 1009 * B + 17 * A)
    offs, width = layout(F, D, c["fields"], seed)
    g = rng.standard_normal((B, D)).astype(np.float32)
    if kind == "gauss":
        e = rng.standard_normal((B, F, D)).astype(np.float32)
        W1 = (rng.standard_normal((A, D)) / np.sqrt(D)).astype(np.float32)
        b1 = (rng.standard_normal(A) / 10).astype(np.float32)
        w2 = (rng.standard_normal(A) / np.sqrt(A)).astype(np.float32)
        return dict(offs=offs, width=width, e=e, W1=W1, b1=b1, w2=w2, g=g)
    e = (rng.integers(-8, 9, (B, F, D)) / 4.0).astype(np.float32)
    W1 = (rng.integers(-8, 9, (A, D)) / 8.0).astype(np.float32)
    b1 = ((2 * rng.integers(-16, 16, A) + 1) / 256.0).astype(np.float32)
    w2 = rng.standard_normal(A).astype(np.float32)
    P = F * (F - 1) // 2
    for _ in range(40):
        if keeps_pairs(forward(e, W1, b1, w2), P):
            break
        w2 = (w2 * np.float32(0.5)).astype(np.float32)
    return dict(offs=offs, width=width, e=e, W1=W1, b1=b1, w2=w2, g=g)
