"""float64 restatement of one Compressed Interaction Network layer (include/nrx_embed.h, nrx_cin_layer_fwd / _bwd), its derived error
bounds, an exact emulation of the header's fp32 chains, and the launch-shape cases the CPU and GPU tests share.  numpy only; held to torch
float64 einsum and autograd by tests/test_cin_ref.py.

Notation: X0 [B, m, D], Xp [B, Hp, D] (layer 1: Xp = X0), W [H, Hp, m], u = 2^-24, gamma(n) = n u / (1 - n u).

Bounds.  Every per-sample result is ONE fp32 fma chain from 0 over n terms (n = the term count rounded up to even: the matrix instruction takes
k in pairs and an odd count appends 0 * 0).  A term is fl(a * b) * w: its first factor carries one rounding (two when a = G = fl(g_p + g_xk) is
itself a rounded sum), and the chain adds at most n roundings, each relative to a partial sum that the sum of the terms' magnitudes bounds.  To
first order the chain stays within (n + r) u sum|terms| of the exact sum, r the roundings inside a term; gamma(n + r) = (n + r) u / (1 - (n + r) u)
makes the bound rigorous (Higham, Accuracy and Stability, lemma 3.1).  2^-126 per term covers a product that leaves the normal range.
  xk      : n = Hp m, r = 2 (the product's rounding and one spare: the issue's K + 2)      |err| <= gamma(n + 2) sum_k |Xp X0 W| + 2^-126 n
  p       : the D values each carry e_d = the bound above, the ascending sum adds D - 1 roundings:
                                                                                           |err| <= sum_d e_d + gamma(D) sum_d (|xk_d| + e_d)
  A, C    : n = H Hp (A, into g_x0) or H m (C, into g_xprev), r = 3 (G's rounding too)      |err| <= gamma(n + 3) sum |G X W| + 2^-126 n
  g_x0    : accumulate: s1 = fl(up + A), one more rounding: e1 = e_A + u (|up + A| + e_A); layer 1 adds C onto it: e = e1 + e_C + u (|s1 + C| + e1 + e_C)
  g_W     : slice s is one chain over its n_s = (samples in it) D terms G * fl(Xp X0), r = 3:  e_s = gamma(n_s + 3) sum_{slice} |G Xp X0| + 2^-126 n_s;
            the S partials are added in order, S - 1 roundings:                             |err| <= sum_s e_s + gamma(S) sum_s (|part_s| + e_s)"""
from fractions import Fraction

import numpy as np

from tests.dot_interact_ref import _round_f32, fmaf, layout, place  # noqa: F401  (the exact fp32 fma and the field layouts are shared)

U = 2.0 ** -24
TINY = 2.0 ** -126


def gamma(n):
    return n * U / (1.0 - n * U)


def even(n):
    return n + (n & 1)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _outer(Xa, Xb):
    """[B, a, D], [B, b, D] -> [B, a * b, D]: Z[b, i * nb + j, d] = Xa[b, i, d] Xb[b, j, d]."""
    B, na, D = Xa.shape
    return (Xa[:, :, None, :] * Xb[:, None, :, :]).reshape(B, na * Xb.shape[1], D)


def layer_fwd(X0, Xp, W):
    """((xk [B, H, D], p [B, H]) float64, (their bounds))."""
    X0, Xp, W = _f64(X0), _f64(Xp), _f64(W)
    H, Hp, m = W.shape
    Z = _outer(Xp, X0)
    W2 = W.reshape(H, Hp * m)
    xk = np.matmul(W2, Z)
    mag = np.matmul(np.abs(W2), np.abs(Z))
    n = even(Hp * m)
    e = gamma(n + 2) * mag + TINY * n
    D = X0.shape[2]
    p = xk.sum(-1)
    ep = e.sum(-1) + gamma(D) * (np.abs(xk) + e).sum(-1)
    return (xk, p), (e, ep)


def layer_G(g_p, g_xk, D):
    g_p = _f64(g_p)
    G = np.repeat(g_p[:, :, None], D, axis=2)
    return G if g_xk is None else G + _f64(g_xk)


def layer_bwd(X0, Xp, W, g_p, g_xk=None, up=None, layer1=False):
    """One layer's data gradients: (g_xprev [B, Hp, D] or None at layer 1, g_x0 [B, m, D]) float64 and their bounds.  `up` [B, m, D]: what g_x0
    holds when accumulate_x0 is set (None: stored).  layer1: Xp is X0 and the g_xprev term is added onto g_x0."""
    X0, Xp, W = _f64(X0), _f64(Xp), _f64(W)
    H, Hp, m = W.shape
    D = X0.shape[2]
    G = layer_G(g_p, g_xk, D)
    A = np.einsum("bhd,hij,bid->bjd", G, W, Xp, optimize=True)
    mA = np.einsum("bhd,hij,bid->bjd", np.abs(G), np.abs(W), np.abs(Xp), optimize=True)
    C = np.einsum("bhd,hij,bjd->bid", G, W, X0, optimize=True)
    mC = np.einsum("bhd,hij,bjd->bid", np.abs(G), np.abs(W), np.abs(X0), optimize=True)
    nA, nC = even(H * Hp), even(H * m)
    eA = gamma(nA + 3) * mA + TINY * nA
    eC = gamma(nC + 3) * mC + TINY * nC
    g0, e0 = A, eA
    if up is not None:
        g0 = _f64(up) + A
        e0 = eA + U * (np.abs(g0) + eA)
    if layer1:
        g1 = g0 + C
        return (None, g1), (None, e0 + eC + U * (np.abs(g1) + e0 + eC))
    return (C, g0), (eC, e0)


def layer_gw(X0, Xp, g_p, g_xk, slice_samples):
    """(g_W [H, Hp, m] float64, its bound) with the partials over slices of `slice_samples` samples."""
    X0, Xp = _f64(X0), _f64(Xp)
    B, m, D = X0.shape
    Hp = Xp.shape[1]
    G = layer_G(g_p, g_xk, D)
    H = G.shape[1]
    total, esum, psum = np.zeros((H, Hp * m)), np.zeros((H, Hp * m)), np.zeros((H, Hp * m))
    S = 0
    for b0 in range(0, B, slice_samples):
        sl = slice(b0, min(b0 + slice_samples, B))
        Z = _outer(Xp[sl], X0[sl])
        part = np.tensordot(G[sl], Z, axes=([0, 2], [0, 2]))
        mag = np.tensordot(np.abs(G[sl]), np.abs(Z), axes=([0, 2], [0, 2]))
        n = (sl.stop - sl.start) * D
        e = gamma(n + 3) * mag + TINY * n
        total += part
        esum += e
        psum += np.abs(part) + e
        S += 1
    return total.reshape(H, Hp, m), (esum + gamma(S) * psum).reshape(H, Hp, m)


# ---------------------------------------------------------------------------------------------------------- the header's fp32 chains, bit for bit
def _pair_chain(P, Q, Wn):
    """out[b, n, d] = chain from 0 over k = u V + v ascending of fmaf(fl(P[b, u, d] Q[b, v, d]), Wn[n, u, v], acc); an odd U V appends fmaf(0, 0, acc)."""
    P, Q, Wn = np.asarray(P, np.float32), np.asarray(Q, np.float32), np.asarray(Wn, np.float32)
    B, Un, D = P.shape
    V, N = Q.shape[1], Wn.shape[0]
    out = np.zeros((B, N, D), np.float32)
    for b in range(B):
        for d in range(D):
            prods = [np.float32(P[b, u, d]) * np.float32(Q[b, v, d]) for u in range(Un) for v in range(V)]       # (numpy fp32 multiply: rounded once)
            for n in range(N):
                w = Wn[n].reshape(-1)
                acc = 0.0
                for k, t in enumerate(prods):
                    acc = fmaf(t, w[k], acc)
                if len(prods) & 1:
                    acc = fmaf(0.0, 0.0, acc)
                out[b, n, d] = acc
    return out


def _add32(a, b):
    return _round_f32(Fraction(float(a)) + Fraction(float(b)))


def chain_G(g_p, g_xk, D):
    g_p = np.asarray(g_p, np.float32)
    G = np.repeat(g_p[:, :, None], D, axis=2)
    return G if g_xk is None else (G + np.asarray(g_xk, np.float32)).astype(np.float32)


def fwd_chain(X0, Xp, W):
    """(xk [B, H, D], p [B, H]) fp32 by the header's chains."""
    xk = _pair_chain(Xp, X0, W)
    B, H, D = xk.shape
    p = np.zeros((B, H), np.float32)
    for b in range(B):
        for h in range(H):
            s = 0.0
            for d in range(D):
                s = _add32(s, xk[b, h, d])
            p[b, h] = s
    return xk, p


def bwd_chain(X0, Xp, W, g_p, g_xk=None, up=None, layer1=False):
    """(g_xprev or None, g_x0) fp32 by the header's chains."""
    W = np.asarray(W, np.float32)
    D = np.asarray(X0).shape[2]
    G = chain_G(g_p, g_xk, D)
    A = _pair_chain(G, Xp, W.transpose(2, 0, 1))           # Wn[j; h, i] = W[h, i, j]
    C = _pair_chain(G, X0, W.transpose(1, 0, 2))           # Wn[i; h, j] = W[h, i, j]
    g0 = A
    if up is not None:
        g0 = np.vectorize(_add32, otypes=[np.float32])(np.asarray(up, np.float32), A)
    if layer1:
        return None, np.vectorize(_add32, otypes=[np.float32])(g0, C)
    return C, g0


def gw_chain(X0, Xp, g_p, g_xk, slice_samples):
    """g_W [H, Hp, m] fp32: per slice one chain over (b, d) ascending of fmaf(G, fl(Xp X0), acc); the partials added in slice order."""
    X0, Xp = np.asarray(X0, np.float32), np.asarray(Xp, np.float32)
    B, m, D = X0.shape
    Hp = Xp.shape[1]
    G = chain_G(g_p, g_xk, D)
    H = G.shape[1]
    out = np.zeros((H, Hp, m), np.float32)
    for h in range(H):
        for i in range(Hp):
            for j in range(m):
                tot = None
                for b0 in range(0, B, slice_samples):
                    acc = 0.0
                    for b in range(b0, min(b0 + slice_samples, B)):
                        for d in range(D):
                            acc = fmaf(G[b, h, d], np.float32(Xp[b, i, d]) * np.float32(X0[b, j, d]), acc)
                    tot = acc if tot is None else _add32(tot, acc)
                out[h, i, j] = tot
    return out


# ---------------------------------------------------------------------------------------------------------- the launch-shape cases
# (m, Hp, H, D, B); Hp None = layer 1 (xprev == NULL, Hp = m).  A covering selection: D over {4, 12, 16, 20, 32, 36, 64} (divides the 32-row
# tile, does not, equals it, spans two tiles), m over {2, 3, 26, 33, 64}, Hp over {1, 5, 32, 33, 64} and layer 1, H over {1, 31, 32, 33, 64} (one
# column tile, its edge, two), odd K = Hp m (3, 9, 15, 99, 1089), B over {1, 2, 3, 5, 67}; (64, 64, 64, 64) is the one that splits K into LDS slabs.
SHAPES = [
    (2, None, 1, 4, 1), (3, None, 31, 12, 2), (26, None, 32, 16, 3), (33, None, 33, 20, 5), (64, None, 64, 32, 2),
    (3, 1, 1, 36, 67), (2, 5, 33, 64, 3), (26, 32, 32, 16, 5), (33, 33, 31, 4, 67), (64, 64, 64, 64, 5),
    (3, 5, 1, 12, 1), (2, 64, 31, 20, 2), (64, 1, 64, 16, 3), (26, 5, 32, 32, 1), (3, 33, 33, 36, 2), (33, 32, 1, 64, 1),
]
FIELD_LAYOUTS = ["adjacent", "permuted", "interleaved"]
# the bounded grid of the pair kernel: 256 * 4 workgroups of 8 waves at a tiny shape, one sample per wave tile at D = 32: this batch wraps it
WRAP = dict(m=2, Hp=None, H=1, D=32, B=256 * 4 * 8 + 3, fields="interleaved", xk_null=False, gxk_null=False, acc=True, p_off=1)


def cases():
    """One dict per case: every shape once with the layout and the options cycling at co-prime periods, then every layout x option at one small
    shape, at layer 1 and above it."""
    out = []
    for n, (m, Hp, H, D, B) in enumerate(SHAPES):
        out.append(dict(m=m, Hp=Hp, H=H, D=D, B=B, fields=FIELD_LAYOUTS[n % 3], xk_null=n % 4 == 1, gxk_null=n % 5 == 2, acc=n % 2 == 1, p_off=(0, 3, 1)[n % 3]))
    for fl in FIELD_LAYOUTS:
        for n in range(8):
            out.append(dict(m=3, Hp=None if (n + len(fl)) % 2 else 5, H=5, D=8, B=3, fields=fl, xk_null=bool(n & 1), gxk_null=bool(n & 2), acc=bool(n & 4),
                            p_off=2 * (n & 1)))
    return out


def case_id(c):
    return (f"m{c['m']}-Hp{c['Hp'] or 'L1'}-H{c['H']}-D{c['D']}-B{c['B']}-{c['fields']}" + ("-noxk" if c["xk_null"] else "") + ("-nogxk" if c["gxk_null"] else "")
            + ("-acc" if c["acc"] else "") + f"-p{c['p_off']}")


def case_data(c, seed=0, scale=1.0, ints=False):
    """dict of a case's fp32 data from its own seed: offs, width, X0 [B, m, D], Xp (None at layer 1), W, g_p, g_xk (None if gxk_null), up (None
    unless acc).  ints: small integers in -3..3 (every sum exact in fp32)."""
    m, Hp, H, D, B = c["m"], c["Hp"], c["H"], c["D"], c["B"]
    rng = np.random.default_rng(seed + 7 * m + 131 * D + 1009 * B + 17 * H + 3 * (Hp or 0))
    offs, width = layout(m, D, c["fields"], seed)

    def draw(*shape):
        if ints:
            return rng.integers(-3, 4, shape).astype(np.float32)
        return (rng.standard_normal(shape) * scale).astype(np.float32)
    X0 = draw(B, m, D)
    Xp = None if Hp is None else draw(B, Hp, D)
    W = draw(H, Hp or m, m) if ints else (rng.standard_normal((H, Hp or m, m))).astype(np.float32)
    g_p = draw(B, H)
    g_xk = None if c["gxk_null"] else draw(B, H, D)
    up = draw(B, m, D) if c["acc"] else None
    return dict(offs=offs, width=width, X0=X0, Xp=Xp, W=W, g_p=g_p, g_xk=g_xk, up=up)
