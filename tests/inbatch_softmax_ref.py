"""float64 restatement of the in-batch softmax loss (include/nrx_embed.h, nrx_inbatch_softmax_fwd / _bwd) and the error bounds
its fp32 matrix-core implementation is held to.  Not a test module: tests/test_inbatch_softmax*.py import it.

    s_ij = dot(U_i, V_j) * inv_t;  column j is excluded for row i when ids are given, j != i and ids[j] == ids[i]
    lse_i = log sum_kept exp(s_ij);  l_i = lse_i - s_ii;  p_ij = exp(s_ij - lse_i) (0 when excluded)
    dU_i = g_i inv_t sum_j (p_ij - [i==j]) V_j        dV_j = inv_t sum_i g_i (p_ij - [i==j]) U_i
"""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
FLT_MIN = 2.0 ** -126          # smallest normal fp32: exp() below it flushes to zero


def inbatch_softmax_ref(U, V, inv_t, ids=None, g=None):
    """All in float64 on the values handed in (fp32 inputs are widened exactly).  Returns a namespace: loss, lse, diag [B]; with g also
    dU, dV [B, d] and abs_dU, abs_dV -- per output element the sum of |g_i inv_t (p_ij - [i==j]) x| over the terms that make it up."""
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    B = U.shape[0]
    inv_t = float(inv_t)
    s = (U @ V.T) * inv_t
    eye = np.eye(B, dtype=bool)
    keep = np.ones((B, B), dtype=bool)
    if ids is not None:
        ids = np.asarray(ids).astype(np.int64)
        keep = (ids[:, None] != ids[None, :]) | eye
    sm = np.where(keep, s, -np.inf)
    m = sm.max(axis=1)
    e = np.where(keep, np.exp(sm - m[:, None]), 0.0)
    lse = m + np.log(e.sum(axis=1))
    diag = np.diagonal(s).copy()
    out = SimpleNamespace(loss=lse - diag, lse=lse, diag=diag, U=U, V=V, inv_t=inv_t)
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        p = np.where(keep, np.exp(sm - lse[:, None]), 0.0)
        c = g[:, None] * inv_t * (p - eye)
        out.dU = c @ V
        out.dV = c.T @ U
        out.abs_dU = np.abs(c) @ np.abs(V)
        out.abs_dV = np.abs(c).T @ np.abs(U)
        # the same sums with every |p_ij - [i==j]| replaced by 1: what the terms weigh when p_ij itself is lost (grad_tolerance)
        out.cap_dU = np.abs(g)[:, None] * inv_t * np.abs(V).sum(axis=0)[None, :] + np.zeros_like(out.dU)
        out.cap_dV = inv_t * (np.abs(g)[:, None] * np.abs(U)).sum(axis=0)[None, :] + np.zeros_like(out.dV)
    return out


def score_error(ref, d):
    """E_s: the fp32 chain of d products (and the scale by inv_t) perturbs a score by at most (d + 2) 2^-24 max|U_i| max|V_j| inv_t."""
    nu = np.sqrt((ref.U ** 2).sum(axis=1)).max() if ref.U.size else 0.0
    nv = np.sqrt((ref.V ** 2).sum(axis=1)).max() if ref.V.size else 0.0
    return (d + 2) * EPS * nu * nv * ref.inv_t


def loss_tolerance(ref, d):
    """|err(l_i)| <= 4 E_s + 8 2^-24 max(1, |lse_i|, |s_ii|)."""
    return 4.0 * score_error(ref, d) + 8.0 * EPS * np.maximum(1.0, np.maximum(np.abs(ref.lse), np.abs(ref.diag)))


def grad_tolerance(ref, d):
    """Every term carries a relative perturbation of at most rho = 2 E_s + 16 2^-24; an element's error is at most 4 rho (sum of |terms|).
    A relative bound holds only for what fp32 can hold: a p_ij below 2^-126 (s_ij - lse_i < -87, everywhere at |s| ~ 1e4) is 0 in ANY fp32
    evaluation while float64 keeps it, so each term may in addition be off by 2^-126 times its weight g_i inv_t |x| (and the sum by one more
    2^-126) -- some 1e-34 absolute at the shapes tested, far below every term fp32 resolves (at scale 3, temperature 0.01
    the float64 dV has elements of 1e-57)."""
    rho = 2.0 * score_error(ref, d) + 16.0 * EPS
    return 4.0 * rho * ref.abs_dU + FLT_MIN * (ref.cap_dU + 1.0), 4.0 * rho * ref.abs_dV + FLT_MIN * (ref.cap_dV + 1.0)
