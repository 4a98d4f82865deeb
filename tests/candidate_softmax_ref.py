"""float64 restatement of the candidate softmax loss (include/nrx_embed.h, nrx_cand_softmax_fwd / _bwd, ops.candidate_softmax): the in-batch
softmax of tests/inbatch_softmax_ref.py over a rectangular candidate set with a per-column additive term, and the error bounds its fp32
matrix-core implementation is held to.  Not a test module: tests/test_candidate_softmax*.py import it.

    U [B, d], V [N, d] with N >= B: column i < B is row i's positive, columns B..N-1 are extra negatives; bias [N] or none (zeros)
    z_ij = dot(U_i, V_j) * inv_t + bias_j;  column j is excluded for row i when ids [N] are given, j != i and ids[j] == ids[i]
    lse_i = log sum_kept exp(z_ij);  l_i = lse_i - z_ii;  p_ij = exp(z_ij - lse_i) (0 when excluded)
    dU_i = g_i inv_t sum_{j<N} (p_ij - [i==j]) V_j        dV_j = inv_t sum_{i<B} g_i (p_ij - [i==j]) U_i   for every j < N
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests.inbatch_softmax_ref import EPS, FLT_MIN, score_error


def candidate_softmax_ref(U, V, inv_t, ids=None, bias=None, g=None):
    """All in float64 on the values handed in (fp32 inputs are widened exactly).  Returns a namespace: loss, lse, diag [B], zmax (the largest
    |z_ij|); with g also dU [B, d], dV [N, d] and abs_dU, abs_dV -- per output element the sum of |g_i| inv_t max(p_ij, |p_ij - [i==j]|) |x|
    over the terms that make it up."""
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    B, N = U.shape[0], V.shape[0]
    assert N >= B
    inv_t = float(inv_t)
    z = (U @ V.T) * inv_t
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)[None, :]
    eye = np.eye(B, N, dtype=bool)
    keep = np.ones((B, N), dtype=bool)
    if ids is not None:
        ids = np.asarray(ids).astype(np.int64)
        keep = (ids[:B, None] != ids[None, :]) | eye
    zm = np.where(keep, z, -np.inf)
    m = zm.max(axis=1) if B else np.zeros(0)
    e = np.where(keep, np.exp(zm - m[:, None]), 0.0)
    lse = m + np.log(e.sum(axis=1))
    diag = np.diagonal(z).copy()
    out = SimpleNamespace(loss=lse - diag, lse=lse, diag=diag, U=U, V=V, inv_t=inv_t, zmax=float(np.abs(z).max()) if z.size else 0.0)
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        p = np.where(keep, np.exp(zm - lse[:, None]), 0.0)
        c = g[:, None] * inv_t * (p - eye)
        # a row with p_ii within 1e-7 of 1 carries an absolute error of about E_z in p_ii - 1: the weight of a term is the larger of p and |p - [i==j]|
        w = np.abs(g)[:, None] * inv_t * np.maximum(p, np.abs(p - eye))
        out.dU = c @ V
        out.dV = c.T @ U
        out.abs_dU = w @ np.abs(V)
        out.abs_dV = w.T @ np.abs(U)
        # the same sums with every weight replaced by 1: what the terms weigh when p_ij itself is lost (below 2^-126)
        out.cap_dU = np.abs(g)[:, None] * inv_t * np.abs(V).sum(axis=0)[None, :] + np.zeros_like(out.dU)
        out.cap_dV = inv_t * (np.abs(g)[:, None] * np.abs(U)).sum(axis=0)[None, :] + np.zeros_like(out.dV)
    return out


def logit_error(ref, d):
    """E_z = E_s + 2^-24 max|z_ij|: the score's error (inbatch_softmax_ref.score_error) and one more rounded addition, of the bias."""
    return score_error(ref, d) + EPS * ref.zmax


def loss_tolerance(ref, d):
    """|err(l_i)| <= 4 E_z + 8 2^-24 max(1, |lse_i|, |z_ii|)."""
    return 4.0 * logit_error(ref, d) + 8.0 * EPS * np.maximum(1.0, np.maximum(np.abs(ref.lse), np.abs(ref.diag)))


def grad_tolerance(ref, d):
    """4 (2 E_z + 16 2^-24) (sum of an element's term weights) plus inbatch_softmax_ref.grad_tolerance's 2^-126 allowance for the p_ij that
    no fp32 evaluation can hold."""
    rho = 2.0 * logit_error(ref, d) + 16.0 * EPS
    return 4.0 * rho * ref.abs_dU + FLT_MIN * (ref.cap_dU + 1.0), 4.0 * rho * ref.abs_dV + FLT_MIN * (ref.cap_dV + 1.0)


def torch_candidate_rows(u, v, inv_t, ids=None, bias=None):
    """The materialised [B, N] form in torch, in the dtype of u: what the fused op avoids.  Differentiable; used as the fp32 stand-in that
    checks the bounds without the kernel, and as the restatement the module tests compare with."""
    import torch
    B, N = u.shape[0], v.shape[0]
    z = (u @ v.t()) * inv_t
    if bias is not None:
        z = z + bias.to(z.dtype)[None, :]
    if ids is not None:
        eye = torch.eye(B, N, dtype=torch.bool, device=u.device)
        z = z.masked_fill((ids[:B, None] == ids[None, :]) & ~eye, float("-inf"))
    return torch.logsumexp(z, dim=1) - z.diagonal()


SMALL_B = (1, 2, 31, 32, 33, 64, 65)
SMALL_E = (0, 1, 31, 32, 33, 95)
DIMS = (4, 8, 12, 16, 32, 64)
DIM_SHAPES = ((33, 33), (65, 31))
LARGE_SHAPES = ((257, 1000), (1000, 24), (40, 4101))
SPLITS = (1, 3, 0)
IDS_KINDS = (None, 32, 64)


@functools.lru_cache(maxsize=None)
def make_case(B, E, d, ids_kind=None, with_bias=False, scale=None, temperature=0.1, seed=0):
    """Inputs (CPU torch, fp32) and the float64 reference of one case, computed once and shared by the tests (read only).  Unit rows, or
    N(0, 1) * scale; ids from max(2, N / 4) values, so that extras collide with positives and with each other; a bias in +-30; g with
    zeros and negative entries."""
    import torch
    N = B + E
    gen = torch.Generator().manual_seed(100003 * B + 101 * E + 7 * d + seed)
    u = torch.randn(B, d, generator=gen)
    v = torch.randn(N, d, generator=gen)
    if scale is None:
        u, v = torch.nn.functional.normalize(u, p=2, dim=1), torch.nn.functional.normalize(v, p=2, dim=1)
    else:
        u, v = u * scale, v * scale
    ids = None
    if ids_kind is not None:
        ids = torch.randint(0, max(2, N // 4), (N,), generator=gen).to(torch.int32 if ids_kind == 32 else torch.int64)
        ids = ids + (0 if ids_kind == 32 else (1 << 33))          # int64 ids beyond 32 bits, equal in their low words only where truly equal
    bias = (torch.rand(N, generator=gen) * 60.0 - 30.0) if with_bias else None
    g = torch.randn(B, generator=gen)
    g[::3] = 0.0
    g[1::5] = -g[1::5].abs()
    ref = candidate_softmax_ref(u.numpy(), v.numpy(), np.float32(1.0 / temperature), ids=None if ids is None else ids.numpy(),
                                bias=None if bias is None else bias.numpy(), g=g.numpy())
    return u, v, ids, bias, g, ref


def small_cases(B):
    """Every E around the 32-row tiles at d = 16, with and without ids (int32, int64) and bias."""
    return [dict(B=B, E=E, d=16, ids_kind=k, with_bias=b) for E in SMALL_E for k in IDS_KINDS for b in (False, True)]


def dim_cases(d):
    return [dict(B=B, E=E, d=d, ids_kind=k, with_bias=b) for (B, E) in DIM_SHAPES for k in IDS_KINDS for b in (False, True)]


def large_cases(B, E):
    return [dict(B=B, E=E, d=16, ids_kind=k, with_bias=b) for k in IDS_KINDS for b in (False, True)]


def hot_cases():
    """Unnormalised rows scaled by 3 at temperature 0.01: |s| reaches 1e4, where exp() without the running maximum overflows."""
    return [dict(B=257, E=95, d=16, ids_kind=k, with_bias=b, scale=3.0, temperature=0.01) for (k, b) in ((64, True), (None, False), (32, True))]


def golden_inputs(B, d, with_ids):
    """The seeded inputs whose ops.inbatch_softmax bits tests/golden/inbatch_softmax_bits.json records (temperature 0.1, col_splits 0)."""
    rng = np.random.default_rng(7000 + 10 * B + d + (1 if with_ids else 0))
    u = rng.standard_normal((B, d)).astype(np.float32) * np.float32(0.25)
    v = rng.standard_normal((B, d)).astype(np.float32) * np.float32(0.25)
    g = rng.standard_normal(B).astype(np.float32)
    g[::3] = 0.0
    ids = rng.integers(0, max(2, B // 4), B).astype(np.int64) if with_ids else None
    return u, v, g, ids
