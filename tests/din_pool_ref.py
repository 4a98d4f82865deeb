"""Float64 restatement of the target-attention pooling (include/nrx_embed.h, nrx_din_pool_fwd / _bwd) and the error bounds the
fp32 forms are held to.  Plain numpy, no torch, no GPU: every test of the operator and of the DIN model shares it.

Definition, with e_l = table[ids[b, l]] (an out-of-range id reads row 0), kept_l = mask is None or mask[b, l] != 0:
    s_l = dot(query_b, e_l) * scale          p = softmax over the kept l          out_b = sum_l p_l e_l          lse_b = log sum_kept exp(s_l)
    delta = dot(g_out_b, out_b)   dp_l = dot(g_out_b, e_l)   ds_l = p_l (dp_l - delta)
    g_query_b = scale sum_l ds_l e_l          g_rows[b, l] = p_l g_out_b + scale ds_l query_b   (0 for an entry not kept or out of range)
A sample with no kept entry: out = 0, lse = -inf, zero gradients.

Bounds (U = 2^-24, the unit roundoff of fp32; in the style of tests/attention_ref.py):
    E_s      = (D + 2) U max|query| max|table| scale       a score's absolute error: D products and sums, the scale, the subtraction of the maximum
    out      : (E_s + (L + D) U) sum_l p_l |e_l|           exp(s - m) carries E_s relatively; L terms in the two sums, D for the exp / divide / scale
    g_query, g_rows : (2 E_s + (L + 2 D) U) * the sum of the |terms| that make them up      (p and ds each carry a score error; dp is a D-term dot)
    lse      : 4 E_s + 8 U max(1, |lse|)
each plus 2^-126 (L + 1): products below the smallest normal number may be flushed or rounded to a subnormal."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


def din_pool_ref(table, ids, mask, query, scale, g_out=None):
    """All in float64.  Returns a dict: out [B, D], lse [B], p [B, L], and with g_out: g_query [B, D], g_rows [B, L, D]; plus the magnitudes
    the bounds multiply: a_out, a_gq, a_rows (sums of the absolute values of the terms) and `bad` [B, L] (ids out of range)."""
    table = np.asarray(table, dtype=np.float64)
    query = np.asarray(query, dtype=np.float64)
    ids = np.asarray(ids).astype(np.int64)
    B, L = ids.shape
    bad = (ids < 0) | (ids >= table.shape[0])
    e = table[np.where(bad, 0, ids)]                                   # [B, L, D]
    keep = np.ones((B, L), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    s = (e * query[:, None, :]).sum(-1) * scale
    s = np.where(keep, s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    m = np.where(np.isinf(m), 0.0, m)
    ex = np.exp(s - m)
    den = ex.sum(axis=1, keepdims=True)
    some = den > 0
    p = np.where(some, ex / np.where(some, den, 1.0), 0.0)
    out = (p[..., None] * e).sum(1)
    with np.errstate(divide="ignore"):
        lse = np.where(some, m + np.log(np.where(some, den, 1.0)), -np.inf)[:, 0]
    res = dict(out=out, lse=lse, p=p, bad=bad, keep=keep, a_out=(p[..., None] * np.abs(e)).sum(1))
    if g_out is not None:
        g = np.asarray(g_out, dtype=np.float64)
        delta = (g * out).sum(-1, keepdims=True)
        dp = (e * g[:, None, :]).sum(-1)
        ds = p * (dp - delta)
        give = (keep & ~bad)[..., None]
        res["g_query"] = scale * (ds[..., None] * e).sum(1)
        res["g_rows"] = np.where(give, p[..., None] * g[:, None, :] + scale * ds[..., None] * query[:, None, :], 0.0)
        a_dp = (np.abs(e) * np.abs(g)[:, None, :]).sum(-1)
        a_delta = (np.abs(g) * res["a_out"]).sum(-1, keepdims=True)
        a_ds = p * (a_dp + a_delta)
        res["a_gq"] = abs(scale) * (a_ds[..., None] * np.abs(e)).sum(1)
        res["a_rows"] = np.where(give, p[..., None] * np.abs(g)[:, None, :] + abs(scale) * a_ds[..., None] * np.abs(query)[:, None, :], 0.0)
    return res


def score_error(table, query, scale):
    D = np.asarray(query).shape[-1]
    return (D + 2) * U * float(np.abs(np.asarray(query, dtype=np.float64)).max(initial=0.0)) * \
        float(np.abs(np.asarray(table, dtype=np.float64)).max(initial=0.0)) * abs(scale)


def bounds(ref, table, query, scale):
    """Elementwise bounds of out / lse / g_query / g_rows for the reference `ref` of din_pool_ref (the gradient entries only if it has them)."""
    B, L = ref["p"].shape
    D = ref["out"].shape[1]
    es = score_error(table, query, scale)
    tiny = TINY * (L + 1)
    with np.errstate(invalid="ignore"):
        lse_mag = np.where(np.isinf(ref["lse"]), 1.0, np.maximum(1.0, np.abs(ref["lse"])))
    b = dict(out=(es + (L + D) * U) * ref["a_out"] + tiny, lse=4 * es + 8 * U * lse_mag + tiny)
    if "g_query" in ref:
        unit = 2 * es + (L + 2 * D) * U
        b["g_query"] = unit * ref["a_gq"] + tiny
        b["g_rows"] = unit * ref["a_rows"] + tiny
    return b


def table_grad_ref(ref, ids, rows, bnd=None):
    """The dense table gradient the per-lookup rows add up to: g_table[r] = sum over the lookups (b, l) of row r of g_rows[b, l] (row 0 and
    out-of-range ids get nothing).  With bnd (bounds()'s dict): also its bound -- the rows' bounds summed per table row, plus n U sum|g_rows| for
    the n - 1 fp32 additions of a row fed by n lookups."""
    ids = np.asarray(ids).astype(np.int64)
    D = ref["g_rows"].shape[-1]
    ok = (ids > 0) & (ids < rows)
    flat = ids[ok]
    g = np.zeros((rows, D))
    np.add.at(g, flat, ref["g_rows"][ok])
    if bnd is None:
        return g
    a = np.zeros((rows, D))
    np.add.at(a, flat, np.abs(ref["g_rows"][ok]))
    n = np.bincount(flat, minlength=rows).astype(np.float64)[:, None]
    bb = np.zeros((rows, D))
    np.add.at(bb, flat, bnd["g_rows"][ok])
    return g, bb + n * U * a + TINY


def worst_ratio(got, want, bound):
    """max |got - want| / bound (0 where both are -inf, e.g. the lse of an empty sample)."""
    got = np.asarray(got, dtype=np.float64)
    same_inf = np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want))
    with np.errstate(invalid="ignore"):
        err = np.where(same_inf, 0.0, np.abs(got - want))
    err = np.where(np.isnan(err), np.inf, err)
    return float((err / bound).max(initial=0.0))
