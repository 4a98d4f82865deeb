"""tests/fm_pool_ref.py held to account on the CPU, so that the GPU tests (tests/test_fm_pool_kernels_gpu.py) compare the kernels with something that
has itself been checked:
  * its float64 definitions are oracle/ref_np.py's formulas (which evaluate in float32: the comparison allows ref_np its own roundings, counted
    next to each assert) and reproduce the committed goldens of tests/golden/ops.npz within the tolerances tests/test_hip_parity.py uses;
  * every float32 restatement lies inside the derived bound around the definition (the bounds are not too tight);
  * dropping a field, keeping the squares, losing the 1/2, reading the first-order weight from column 1, S for S - v_f and a denominator without
    the mask all land outside the bounds on a majority of samples (the bounds are not so loose that they hide a structural mistake)."""
import os

import numpy as np
import pytest

from oracle import ref_np as R
from tests import fm_pool_ref as P
from tests.conftest import GOLDEN

F32 = np.float32
FM_IDS = [f"F{f}-D{d}" for f, d in P.FM_PAIRS]
POOL_IDS = [f"B{b}-L{l}-D{d}" for b, l, d in P.POOL_CASES]


def _golden():
    return dict(np.load(os.path.join(GOLDEN, "ops.npz"), allow_pickle=False))


def _ratio(got, ref, bound):
    """Largest |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------- the case lists say what they claim
def test_case_lists_reach_every_instantiation_and_edge():
    assert {P.fm_qlog2(d) for _, d in P.FM_PAIRS} == set(range(7))
    assert {f for f, _ in P.FM_PAIRS} >= {1, 7, 8, 9, 16, 17, 70}
    assert [P.fm_passes(d) for d in (256, 260, 300, 516)] == [1, 2, 2, 3]
    assert [(-(-d // 4) - 1) % 64 + 1 for d in (260, 300, 516)] == [1, 11, 1]          # chunks in the last pass
    for f, d in P.FM_PAIRS:
        tb = P.fm_tb(d)
        assert P.fm_batches(f, d) == sorted({b for b in (1, tb - 1, tb, tb + 1, 3 * tb + 5) if b >= 1})      # (nothing needed dropping)
        assert all(b * f * d <= P.FM_MAX_ELEMS for b in P.fm_batches(f, d))
    assert all(d % 4 == 0 for _, d in P.FM_VARIANT_PAIRS) and {16, 32, 128, 260} <= {d for _, d in P.FM_VARIANT_PAIRS}
    assert all(p in P.FM_PAIRS for p in P.FM_VARIANT_PAIRS)
    assert any(f >= 16 and f % 8 for f, _ in P.FM_VARIANT_PAIRS)                         # the 8-field body AND its tail, on the vector path
    cap = P.POOL_GRID_CAP
    assert (8193, 3, 64) in P.POOL_CASES and 8193 * 64 - cap * 256 == 64 and 8193 - cap * 4 == 1
    assert (8193, 2, 3) in P.POOL_CASES
    assert {-(-l // 64) for _, l, _ in P.POOL_CASES} >= {1, 2, 3} and (7, 64, 4) in P.POOL_CASES
    for b, l, d in P.POOL_CASES:
        _, _, masks = P.pool_inputs(b, l, d)
        m, w = masks["bin"], masks["w"]
        assert set(np.unique(m)) <= {0.0, 1.0} and np.all(w >= 0) and np.all((w > 0) <= (m > 0))
        assert not m[0].any() and (b == 1 or m[1].all())
        if l >= 2:
            partial = (m.sum(1) > 0) & (m.sum(1) < l)
            assert partial.sum() * 2 > b


# ------------------------------------------------------------------------------------------------- definitions = oracle/ref_np.py
@pytest.mark.parametrize("F,D", P.FM_PAIRS, ids=FM_IDS)
def test_fm_definitions_are_ref_np(F, D):
    """ref_np evaluates in float32 in numpy's order.  Its logit carries at most 2 (F - 1) + 1 + 1 + (D - 2) + 1 + 1 + 1 roundings (the field chain
    twice through the square, the square, the difference, the sum over k, the half, the first-order term, the bias): gamma(2 F + D + 8) M_i.  Its
    g_v = gl (S - v): F - 1 roundings on S (bounded by sum |v|), then two on |S| + |v| <= 2 sum |v|: gamma(F + 3) |gl| sum |v|.  g_w = gl."""
    for B in P.fm_batches(F, D):
        feat, gl, _ = P.fm_inputs(F, D, B)
        w, v = feat[:, :, 0], feat[:, :, 1:]
        ref = P.fm_logit64(feat)
        got = R.fm_logit(w, v, 0.0)[:, 0]
        assert np.all(np.abs(got - ref) <= P.gamma(2 * F + D + 8) * P.fm_logit_scale(feat))
        s64 = P.fm_sums64(feat)
        np.testing.assert_allclose(s64[:, 0] + 0.5 * ((s64[:, 1:] ** 2).sum(1) - (v.astype(np.float64) ** 2).sum((1, 2))), ref,
                                   rtol=0, atol=1e-12 * max(1.0, np.abs(P.fm_logit_scale(feat)).max()))
        gw, gv, _ = R.fm_logit_bwd(w, v, gl[:, None])
        g64 = P.fm_grad64(feat, gl)
        assert np.array_equal(gw.astype(np.float64), g64[:, :, 0])
        lim = P.gamma(F + 3) * np.abs(gl.astype(np.float64))[:, None, None] * np.abs(v.astype(np.float64)).sum(1, keepdims=True)
        assert np.all(np.abs(gv - g64[:, :, 1:]) <= lim)


@pytest.mark.parametrize("B,L,D", P.POOL_CASES, ids=POOL_IDS)
def test_pool_definitions_are_ref_np(B, L, D):
    """ref_np: a product, a sum over L, a sum of the mask, + 1e-8, a division -- at most L + 1 roundings on a numerator term and L + 1 on the
    denominator, plus the division: gamma(2 L + 3) sum |e m| / den forward, gamma(L + 3) |g m / den| backward."""
    emb, up, masks = P.pool_inputs(B, L, D)
    for tag in P.POOL_MASKS:
        m = masks[tag]
        m64 = np.ones((B, L)) if m is None else m.astype(np.float64)
        scale = (np.abs(emb.astype(np.float64)) * m64[:, :, None]).sum(1) / P.pool_den64(m, B, L)[:, None]
        assert np.all(np.abs(R.array_pool(emb, m) - P.pool_fwd64(emb, m)) <= P.gamma(2 * L + 3) * scale), tag
        ref = P.pool_bwd64(up, m, L)
        assert np.all(np.abs(R.array_pool_bwd(emb, m, up) - ref) <= P.gamma(L + 3) * np.abs(ref)), tag


# ------------------------------------------------------------------------------------------------- definitions = the reference's recorded results
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_fm_definitions_reproduce_the_goldens(tag):
    g = _golden()
    w, v = g[f"fm/{tag}/w"], g[f"fm/{tag}/v"]
    feat = np.concatenate([w[:, :, None], v], axis=2)
    s = 1.0 / (1.0 + np.exp(-(P.fm_logit64(feat)[:, None] + g[f"fm/{tag}/bias"].astype(np.float64).reshape(1, 1))))
    np.testing.assert_allclose(s, g[f"fm/{tag}/out"], rtol=1e-5, atol=1e-5)
    gl = (g[f"fm/{tag}/up"].astype(np.float64) * s * (1 - s))[:, 0]
    g64 = P.fm_grad64(feat, gl)
    np.testing.assert_allclose(g64[:, :, 0], g[f"fm/{tag}/gw"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g64[:, :, 1:], g[f"fm/{tag}/gv"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
@pytest.mark.parametrize("mtag", ["none", "bin", "w"])
def test_pool_definitions_reproduce_the_goldens(tag, mtag):
    g = _golden()
    emb = g[f"pool/{tag}/emb"]
    mask = {"none": None, "bin": g[f"pool/{tag}/mask"], "w": g[f"pool/{tag}/wmask"]}[mtag]
    np.testing.assert_allclose(P.pool_fwd64(emb, mask), g[f"pool/{tag}/{mtag}/out"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(P.pool_bwd64(g[f"pool/{tag}/up"], mask, emb.shape[1]), g[f"pool/{tag}/{mtag}/gemb"], rtol=1e-6, atol=1e-7)
    if mask is not None and not mask[0].any():
        assert np.all(P.pool_fwd32(emb, mask.astype(F32))[0] == 0.0)


# ------------------------------------------------------------------------------------------------- the bounds are not too tight
WORST = {}


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"fm_pool_ref worst error / bound: {key} {r:.4f}")


@pytest.mark.parametrize("F,D", P.FM_PAIRS, ids=FM_IDS)
def test_fm_restatements_lie_inside_the_bounds(F, D):
    """Worst |restatement - definition| / bound over the case list (this run, numpy on the CPU):
         logit, kernel order, plain                     0.089   (at F = 2, where the count has the least to cancel)
         logit, kernel order, fused                     0.094
         field sums (gamma(F - 1) sum |x|)              1.00    (F = 2: one rounding under a bound of one rounding)
         gradient without g_in                          0.52
         gradient with g_in, columns 1.., plain         0.47
         gradient with g_in, columns 1.., fused         0.44
         gradient with g_in, column 0 (up + gl)         1.00    (one rounding under a bound of one rounding)
    The field sums and the gradient without g_in are asked of the GPU bit for bit; their ratios only show that the bound they would fall back to
    holds.  The logit's roundings mostly cancel (the bound adds them up as if they never did): under a tenth of the bound is the factor one
    expects between a worst-case count over 2 F + P + 12 roundings and their random walk."""
    for B in P.fm_batches(F, D):
        feat, gl, g_in = P.fm_inputs(F, D, B)
        ref, bound = P.fm_logit64(feat), P.fm_logit_bound(feat)
        for fma in (False, True):
            r = _ratio(P.fm_logit32(feat, fma), ref, bound)
            _note(f"logit fma={fma}", r)
            assert r <= 1.0, (B, fma, r)
        r = _ratio(P.fm_sums32(feat), P.fm_sums64(feat), P.gamma(max(F - 1, 1)) * np.abs(feat.astype(np.float64)).sum(1))
        _note("sums", r)
        assert r <= 1.0 and (F > 1 or r == 0.0)
        r = _ratio(P.fm_grad32(feat, gl), P.fm_grad64(feat, gl), P.fm_grad_up_bound(feat, gl, np.zeros_like(g_in)))
        _note("grad", r)
        assert r <= 1.0
        ref, bound = P.fm_grad64(feat, gl, g_in), P.fm_grad_up_bound(feat, gl, g_in)
        for fma in (False, True):
            got = P.fm_grad32_up(feat, gl, g_in, fma)
            r = _ratio(got, ref, bound)
            assert r <= 1.0, (B, fma, r)
            _note(f"grad+g_in fma={fma} column 0", _ratio(got[:, :, 0], ref[:, :, 0], bound[:, :, 0]))
            if D > 1:
                _note(f"grad+g_in fma={fma} columns 1..", _ratio(got[:, :, 1:], ref[:, :, 1:], bound[:, :, 1:]))


@pytest.mark.parametrize("B,L,D", P.POOL_CASES, ids=POOL_IDS)
def test_pool_restatements_lie_inside_the_bounds(B, L, D):
    """Worst |restatement - definition| / bound over the case list (this run):
         forward (gamma(2 L + 1) sum |e m| / den: a product and L - 1 adds on a term, L on den, the division)       0.51
         backward, no mask, rtol (ceil(L/64) + 10) u              0.087
         backward, binary mask                                    0.080
         backward, weighted mask, the wavefront's order           0.29
    The forward and the none / binary backward are asked of the GPU bit for bit."""
    emb, up, masks = P.pool_inputs(B, L, D)
    for tag in P.POOL_MASKS:
        m = masks[tag]
        m64 = np.ones((B, L)) if m is None else m.astype(np.float64)
        scale = (np.abs(emb.astype(np.float64)) * m64[:, :, None]).sum(1) / P.pool_den64(m, B, L)[:, None]
        r = _ratio(P.pool_fwd32(emb, m), P.pool_fwd64(emb, m), P.gamma(2 * L + 1) * scale)
        _note("pool fwd", r)
        assert r <= 1.0, tag
        ref = P.pool_bwd64(up, m, L)
        got = P.pool_bwd32(up, m, L) if tag != "w" else P.pool_bwd32_lanes(up, m, L)
        r = _ratio(got, ref, P.pool_bwd_weighted_rtol(L) * np.abs(ref))
        _note(f"pool bwd {tag}", r)
        assert r <= 1.0, tag
        if tag == "bin":
            assert P.same_bits(P.pool_bwd32_lanes(up, m, L), got)          # binary: any order gives the same den
            assert np.all(P.pool_fwd32(emb, m)[0] == 0.0) and np.all(got[0] == 0.0)       # the all-zero row: exactly 0


# ------------------------------------------------------------------------------------------------- the bounds are not too loose
def _majority(err, bound, axis=None):
    """More than half of the samples (rows) hold an element outside the bound."""
    bad = err > bound
    rows = bad.reshape(bad.shape[0], -1).any(1)
    return rows.sum() * 2 > rows.size


@pytest.mark.parametrize("F,D", P.FM_PAIRS, ids=FM_IDS)
def test_fm_bounds_expose_structural_mistakes(F, D):
    """(D = 1 has no second-order term: nothing to get wrong there; the lost 1/2 needs two fields -- with one, the second-order term is 0.)"""
    if D == 1:
        for B in P.fm_batches(F, D):
            feat, _, _ = P.fm_inputs(F, D, B)
            assert np.array_equal(P.fm_logit64(feat), feat[:, :, 0].astype(np.float64).sum(1))
        return
    for B in P.fm_batches(F, D):
        feat, gl, g_in = P.fm_inputs(F, D, B)
        ref, bound = P.fm_logit64(feat), P.fm_logit_bound(feat)
        muts = [P.mut_logit_field_dropped, P.mut_logit_squares_kept, P.mut_logit_first_order_in_column_1]
        if F >= 2:
            muts.append(P.mut_logit_no_half)
        for mut in muts:
            assert _majority(np.abs(mut(feat) - ref), bound), (mut.__name__, B)
        for up in (None, g_in):
            ref = P.fm_grad64(feat, gl, up)
            bound = P.fm_grad_up_bound(feat, gl, np.zeros_like(g_in) if up is None else up)
            bad = np.abs(P.mut_grad_sum_not_reduced(feat, gl, up) - ref)[:, :, 1:] > bound[:, :, 1:]
            assert _majority(bad.astype(np.float64), 0.5), B
            assert bad.mean() > 0.5, B                                      # ... and of the elements, too


@pytest.mark.parametrize("B,L,D", P.POOL_CASES, ids=POOL_IDS)
def test_pool_bounds_expose_a_denominator_without_the_mask(B, L, D):
    """(L = 1: a row's mask is empty or full, and the two denominators then give the same result up to the 1e-8.)"""
    emb, up, masks = P.pool_inputs(B, L, D)
    for tag in ("bin", "w"):
        m = masks[tag]
        scale = (np.abs(emb.astype(np.float64)) * m.astype(np.float64)[:, :, None]).sum(1) / P.pool_den64(m, B, L)[:, None]
        err = np.abs(P.mut_pool_den_without_mask(emb, m) - P.pool_fwd64(emb, m))
        if L >= 2:
            assert _majority(err, P.gamma(2 * L + 1) * scale), tag
        # the backward: g m / L against g m / den
        ref = P.pool_bwd64(up, m, L)
        mut = up.astype(np.float64)[:, None, :] * m.astype(np.float64)[:, :, None] / float(L)
        if L >= 2:
            assert _majority(np.abs(mut - ref), P.pool_bwd_weighted_rtol(L) * np.abs(ref)), tag
