"""tests/cin_ref.py held to an independent restatement (torch float64 einsum, torch autograd), ops.cin_math on CPU tensors held to cin_ref, and the
emulated fp32 chains of include/nrx_embed.h inside cin_ref's bounds.  No GPU is touched."""
import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from tests import cin_ref as R

SHAPES = [(3, None, 4, 4, 2), (2, 5, 3, 12, 3), (5, 3, 7, 8, 2), (26, 32, 32, 16, 2)]          # (m, Hp, H, D, B)


def _data(m, Hp, H, D, B, seed=0, gxk_null=False, acc=True):
    c = dict(m=m, Hp=Hp, H=H, D=D, B=B, fields="adjacent", xk_null=False, gxk_null=gxk_null, acc=acc, p_off=0)
    return R.case_data(c, seed=seed)


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@pytest.mark.parametrize("m, Hp, H, D, B", SHAPES)
def test_the_restatement_matches_torch_float64_einsum_and_autograd(m, Hp, H, D, B):
    d = _data(m, Hp, H, D, B)
    layer1 = d["Xp"] is None
    X0 = _t(d["X0"]).requires_grad_(True)
    Xp = X0 if layer1 else _t(d["Xp"]).requires_grad_(True)
    W = _t(d["W"]).requires_grad_(True)
    xk = torch.einsum("hij,bijd->bhd", W, torch.einsum("bid,bjd->bijd", Xp, X0))
    p = xk.sum(-1)
    (ref_xk, ref_p), (e_xk, e_p) = R.layer_fwd(d["X0"], d["X0"] if layer1 else d["Xp"], d["W"])
    np.testing.assert_allclose(ref_xk, xk.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref_p, p.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert (e_xk > 0).all() and (e_p > 0).all()
    ((p * _t(d["g_p"])).sum() + (xk * _t(d["g_xk"])).sum()).backward()
    (g_xp, g_x0), _ = R.layer_bwd(d["X0"], d["X0"] if layer1 else d["Xp"], d["W"], d["g_p"], d["g_xk"], up=d["up"], layer1=layer1)
    np.testing.assert_allclose(g_x0, X0.grad.numpy() + d["up"], rtol=1e-12, atol=1e-12)
    if not layer1:
        np.testing.assert_allclose(g_xp, Xp.grad.numpy(), rtol=1e-12, atol=1e-12)
    for sl in (1, 2, B + 3):
        g_W, e_W = R.layer_gw(d["X0"], d["X0"] if layer1 else d["Xp"], d["g_p"], d["g_xk"], sl)
        np.testing.assert_allclose(g_W, W.grad.numpy(), rtol=1e-12, atol=1e-11)
        assert (e_W > 0).all()


@pytest.mark.parametrize("m, D, sizes", [(3, 4, (4,)), (4, 8, (6, 5)), (5, 4, (3, 7, 2))])
def test_cin_math_on_cpu_tensors_is_the_composition_of_the_restated_layers(m, D, sizes):
    rng = np.random.default_rng(m + D)
    B = 3
    offs, width = R.layout(m, D, "interleaved", seed=2)
    x = rng.standard_normal((B, width))
    ws, Hp = [], m
    for H in sizes:
        ws.append(rng.standard_normal((H, Hp, m)))
        Hp = H
    X0 = np.stack([x[:, o:o + D] for o in offs], axis=1)
    Xp, pooled = X0, []
    for W in ws:
        (Xp, p), _ = R.layer_fwd(X0, Xp, W)
        pooled.append(p)
    want = np.concatenate(pooled, axis=1)
    got = ops.cin_math(torch.from_numpy(x), offs, D, [torch.from_numpy(w) for w in ws])
    assert got.dtype == torch.float64 and got.shape == (B, ops.cin_out_width(sizes))
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    # the op itself takes the same path for CPU tensors, in the dtype of x; and it is differentiable
    xt = torch.from_numpy(x.astype(np.float32)).requires_grad_(True)
    wt = [torch.from_numpy(w.astype(np.float32)).requires_grad_(True) for w in ws]
    out = ops.cin(xt, offs, D, wt)
    assert out.dtype == torch.float32 and torch.equal(out, ops.cin_math(xt, offs, D, wt))
    np.testing.assert_allclose(out.detach().numpy(), want, rtol=1e-3, atol=1e-3)
    out.sum().backward()
    assert xt.grad is not None and all(w.grad is not None for w in wt)
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        ops.cin_math(torch.from_numpy(x), offs, D, [torch.from_numpy(ws[0]), torch.zeros(2, sizes[0] + 1, m)])


@pytest.mark.parametrize("m, Hp, H, D, B", [(3, None, 3, 4, 2), (2, 5, 3, 4, 2), (3, 3, 2, 8, 5)])
def test_the_emulated_chains_lie_within_the_bounds(m, Hp, H, D, B):
    for gxk_null, acc, sl in ((False, True, 2), (True, False, 64)):
        d = _data(m, Hp, H, D, B, seed=5, gxk_null=gxk_null, acc=acc)
        layer1 = d["Xp"] is None
        Xp = d["X0"] if layer1 else d["Xp"]
        (ref_xk, ref_p), (e_xk, e_p) = R.layer_fwd(d["X0"], Xp, d["W"])
        xk, p = R.fwd_chain(d["X0"], Xp, d["W"])
        assert (np.abs(xk - ref_xk) <= e_xk).all() and (np.abs(p - ref_p) <= e_p).all()
        assert np.abs(xk - ref_xk).max() > 0          # (fp32 chains: not the float64 values themselves)
        (r_xp, r_x0), (e_xp, e_x0) = R.layer_bwd(d["X0"], Xp, d["W"], d["g_p"], d["g_xk"], up=d["up"], layer1=layer1)
        g_xp, g_x0 = R.bwd_chain(d["X0"], Xp, d["W"], d["g_p"], d["g_xk"], up=d["up"], layer1=layer1)
        assert (np.abs(g_x0 - r_x0) <= e_x0).all()
        assert layer1 or (np.abs(g_xp - r_xp) <= e_xp).all()
        r_W, e_W = R.layer_gw(d["X0"], Xp, d["g_p"], d["g_xk"], sl)
        assert (np.abs(R.gw_chain(d["X0"], Xp, d["g_p"], d["g_xk"], sl) - r_W) <= e_W).all()


def test_small_integers_leave_the_chains_exact():
    c = dict(m=3, Hp=2, H=3, D=4, B=3, fields="adjacent", xk_null=False, gxk_null=False, acc=True, p_off=0)
    d = R.case_data(c, ints=True)
    (ref_xk, ref_p), _ = R.layer_fwd(d["X0"], d["Xp"], d["W"])
    xk, p = R.fwd_chain(d["X0"], d["Xp"], d["W"])
    assert np.array_equal(xk, ref_xk) and np.array_equal(p, ref_p)
    (r_xp, r_x0), _ = R.layer_bwd(d["X0"], d["Xp"], d["W"], d["g_p"], d["g_xk"], up=d["up"])
    g_xp, g_x0 = R.bwd_chain(d["X0"], d["Xp"], d["W"], d["g_p"], d["g_xk"], up=d["up"])
    assert np.array_equal(g_xp, r_xp) and np.array_equal(g_x0, r_x0)
    assert np.array_equal(R.gw_chain(d["X0"], d["Xp"], d["g_p"], d["g_xk"], 2), R.layer_gw(d["X0"], d["Xp"], d["g_p"], d["g_xk"], 2)[0])


def test_the_case_list_covers_what_it_says():
    cs = R.cases()
    assert 30 <= len(cs) <= 60 and len({R.case_id(c) for c in cs}) == len(cs)
    assert {c["D"] for c in cs} >= {4, 12, 16, 20, 32, 36, 64} and {c["m"] for c in cs} >= {2, 3, 26, 33, 64}
    assert {c["Hp"] for c in cs} >= {None, 1, 5, 32, 33, 64} and {c["H"] for c in cs} >= {1, 31, 32, 33, 64}
    assert {c["B"] for c in cs} >= {1, 2, 3, 5, 67} and any(((c["Hp"] or c["m"]) * c["m"]) % 2 for c in cs)
    assert {c["fields"] for c in cs} == set(R.FIELD_LAYOUTS)
    for key in ("xk_null", "gxk_null", "acc"):
        assert {c[key] for c in cs} == {False, True}
    assert any(c["p_off"] > 0 for c in cs)
