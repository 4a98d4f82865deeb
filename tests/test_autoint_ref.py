"""tests/autoint_ref.py against torch: its hand-written float64 gradients equal float64 autograd of ops.interacting_layer_math to float64 rounding,
and the math form run in fp32 on the CPU stays inside the derived bounds (so the bounds are not vacuous: an fp32 evaluation in another order
meets them, with the worst error / bound printed)."""
import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from tests import autoint_ref as R

SMALL = [c for c in R.cases() if c["B"] * c["F"] * c["F"] * c["heads"] <= 70000]


def _torch_inputs(d, dtype):
    x = torch.from_numpy(R.place(d["x"], d["offs"], d["width"], fill=0.0)).to(dtype).requires_grad_()
    ws = [None if d[k] is None else torch.from_numpy(d[k]).to(dtype).requires_grad_() for k in ("Wq", "Wk", "Wv", "Wres")]
    return x, ws


def _cols(offs, din):
    return np.concatenate([np.arange(o, o + din) for o in offs])


def _run_math(c, d, dtype):
    x, ws = _torch_inputs(d, dtype)
    out = ops.interacting_layer_math(x, d["offs"], c["din"], *ws, heads=c["heads"], scale=d["scale"])
    out.backward(torch.from_numpy(d["g"]).to(dtype))
    B, F = d["x"].shape[:2]
    gx = x.grad.numpy()[:, _cols(d["offs"], c["din"])].reshape(B, F, c["din"])
    return out.detach().numpy(), gx, [None if w is None else w.grad.numpy() for w in ws]


@pytest.mark.parametrize("c", SMALL, ids=R.case_id)
def test_hand_written_gradients_equal_float64_autograd(c):
    d = R.case_data(c)
    out, gx, gws = _run_math(c, d, torch.float64)
    (rgx, *rgw), _, f = R.backward(d["x"], d["Wq"], d["Wk"], d["Wv"], d["Wres"], c["heads"], d["scale"], d["g"])
    B, F = d["x"].shape[:2]
    np.testing.assert_allclose(out.reshape(B, F, -1), f["out"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gx, rgx, rtol=1e-10, atol=1e-11)
    for got, ref in zip(gws, rgw):
        assert (got is None) == (ref is None)
        if ref is not None:
            np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10)


def test_the_mask_is_a_parameter_of_the_backward():
    c = dict(F=3, din=4, heads=1, hd=4, B=5, fields="adjacent", pad=0, res=True, scaled=False)
    d = R.case_data(c)
    ones = np.ones((5, 3, 4), bool)
    (gx1, *_), _, f = R.backward(d["x"], d["Wq"], d["Wk"], d["Wv"], d["Wres"], 1, 1.0, d["g"], mask=ones)
    (gx0, *_), _, _ = R.backward(d["x"], d["Wq"], d["Wk"], d["Wv"], d["Wres"], 1, 1.0, d["g"])
    assert not (f["pre"] > 0).all() and not np.allclose(gx0, gx1)
    (gxz, *gwz), _, _ = R.backward(d["x"], d["Wq"], d["Wk"], d["Wv"], d["Wres"], 1, 1.0, d["g"], mask=~ones)
    assert not gxz.any() and not any(g.any() for g in gwz)


@pytest.mark.parametrize("c", SMALL, ids=R.case_id)
def test_fp32_math_form_stays_inside_the_bounds(c):
    d = R.case_data(c, seed=3)
    out, gx, gws = _run_math(c, d, torch.float32)
    B, F = d["x"].shape[:2]
    out = out.reshape(B, F, -1)
    # the fp32 run's own mask; it may differ from the float64 one only where the pre-activation lies within its forward bound
    (rgx, *rgw), (egx, *egw), f = R.backward(d["x"], d["Wq"], d["Wk"], d["Wv"], d["Wres"], c["heads"], d["scale"], d["g"], mask=out > 0)
    flipped = (out > 0) != (f["pre"] > 0)
    assert (np.abs(f["pre"][flipped]) <= f["e_pre"][flipped]).all()
    worst = float((np.abs(out - f["out"]) / f["e_pre"]).max())
    assert worst <= 1
    pairs = [(gx, rgx, egx)] + [(g, r, e) for g, r, e in zip(gws, rgw, egw) if r is not None]
    for got, ref, bound in pairs:
        ratio = float((np.abs(got - ref) / bound).max())
        assert ratio <= 1, ratio
        worst = max(worst, ratio)
    print(f"autoint cpu fp32 worst error / bound: {R.case_id(c)} {worst:.4f}")
    assert worst > 1e-4            # not vacuous: an fp32 evaluation comes within four orders of magnitude of the bound


def test_slice_and_support_envelope():
    assert R.wgrad_slice(26, 16, 2, 16) == 64 and R.wgrad_slice(26, 64, 2, 32) == 16 and R.wgrad_slice(2, 64, 4, 4) == 64
    ok = ops.interacting_layer_supported
    assert ok(2, 4, 1, 4) and ok(64, 64, 1, 64) and ok(64, 64, 16, 4) and ok(39, 16, 2, 16) and ok(26, 12, 2, 12)
    assert not ok(1, 4, 1, 4) and not ok(65, 4, 1, 4) and not ok(2, 6, 1, 4) and not ok(2, 68, 1, 4) and not ok(2, 4, 1, 6)
    assert not ok(2, 4, 5, 16) and not ok(2, 4, 1, 2) and not ok(2, 4, 0, 4)
