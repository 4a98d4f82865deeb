"""CPU checks of tests/afm_ref.py (the float64 restatement of the attentional pooling, nrx_afm_fwd / _bwd): its hand-written
gradients against torch float64 autograd of ops.afm_pool_math, afm_pool_math on CPU tensors, the properties of the dyadic input grids the GPU
test relies on, the bounds' behaviour, the exact score chain, and the case list's coverage.  No GPU is touched."""
import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from tests import afm_ref as R


def _torch_ref(d, D):
    x = torch.from_numpy(R.place(d["e"], d["offs"], d["width"], fill=0.0)).double().requires_grad_()
    ps = [torch.from_numpy(np.asarray(d[k], np.float64)).requires_grad_() for k in ("W1", "b1", "w2")]
    out = ops.afm_pool_math(x, d["offs"], D, *ps)
    out.backward(torch.from_numpy(d["g"]).double())
    return out, x, ps


@pytest.mark.parametrize("shape", [(2, 4, 1, 3), (3, 12, 5, 5), (9, 8, 7, 19), (5, 16, 33, 17)], ids=str)
@pytest.mark.parametrize("fields", R.FIELD_LAYOUTS)
def test_hand_written_gradients_agree_with_float64_autograd(shape, fields):
    F, D, A, B = shape
    c = dict(F=F, D=D, A=A, B=B, fields=fields, pad=0)
    d = R.case_data(c, seed=3, kind="gauss")
    out, x, ps = _torch_ref(d, D)
    (ge, gW1, gb1, gw2), _, f = R.backward(d["e"], d["W1"], d["b1"], d["w2"], d["g"])
    np.testing.assert_allclose(f["out"], out.detach().numpy(), rtol=1e-12, atol=1e-13)
    gx = x.grad.numpy()
    for k, o in enumerate(d["offs"]):
        np.testing.assert_allclose(ge[:, k], gx[:, o:o + D], rtol=1e-10, atol=1e-12)
    mask = np.ones(d["width"], bool)
    for o in d["offs"]:
        mask[o:o + D] = False
    assert not gx[:, mask].any()                                  # zero outside the fields
    for mine, p in zip((gW1, gb1, gw2), ps):
        np.testing.assert_allclose(mine, p.grad.numpy(), rtol=1e-10, atol=1e-12)
    lse = torch.logsumexp(torch.from_numpy(f["a"]), 1).numpy()
    np.testing.assert_allclose(f["lse"], lse, rtol=1e-13)


def test_afm_pool_takes_the_math_form_on_cpu_tensors_and_other_dtypes():
    torch.manual_seed(0)
    n0 = ops.afm_calls
    x = torch.randn(5, 40, requires_grad=True)
    w1, b1, w2 = torch.randn(6, 8), torch.randn(6), torch.randn(6)
    offs = [0, 8, 24, 32]
    a, b = ops.afm_pool(x, offs, 8, w1, b1, w2), ops.afm_pool_math(x, offs, 8, w1, b1, w2)
    assert torch.equal(a, b) and a.shape == (5, 8) and ops.afm_calls == n0
    a.sum().backward()
    assert not x.grad[:, 16:24].any() and x.grad[:, :16].any()
    assert ops.afm_pool(x.double(), 5, 8, w1.double(), b1.double(), w2.double()).dtype == torch.float64
    with pytest.raises(ValueError, match="w1 must be"):
        ops.afm_pool(x, offs, 8, torch.randn(6, 4), b1, w2)
    with pytest.raises(ValueError, match="b1 and w2"):
        ops.afm_pool(x, offs, 8, w1, b1[:5], w2)
    with pytest.raises(ValueError, match="leaves the 40 columns"):
        ops.afm_pool(x, [0, 36], 8, w1, b1, w2)
    assert [ops.afm_supported(*s) for s in ((2, 4, 1), (64, 64, 64), (1, 4, 1), (65, 4, 1), (2, 6, 1), (2, 68, 1), (2, 4, 0), (2, 4, 65))] \
        == [True, True, False, False, False, False, False, False]


def test_uniform_weights_when_w2_is_zero():
    c = dict(F=5, D=8, A=3, B=2, fields="adjacent", pad=0)
    d = R.case_data(c)
    f = R.forward(d["e"], d["W1"], d["b1"], np.zeros(3, np.float32), exp_rel=0.0)
    assert np.array_equal(f["alpha"], np.full((2, 10), 0.1)) and not f["ea"].any()
    np.testing.assert_allclose(f["out"], (d["e"][:, f["ii"]].astype(np.float64) * d["e"][:, f["jj"]]).mean(1), rtol=1e-14)
    assert np.allclose(f["lse"], np.log(10))
    # the exp-free bound: the division, the sum and the pooling chain only -- a few dozen roundings of the magnitudes
    mag = np.abs(d["e"][:, f["ii"]].astype(np.float64) * d["e"][:, f["jj"]]).mean(1)
    assert (f["e_out"] <= 40 * R.U * mag + 1e-30).all()
    full = R.forward(d["e"], d["W1"], d["b1"], np.zeros(3, np.float32))
    assert (full["e_out"] >= f["e_out"]).all() and (full["e_out"] > f["e_out"]).any()


def test_dyadic_grids_make_every_preactivation_exact_and_clear_of_the_kink():
    """|z| >= 2^-8 and z a multiple of 2^-8 below 2^24 * 2^-8: exact in fp32 whatever the summation order -- at the largest shape too."""
    for c in (dict(F=64, D=64, A=64, B=2, fields="adjacent", pad=0), dict(F=9, D=12, A=5, B=5, fields="permuted", pad=0)):
        d = R.case_data(c)
        f = R.forward(d["e"], d["W1"], d["b1"], d["w2"])
        z = f["z"] * 256
        assert np.array_equal(z, np.round(z)) and (np.abs(z) >= 1).all() and (np.round(z) % 2 != 0).all()
        # every partial sum is bounded by the sum of magnitudes: below 2^24 in units of 2^-8
        assert (np.abs(f["h"]) @ np.abs(d["W1"].astype(np.float64)).T + np.abs(d["b1"])).max() * 256 < 2 ** 24
        P = c["F"] * (c["F"] - 1) // 2
        assert R.keeps_pairs(f, P)


def test_bounds_scale_with_the_chain_lengths_and_stay_small():
    c = dict(F=9, D=16, A=16, B=17, fields="adjacent", pad=0)
    d = R.case_data(c, kind="gauss")
    (ge, gW1, gb1, gw2), (e_ge, eW1, eb1, ew2), f = R.backward(d["e"], d["W1"], d["b1"], d["w2"], d["g"])
    for v, b in ((f["out"], f["e_out"]), (ge, e_ge), (gW1, eW1), (gb1, eb1), (gw2, ew2)):
        assert (b > 0).all() and np.median(b / (np.abs(v) + 1e-30)) < 1e-2      # not vacuous: the batch sums cancel, their bounds do not
    assert (f["e_lse"] < 1e-4).all()
    # two slices: the bound of one slice of 17 would lack the slice add
    _, (_, eW1_one, _, _), _ = R.backward(d["e"], d["W1"], d["b1"], d["w2"], d["g"], slice_samples=17)
    assert eW1.shape == eW1_one.shape
    assert R.gamma(10) > 10 * R.U and R.min_margin(f) >= 0


def test_score_chain_is_the_float64_score_to_within_its_bound_and_exact_on_dyadic_inputs():
    c = dict(F=2, D=12, A=5, B=3, fields="adjacent", pad=0)
    d = R.case_data(c)
    f = R.forward(d["e"], d["W1"], d["b1"], d["w2"])
    for b in range(3):
        z, a = R.score_chain(d["e"][b, 1], d["e"][b, 0], d["W1"], d["b1"], d["w2"])
        assert np.array_equal(z.astype(np.float64), f["z"][b, 0])                # dyadic: exact
        assert abs(float(a) - f["a"][b, 0]) <= f["ea"][b, 0] + 1e-300
    g = R.case_data(c, kind="gauss")
    fg = R.forward(g["e"], g["W1"], g["b1"], g["w2"])
    z, a = R.score_chain(g["e"][0, 1], g["e"][0, 0], g["W1"], g["b1"], g["w2"])
    assert (np.abs(z - fg["z"][0, 0]) <= fg["ez"][0, 0]).all() and abs(float(a) - fg["a"][0, 0]) <= fg["ea"][0, 0]


def test_case_list_covers_every_named_value():
    cs = R.cases()
    assert 38 <= len(cs) <= 45
    assert {c["F"] for c in cs} == {2, 3, 8, 9, 26, 32, 33, 64}
    assert {c["D"] for c in cs} == {4, 12, 16, 20, 32, 36, 64}
    assert {c["A"] for c in cs} == {1, 5, 16, 31, 32, 33, 64}
    assert {1, 2, 3, 5, 67, R.SLICE, R.SLICE + 1} <= {c["B"] for c in cs}
    assert (2, 4, 1) in {(c["F"], c["D"], c["A"]) for c in cs} and (64, 64, 64) in {(c["F"], c["D"], c["A"]) for c in cs}
    assert {c["fields"] for c in cs} == set(R.FIELD_LAYOUTS) and {c["pad"] for c in cs} == {0, 3, 4, 8}
    assert len({R.case_id(c) for c in cs}) == len(cs)
    assert R.WRAP["B"] > R.GRID_WAVES * R.SLICE
    for c in cs:                                                   # the scaling of w2 reached its goal at every shape
        if c["F"] <= 9:
            d = R.case_data(c)
            assert R.keeps_pairs(R.forward(d["e"], d["W1"], d["b1"], d["w2"]), c["F"] * (c["F"] - 1) // 2), R.case_id(c)
    for F, D, A, B in R.GAUSS_BWD:
        d = R.case_data(dict(F=F, D=D, A=A, B=B, fields="adjacent", pad=0), kind="gauss")
        assert R.min_margin(R.forward(d["e"], d["W1"], d["b1"], d["w2"])) > 100, (F, D, A, B)
