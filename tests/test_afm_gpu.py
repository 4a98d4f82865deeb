"""The attentional-pooling kernels of csrc/nrx_afm.hip alone, through the C ABI (nrx_afm_fwd / _bwd), at the edges of their launch arithmetic
(tests/afm_ref.py lists them: P = 1 .. 2016 pairs around the 32-pair tile, dim dividing 64 and not, one and two row tiles of A, 1 .. 67 samples,
a batch that wraps the grid loop, one weight-gradient slice, one plus a sample, several), adjacent, permuted and interleaved fields, padded
out / g_out / g_x strides -- against the float64 restatement and the bounds derived there (asserted as derived; each test prints its worst
error / bound, pytest -s shows them).
Every buffer is the head of a larger allocation filled with NaN, gaps between fields included: a read outside an input would poison a result,
and every float that is not a result must hold the very bits it held before the call.
The launch-shape cases draw from dyadic grids on which every pre-activation is exact in fp32 and at least 2^-8 from the ReLU kink, so the
activation pattern is the float64 one by construction (asserted on the reference).  Then: gaussian inputs (forward everywhere, backward where
the reference stays 100 bounds clear of the kink), uniform weights at w2 = 0, the score chains bit for bit, scores of +-1e4, the same bits run
to run, alone or inside a batch, replayed from a graph; ops.afm_pool's autograd, views, fallbacks and allocator peak."""
import ctypes

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd._lib import NRX_OK
from tests import afm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CASES = R.cases()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == NRX_OK, (what, rc, _lib.load().nrx_last_error())
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _round4(n):
    return (n + 3) // 4 * 4


def _ratio(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    assert not np.isnan(err).any(), "NaN in a result: a sentinel was read"
    rel = err / np.maximum(bound, 1e-300)                      # (a result that is exactly 0 by its inputs has a bound of 0)
    assert (err <= bound).all(), f"worst error / bound {float(rel.max()):.3f}"
    return float(rel.max()) if err.size else 0.0


def _note(key, r):
    print(f"afm gpu worst error / bound: {key} {r:.4f}")


def _off_arr(offs):
    return (ctypes.c_int32 * len(offs))(*offs)


class Arena:
    """[rows, ld] floats starting `off` floats into a NaN-filled device allocation that goes on for more than a row past the last one."""

    def __init__(self, rows, ld, off=0, data=None):
        self.rows, self.ld, self.off = rows, ld, off
        self.host = np.full(off + rows * ld + ld + 67, np.nan, F32)
        if data is not None:
            self.body()[:, :data.shape[1]] = data
        self.t = torch.from_numpy(self.host).to(DEV)

    def body(self, host=None):
        host = self.host if host is None else host
        return host[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    def take(self, cols):
        """The [rows, cols] block `cols` (a column index array) after the call; every other float must hold the bits it was uploaded with."""
        after = self.t.cpu().numpy()
        vals = self.body(after)[:, cols].copy()
        self.body(after)[:, cols] = self.body()[:, cols]
        assert np.array_equal(_bits(after), _bits(self.host)), "a float outside the result was written"
        return vals


def _field_cols(offs, D):
    return np.concatenate([np.arange(o, o + D) for o in offs])


def run(c, d, bwd=True):
    """dict(out [B, D], lse [B], ge [B, F, D], gW1, gb1, gw2) of a case on its data, through the C ABI; every input and every float around the
    outputs checked for untouched bits.  The backward reads the out and lse the forward wrote."""
    lib = _lib.load()
    F, D, A, B = c["F"], c["D"], c["A"], d["e"].shape[0]
    ld = _round4(d["width"])
    pad = c["pad"]
    xa = Arena(B, ld, data=R.place(d["e"], d["offs"], d["width"]))
    w1a, b1a, w2a = Arena(1, A * D, off=1, data=d["W1"].reshape(1, -1)), Arena(1, A, off=2, data=d["b1"][None]), Arena(1, A, off=3, data=d["w2"][None])
    oa, la = Arena(B, D + pad, off=1), Arena(1, B, off=1)
    off = _off_arr(d["offs"])
    _ok(lib.nrx_afm_fwd(xa.ptr, ld, off, F, D, w1a.ptr, b1a.ptr, w2a.ptr, A, B, oa.ptr, D + pad, la.ptr, _stream()), "nrx_afm_fwd")
    res = dict(out=oa.take(np.arange(D)), lse=la.take(np.arange(B))[0])
    for a in (xa, w1a, b1a, w2a):
        a.take(np.arange(0))
    if not bwd:
        return res
    oin, lin = Arena(B, D + pad, data=res["out"]), Arena(1, B, off=1, data=res["lse"][None])
    ga = Arena(B, D + (pad + 1) // 2, off=1, data=d["g"])
    gx = Arena(B, ld + 4 * (pad % 3))
    gw1, gb1, gw2 = Arena(1, A * D, off=1), Arena(1, A, off=2), Arena(1, A, off=3)
    nws = lib.nrx_afm_bwd_workspace(B, F, D, A)
    sl = lib.nrx_afm_wgrad_slice(F, D, A)
    assert sl == R.SLICE and nws == -(-B // sl) * (A * D + 2 * A) * 4
    wsp = torch.full((nws // 4 + 16,), float("nan"), device=DEV)
    _ok(lib.nrx_afm_bwd(xa.ptr, ld, off, F, D, w1a.ptr, b1a.ptr, w2a.ptr, A, B, oin.ptr, D + pad, lin.ptr, ga.ptr, ga.ld, gx.ptr, gx.ld, gw1.ptr, gb1.ptr,
                        gw2.ptr, wsp.data_ptr(), _stream()), "nrx_afm_bwd")
    assert torch.isnan(wsp[nws // 4:]).all(), "a float past the workspace was written"
    res.update(ge=gx.take(_field_cols(d["offs"], D)).reshape(B, F, D), gW1=gw1.take(np.arange(A * D)).reshape(A, D), gb1=gb1.take(np.arange(A))[0],
               gw2=gw2.take(np.arange(A))[0])
    for a in (xa, w1a, b1a, w2a, oin, lin, ga):
        a.take(np.arange(0))
    return res


def _check(key, res, d, bwd=True, exp_rel=R.EXP_REL):
    (ge, gW1, gb1, gw2), (e_ge, eW1, eb1, ew2), f = R.backward(d["e"], d["W1"], d["b1"], d["w2"], d["g"], exp_rel=exp_rel)
    worst = max(_ratio(res["out"], f["out"], f["e_out"]), _ratio(res["lse"], f["lse"], f["e_lse"]))
    if bwd:
        worst = max(worst, _ratio(res["ge"], ge, e_ge), _ratio(res["gW1"], gW1, eW1), _ratio(res["gb1"], gb1, eb1), _ratio(res["gw2"], gw2, ew2))
    _note(key, worst)
    return f


@pytest.mark.parametrize("c", CASES + [R.WRAP], ids=R.case_id)
def test_launch_shapes_on_the_dyadic_grids(c):
    d = R.case_data(c)
    f = _check(R.case_id(c), run(c, d), d)
    # the grids' promise, on the reference: every z exact in fp32 in any order (a multiple of 2^-8, the magnitudes sum below 2^24 of them), odd
    z = f["z"] * 256
    assert np.array_equal(z, np.round(z)) and (np.abs(z) >= 1).all()
    assert (np.abs(f["h"]) @ np.abs(d["W1"].astype(np.float64)).T + np.abs(d["b1"])).max() * 256 < 2 ** 24
    assert R.keeps_pairs(f, c["F"] * (c["F"] - 1) // 2)


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_forward_on_gaussian_inputs(c):
    d = R.case_data(c, seed=1, kind="gauss")
    _check("gauss fwd " + R.case_id(c), run(c, d, bwd=False), d, bwd=False)


@pytest.mark.parametrize("shape", R.GAUSS_BWD, ids=str)
def test_forward_and_backward_on_gaussian_inputs(shape):
    F, D, A, B = shape
    c = dict(F=F, D=D, A=A, B=B, fields="interleaved", pad=4)
    d = R.case_data(c, kind="gauss")
    f = _check(f"gauss fwd+bwd {shape}", run(c, d), d)
    assert R.min_margin(f) > 100            # the float64 min |z| is 100 of its fp32 bounds from the kink: the patterns agree


def test_w2_zero_gives_uniform_weights_within_the_exp_free_bound():
    c = dict(F=9, D=12, A=5, B=5, fields="permuted", pad=3)
    d = R.case_data(c)
    d["e"] = np.random.default_rng(5).integers(-3, 4, d["e"].shape).astype(F32)
    d["w2"] = np.zeros(5, F32)
    res = run(c, d)
    f0 = R.forward(d["e"], d["W1"], d["b1"], d["w2"], exp_rel=0.0)            # every argument of expf is 0 and expf(0) = 1: no exp term
    assert np.array_equal(f0["alpha"], np.full_like(f0["alpha"], 1 / 36))
    _note("w2 = 0, out against the exp-free bound", _ratio(res["out"], f0["out"], f0["e_out"]))
    _check("w2 = 0", res, d)
    assert not res["gW1"].any() and not res["gb1"].any()                      # u = da w2 = 0


@pytest.mark.parametrize("DA", R.EXACT, ids=str)
def test_scores_reproduce_the_headers_chains_bit_for_bit(DA):
    """P = 1: alpha = fl(E / E) = 1, lse = fl(a + logf(1)) = a and out = fmaf(1, h, 0) = h: the score chain is read off lse, debug-free."""
    D, A = DA
    c = dict(F=2, D=D, A=A, B=6, fields="interleaved", pad=3)
    d = R.case_data(c, seed=2, kind="gauss")
    res = run(c, d, bwd=False)
    for b in range(6):
        _, a = R.score_chain(d["e"][b, 1], d["e"][b, 0], d["W1"], d["b1"], d["w2"])
        assert _bits(res["lse"][b]) == _bits(a), (b, res["lse"][b], a)
    assert np.array_equal(_bits(res["out"]), _bits(d["e"][:, 1] * d["e"][:, 0]))


@pytest.mark.parametrize("sign", [1, -1], ids=["plus", "minus"])
def test_scores_of_1e4_stay_finite(sign):
    c = dict(F=9, D=16, A=16, B=5, fields="adjacent", pad=0)
    d = R.case_data(c)
    d["w2"] = np.abs(d["w2"])                                                   # scores of one sign: a = sum w2 relu(z) >= 0
    f0 = R.forward(d["e"], d["W1"], d["b1"], d["w2"])
    d["w2"] = (d["w2"] * F32(sign * 1e4 / f0["a"].max())).astype(F32)
    f = R.forward(d["e"], d["W1"], d["b1"], d["w2"])
    assert np.abs(f["a"]).max() > 9.9e3 and (sign * f["a"] >= 0).all() and np.ptp(f["a"]) > 5e3
    res = run(c, d)
    assert all(np.isfinite(v).all() for v in res.values())
    _ratio(res["out"], f["out"], f["e_out"])
    _ratio(res["lse"], f["lse"], f["e_lse"])


def test_same_bits_run_to_run_and_alone_or_inside_a_batch():
    c = dict(F=26, D=16, A=16, B=37, fields="interleaved", pad=4)
    d = R.case_data(c, kind="gauss")
    r1, r2 = run(c, d), run(c, d)
    for k in r1:
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), k
    b = 21
    one = {k: (v[b:b + 1] if k in ("e", "g") else v) for k, v in d.items()}
    ra = run(dict(c, B=1), one)
    for k in ("out", "lse", "ge"):
        assert np.array_equal(_bits(ra[k][0]), _bits(r1[k][b])), k


def _torch_inputs(d, dtype, dev):
    x = torch.from_numpy(R.place(d["e"], d["offs"], d["width"], fill=0.0)).to(dev, dtype).requires_grad_()
    ps = [torch.from_numpy(d[k]).to(dev, dtype).requires_grad_() for k in ("W1", "b1", "w2")]
    return x, ps


def test_ops_autograd_views_and_fallbacks():
    c = dict(F=9, D=16, A=5, B=19, fields="interleaved", pad=0)
    d = R.case_data(c, kind="gauss")
    (ge, gW1, gb1, gw2), (e_ge, eW1, eb1, ew2), f = R.backward(d["e"], d["W1"], d["b1"], d["w2"], d["g"])
    x, ps = _torch_inputs(d, torch.float32, DEV)
    n0 = ops.afm_calls
    out = ops.afm_pool(x, d["offs"], 16, *ps)
    out.backward(torch.from_numpy(d["g"]).to(DEV))
    assert ops.afm_calls == n0 + 1
    _ratio(out.detach().cpu().numpy(), f["out"], f["e_out"])
    gx = x.grad.cpu().numpy()
    _ratio(gx[:, _field_cols(d["offs"], 16)].reshape(19, 9, 16), ge, e_ge)
    rest = np.ones(gx.shape[1], bool)
    rest[_field_cols(d["offs"], 16)] = False
    assert not gx[:, rest].any()                                               # zero outside the fields
    for p, ref, b in zip(ps, (gW1, gb1, gw2), (eW1, eb1, ew2)):
        _ratio(p.grad.cpu().numpy(), ref, b)
    # a row-strided aligned view is read in place: the same bits, no copy of x
    W = x.shape[1]
    wide = torch.full((19, _round4(W) + 8), float("nan"), device=DEV)
    wide[:, 4:4 + W] = x.detach()
    view = wide[:, 4:4 + W]
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        ov = ops.afm_pool(view, d["offs"], 16, *ps)
    torch.cuda.synchronize()
    assert torch.equal(ov, out.detach()) and torch.cuda.max_memory_allocated() - m0 < x.numel() * 4
    # fallbacks: other dtypes, misaligned fields, unsupported shapes -- afm_calls unchanged, the math form's values
    n1 = ops.afm_calls
    xd, pd = _torch_inputs(d, torch.float64, DEV)
    assert ops.afm_pool(xd, d["offs"], 16, *pd).dtype == torch.float64
    xm = torch.nn.functional.pad(x.detach(), (2, 0))
    om = ops.afm_pool(xm, [o + 2 for o in d["offs"]], 16, *ps)
    assert torch.allclose(om, out.detach(), rtol=1e-4, atol=1e-5)
    big = torch.randn(3, 65 * 4, device=DEV)
    assert ops.afm_pool(big, 65, 4, torch.randn(2, 4, device=DEV), torch.zeros(2, device=DEV), torch.ones(2, device=DEV)).shape == (3, 4)
    assert ops.afm_calls == n1


def test_graph_replay_equals_eager():
    c = dict(F=26, D=16, A=16, B=33, fields="adjacent", pad=0)
    d = R.case_data(c, kind="gauss")
    x, ps = _torch_inputs(d, torch.float32, DEV)
    x, ps = x.detach(), [p.detach() for p in ps]
    g = torch.from_numpy(d["g"]).to(DEV)
    lib = _lib.load()
    F, D, A, B = 26, 16, 16, 33
    off = _off_arr(d["offs"])

    def bufs():
        return dict(out=torch.zeros(B, D, device=DEV), lse=torch.zeros(B, device=DEV), gx=torch.zeros(B, x.shape[1], device=DEV),
                    gw1=torch.zeros(A, D, device=DEV), gb1=torch.zeros(A, device=DEV), gw2=torch.zeros(A, device=DEV),
                    ws=torch.zeros(lib.nrx_afm_bwd_workspace(B, F, D, A) // 4, device=DEV))

    def both(o, st):
        assert lib.nrx_afm_fwd(x.data_ptr(), x.shape[1], off, F, D, ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(), A, B, o["out"].data_ptr(), D,
                               o["lse"].data_ptr(), st) == NRX_OK
        assert lib.nrx_afm_bwd(x.data_ptr(), x.shape[1], off, F, D, ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(), A, B, o["out"].data_ptr(), D,
                               o["lse"].data_ptr(), g.data_ptr(), D, o["gx"].data_ptr(), x.shape[1], o["gw1"].data_ptr(), o["gb1"].data_ptr(),
                               o["gw2"].data_ptr(), o["ws"].data_ptr(), st) == NRX_OK
    eager = bufs()
    both(eager, _stream())
    torch.cuda.synchronize()
    rep = bufs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both(rep, s.cuda_stream)           # (warm-up on the side stream: the LDS attribute is set outside the capture)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        for v in rep.values():
            v.zero_()
        with torch.cuda.graph(graph, stream=s):
            both(rep, s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("out", "lse", "gx", "gw1", "gb1", "gw2"):
        assert torch.equal(eager[k], rep[k]), k


def test_allocator_peak_is_the_named_buffers():
    B, F, D, A = 2048, 26, 16, 16
    torch.manual_seed(0)
    x = torch.randn(B, F * D, device=DEV, requires_grad=True)
    ps = [torch.randn(A, D, device=DEV, requires_grad=True), torch.zeros(A, device=DEV, requires_grad=True), torch.randn(A, device=DEV, requires_grad=True)]
    g = torch.randn(B, D, device=DEV)
    ws = _lib.load().nrx_afm_bwd_workspace(B, F, D, A)
    named = 4 * (B * D + B + B * F * D + A * D + 2 * A) + ws
    assert named + (1 << 20) < 0.5 * 4 * B * (F * (F - 1) // 2) * D
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.afm_pool(x, F, D, *ps)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - m0
    print(f"afm gpu allocator peak {peak} named {named}")
    assert peak <= named + (1 << 20)
