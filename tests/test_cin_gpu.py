"""The Compressed Interaction Network kernels of csrc/nrx_cin.hip alone, through the C ABI (nrx_cin_layer_fwd / _bwd), at the edges of their
launch arithmetic (tests/cin_ref.py lists them: dim dividing the 32-row tile, not dividing it, equal to it, spanning two tiles; one and two column
tiles of H, m and Hp; odd K; K split into LDS slabs; 1 .. 67 samples and a batch that wraps the grid loop; one slice of the weight gradient, one
slice plus a sample, several), layer 1 (xprev == NULL) and above, xk == NULL, g_xk == NULL, g_x0 stored and accumulated, adjacent, permuted and
interleaved fields, p at a column offset of a wider buffer -- against the float64 restatement and the bounds derived there (asserted as derived;
each test prints its worst error / bound, pytest -s shows them).
Every buffer is the head of a larger allocation filled with NaN, gaps between fields included: a read outside an input would poison a result, and
every float that is not a result must hold the very bits it held before the call.
Then: small-integer inputs, where every sum is exact and the result must EQUAL the float64 one; the kernels' bits against an exact emulation of
the header's fma chains; inputs at +-1e3; the same bits run to run, alone or inside a batch, replayed from a graph; ops.cin's autograd against
float64 and its allocator peak."""
import ctypes

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd._lib import NRX_OK
from tests import cin_ref as R

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
    assert (err <= bound).all(), f"worst error / bound {float((err / bound).max()):.3f}"
    return float((err / bound).max()) if err.size else 0.0


def _note(key, r):
    print(f"cin gpu worst error / bound: {key} {r:.4f}")


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


def run_fwd(c, d):
    """(xk [B, H, D] or None, p [B, H]) of a case on its data; every input and every float around the outputs checked for untouched bits."""
    m, H, D, B = c["m"], c["H"], c["D"], d["X0"].shape[0]
    Hp = c["Hp"] or m
    ld = _round4(d["width"])
    xa = Arena(B, ld, data=R.place(d["X0"], d["offs"], d["width"]))
    pa = None if d["Xp"] is None else Arena(B, Hp * D + 4, data=d["Xp"].reshape(B, -1))
    wa = Arena(1, H * Hp * m, off=1, data=d["W"].reshape(1, -1))
    ka = None if c["xk_null"] else Arena(B, H * D + 8)
    p_ld = H + c["p_off"] + 2
    oa = Arena(B, p_ld, off=3)
    _ok(_lib.load().nrx_cin_layer_fwd(xa.ptr, ld, _off_arr(d["offs"]), m, D, None if pa is None else pa.ptr, Hp * D + 4, Hp, wa.ptr, H, B,
                                      None if ka is None else ka.ptr, H * D + 8, oa.ptr + 4 * c["p_off"], p_ld, _stream()), "nrx_cin_layer_fwd")
    p = oa.take(np.arange(c["p_off"], c["p_off"] + H))
    xk = None if ka is None else ka.take(np.arange(H * D)).reshape(B, H, D)
    for a in (xa, pa, wa):
        if a is not None:
            a.take(np.arange(0))
    return xk, p


def run_bwd(c, d):
    """(g_xprev [B, Hp, D] or None, g_x0 [B, m, D], g_W [H, Hp, m])."""
    lib = _lib.load()
    m, H, D, B = c["m"], c["H"], c["D"], d["X0"].shape[0]
    Hp = c["Hp"] or m
    ld = _round4(d["width"])
    xa = Arena(B, ld, data=R.place(d["X0"], d["offs"], d["width"]))
    pa = None if d["Xp"] is None else Arena(B, Hp * D, data=d["Xp"].reshape(B, -1))
    wa = Arena(1, H * Hp * m, data=d["W"].reshape(1, -1))
    gp_ld = H + c["p_off"] + 1
    gpa = Arena(B, gp_ld, off=1)
    gpa.body()[:, c["p_off"]:c["p_off"] + H] = d["g_p"]
    gpa.t = torch.from_numpy(gpa.host).to(DEV)
    gka = None if d["g_xk"] is None else Arena(B, H * D + 4, data=d["g_xk"].reshape(B, -1))
    gxp = None if d["Xp"] is None else Arena(B, Hp * D + 4)
    gx0 = Arena(B, ld + 4, data=None if d["up"] is None else R.place(d["up"], d["offs"], d["width"]))      # (the off-field columns keep their sentinels)
    gw = Arena(1, H * Hp * m, off=1)
    nws = lib.nrx_cin_layer_bwd_workspace(B, m, Hp, H, D)
    sl = lib.nrx_cin_wgrad_slice(D)
    assert nws == -(-B // sl) * H * Hp * m * 4
    wsp = torch.full((nws // 4 + 16,), float("nan"), device=DEV)
    _ok(lib.nrx_cin_layer_bwd(xa.ptr, ld, _off_arr(d["offs"]), m, D, None if pa is None else pa.ptr, Hp * D, Hp, wa.ptr, H, B, gpa.ptr + 4 * c["p_off"],
                              gp_ld, None if gka is None else gka.ptr, H * D + 4, None if gxp is None else gxp.ptr, Hp * D + 4, gx0.ptr, ld + 4,
                              0 if d["up"] is None else 1, gw.ptr, wsp.data_ptr(), _stream()), "nrx_cin_layer_bwd")
    assert torch.isnan(wsp[nws // 4:]).all(), "a float past the workspace was written"
    g_x0 = gx0.take(_field_cols(d["offs"], D)).reshape(B, m, D)
    g_xp = None if gxp is None else gxp.take(np.arange(Hp * D)).reshape(B, Hp, D)
    g_W = gw.take(np.arange(H * Hp * m)).reshape(H, Hp, m)
    for a in (xa, pa, wa, gpa, gka):
        if a is not None:
            a.take(np.arange(0))
    return g_xp, g_x0, g_W


def _refs(c, d):
    Xp = d["X0"] if d["Xp"] is None else d["Xp"]
    sl = _lib.load().nrx_cin_wgrad_slice(c["D"])
    fwd = R.layer_fwd(d["X0"], Xp, d["W"])
    bwd = R.layer_bwd(d["X0"], Xp, d["W"], d["g_p"], d["g_xk"], up=d["up"], layer1=d["Xp"] is None)
    gw = R.layer_gw(d["X0"], Xp, d["g_p"], d["g_xk"], sl)
    return fwd, bwd, gw


def check_case(c, key, scale=1.0, seed=0):
    d = R.case_data(c, seed=seed, scale=scale)
    ((xk_r, p_r), (xk_b, p_b)), ((gxp_r, gx0_r), (gxp_b, gx0_b)), (gw_r, gw_b) = _refs(c, d)
    xk, p = run_fwd(c, d)
    r = dict(p=_ratio(p, p_r, p_b))
    if xk is not None:
        r["xk"] = _ratio(xk, xk_r, xk_b)
    g_xp, g_x0, g_W = run_bwd(c, d)
    r["g_x0"] = _ratio(g_x0, gx0_r, gx0_b)
    if g_xp is not None:
        r["g_xprev"] = _ratio(g_xp, gxp_r, gxp_b)
    r["g_W"] = _ratio(g_W, gw_r, gw_b)
    _note(key, max(r.values()))
    return r


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_launch_shape_edges(c):
    check_case(c, R.case_id(c))


def test_the_grid_loop_wraps():
    check_case(R.WRAP, "wrap")


@pytest.mark.parametrize("D, m, Hp, H", [(16, 3, 2, 3), (12, 2, None, 33)])
def test_weight_gradient_slices(D, m, Hp, H):
    """Batches of exactly one slice of the weight gradient, one slice plus one sample, several slices and a part (the slice size from the library)."""
    sl = _lib.load().nrx_cin_wgrad_slice(D)
    assert sl >= 1
    for B in (sl, sl + 1, 3 * sl + 2):
        check_case(dict(m=m, Hp=Hp, H=H, D=D, B=B, fields="permuted", xk_null=True, gxk_null=False, acc=False, p_off=0), f"slices-D{D}-B{B}")


@pytest.mark.parametrize("m, Hp, H, D", [(26, 32, 32, 16), (33, None, 33, 20), (64, 64, 64, 64), (3, 1, 1, 4)])
def test_inputs_at_1e3(m, Hp, H, D):
    check_case(dict(m=m, Hp=Hp, H=H, D=D, B=3, fields="permuted", xk_null=False, gxk_null=False, acc=True, p_off=1), f"1e3-m{m}-H{H}-D{D}", scale=1e3, seed=3)


@pytest.mark.parametrize("m, Hp, H, D", [(3, None, 5, 4), (5, 7, 33, 12), (26, 32, 40, 16), (33, None, 64, 20), (7, 33, 31, 36), (64, 64, 64, 64)])
def test_small_integers_are_exact(m, Hp, H, D):
    """Every product and every partial sum is a small integer (below 2^24): no rounding anywhere, so the kernels must give the float64 result
    exactly, forward and all three gradients -- a lane or register of the matrix instruction's maps read wrongly cannot hide inside a bound."""
    sl = _lib.load().nrx_cin_wgrad_slice(D)
    for acc, B in ((False, 5), (True, sl + 3 if D <= 36 else 3)):          # (a second slice where the float64 reference stays small)
        c = dict(m=m, Hp=Hp, H=H, D=D, B=B, fields="interleaved", xk_null=False, gxk_null=False, acc=acc, p_off=1)
        d = R.case_data(c, seed=m + D, ints=True)
        ((xk_r, p_r), _), ((gxp_r, gx0_r), _), (gw_r, _) = _refs(c, d)
        xk, p = run_fwd(c, d)
        assert np.array_equal(xk.astype(np.float64), xk_r) and np.array_equal(p.astype(np.float64), p_r)
        g_xp, g_x0, g_W = run_bwd(c, d)
        assert np.array_equal(g_x0.astype(np.float64), gx0_r)
        assert g_xp is None or np.array_equal(g_xp.astype(np.float64), gxp_r)
        assert np.array_equal(g_W.astype(np.float64), gw_r)


@pytest.mark.parametrize("m, Hp, H, D, B", [(3, None, 3, 4, 2), (2, 5, 3, 12, 2), (3, 3, 33, 4, 1), (5, None, 2, 36, 1), (2, 1, 2, 8, -1)])
def test_bits_are_the_headers_fma_chains(m, Hp, H, D, B):
    """include/nrx_embed.h spells every result as fp32 fma chains: the kernels' bits against an exact emulation of them (tests/cin_ref.py): odd and
    even K, one and two column tiles, one and two row tiles, layer 1, and (B = -1: one slice of the weight gradient plus one sample) the partials' sum."""
    sl = _lib.load().nrx_cin_wgrad_slice(D)
    B = sl + 1 if B < 0 else B
    for acc, gxk_null in ((False, False), (True, True)):
        c = dict(m=m, Hp=Hp, H=H, D=D, B=B, fields="permuted", xk_null=False, gxk_null=gxk_null, acc=acc, p_off=0)
        d = R.case_data(c, seed=11)
        Xp = d["X0"] if d["Xp"] is None else d["Xp"]
        xk, p = run_fwd(c, d)
        xk_c, p_c = R.fwd_chain(d["X0"], Xp, d["W"])
        assert np.array_equal(_bits(xk), _bits(xk_c)) and np.array_equal(_bits(p), _bits(p_c))
        g_xp, g_x0, g_W = run_bwd(c, d)
        gxp_c, gx0_c = R.bwd_chain(d["X0"], Xp, d["W"], d["g_p"], d["g_xk"], up=d["up"], layer1=d["Xp"] is None)
        assert np.array_equal(_bits(g_x0), _bits(gx0_c))
        assert g_xp is None or np.array_equal(_bits(g_xp), _bits(gxp_c))
        assert np.array_equal(_bits(g_W), _bits(R.gw_chain(d["X0"], Xp, d["g_p"], d["g_xk"], sl)))


@pytest.mark.parametrize("m, Hp, H, D", [(26, 32, 32, 16), (5, None, 33, 20), (3, 4, 5, 36)])
def test_same_bits_run_to_run_and_alone_or_in_a_batch(m, Hp, H, D):
    c = dict(m=m, Hp=Hp, H=H, D=D, B=67, fields="permuted", xk_null=False, gxk_null=False, acc=True, p_off=0)
    d = R.case_data(c)
    f0, f1 = (run_fwd(c, d) for _ in range(2))
    b0, b1 = (run_bwd(c, d) for _ in range(2))
    for a, b in zip(f0 + b0, f1 + b1):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))          # (g_W included: the same bits run to run)
    for k in (0, 13, 66):
        one = {n: (v[k:k + 1] if n in ("X0", "Xp", "g_p", "g_xk", "up") and v is not None else v) for n, v in d.items()}
        xk, p = run_fwd(c, one)
        assert np.array_equal(_bits(xk), _bits(f0[0][k:k + 1])) and np.array_equal(_bits(p), _bits(f0[1][k:k + 1]))
        g_xp, g_x0, _ = run_bwd(c, one)
        assert np.array_equal(_bits(g_x0), _bits(b0[1][k:k + 1]))
        assert g_xp is None or np.array_equal(_bits(g_xp), _bits(b0[0][k:k + 1]))


# ------------------------------------------------------------------------------------------------- the op
def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _op_data(m, D, sizes, B, kind="adjacent", seed=5, pad=0):
    rng = np.random.default_rng(seed)
    offs, width = R.layout(m, D, kind, seed=1)
    xh = rng.standard_normal((B, _round4(width) + pad)).astype(F32)
    ws, Hp = [], m
    for H in sizes:
        ws.append((rng.standard_normal((H, Hp, m)) / np.sqrt(Hp * m)).astype(F32))
        Hp = H
    return offs, xh, ws


def _f64_grads(xh, offs, D, ws, wz):
    """cin_math in float64 on the CPU and its gradients by autograd: the restatement tests/test_cin_ref.py pins to tests/cin_ref.py."""
    x = torch.from_numpy(xh.astype(np.float64)).requires_grad_(True)
    w = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in ws]
    z = ops.cin_math(x, offs, D, w)
    (z * torch.from_numpy(wz.astype(np.float64))).sum().backward()
    return z.detach().numpy(), x.grad.numpy(), [a.grad.numpy() for a in w]


def _depths(m, D, sizes, B, sl):
    """The most roundings on any path from the inputs to (z, g_x, g_W): the chains of tests/cin_ref.py laid end to end."""
    per, Hp = [], m
    for H in sizes:
        per.append((Hp, H))
        Hp = H
    nz = sum(R.even(Hp * m) + 2 for Hp, _ in per) + D
    nb = sum(max(R.even(H * Hp), R.even(H * m)) + 3 + 2 for Hp, H in per)
    return nz, nz + nb, nz + nb + min(B, sl) * D + 3 + -(-B // sl)


@pytest.mark.parametrize("m, D, sizes, kind", [(26, 16, (32, 32), "adjacent"), (5, 8, (6, 5, 3), "interleaved"), (33, 20, (33, 7), "permuted")])
def test_autograd_against_float64(m, D, sizes, kind):
    """ops.cin at two and three layers: the result and the gradients of x and of every W_k against cin_math in float64.  Bound: z and every
    gradient are polynomials in (x, W, the upstream weights) whose every monomial the kernels form by products and sums that each round once, so the
    computed value is within gamma(n) P(|x|, |W|, |g|) of the exact one, n the most roundings on any path and P the same polynomial on the
    magnitudes (Higham, lemma 3.3) -- which is cin_math and its autograd gradients evaluated at |x|, |W|, |g|.  n comes from the chains' lengths."""
    B = 9
    offs, xh, ws = _op_data(m, D, sizes, B, kind)
    rng = np.random.default_rng(1)
    wz = rng.standard_normal((B, sum(sizes))).astype(F32)
    z_r, gx_r, gw_r = _f64_grads(xh, offs, D, ws, wz)
    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    w = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in ws]
    before = ops.cin_calls
    z = ops.cin(x, offs, D, w)
    assert ops.cin_calls == before + len(sizes)
    (z * torch.from_numpy(wz).to(DEV)).sum().backward()
    z_m, gx_m, gw_m = _f64_grads(np.abs(xh), offs, D, [np.abs(a) for a in ws], np.abs(wz))
    nz, nx, nw = _depths(m, D, sizes, B, _lib.load().nrx_cin_wgrad_slice(D))
    worst = 0.0
    for name, got, ref, mag, n in [("z", z.detach(), z_r, z_m, nz), ("g_x", x.grad, gx_r, gx_m, nx)] + [
            (f"g_W{k}", a.grad, r, mm, nw) for k, (a, r, mm) in enumerate(zip(w, gw_r, gw_m))]:
        got = got.cpu().numpy()
        assert got.shape == ref.shape
        bound = R.gamma(n) * mag + R.TINY * n
        live = bound > R.TINY * n          # (columns outside every field: magnitude 0, gradient 0 -- checked below)
        worst = max(worst, _ratio(got[live], ref[live], bound[live]))
    cols = _field_cols(offs, D)
    rest = x.grad.cpu().numpy().copy()
    rest[:, cols] = 0
    assert not rest.any()          # columns outside every field: gradient 0
    _note(f"autograd-m{m}-D{D}-{sizes}", worst)


def test_views_are_read_in_place_or_copied_with_the_same_bits():
    m, D, sizes, B = 26, 16, (32, 32), 37
    offs, xh, ws = _op_data(m, D, sizes, B)
    W = xh.shape[1]
    x = torch.from_numpy(xh).to(DEV)
    w = [torch.from_numpy(a).to(DEV) for a in ws]
    z = ops.cin(x, offs, D, w)
    big = torch.zeros((B, W + 8), device=DEV)
    big[:, 4:4 + W] = x
    assert ops._rows16(big[:, 4:4 + W], "x").data_ptr() == big.data_ptr() + 16
    assert _same_bits(ops.cin(big[:, 4:4 + W], offs, D, w), z)
    big[:, 1:1 + W] = x
    assert _same_bits(ops.cin(big[:, 1:1 + W], offs, D, w), z)
    assert _same_bits(ops.cin(x[3:4], offs, D, w), z[3:4])


def test_unsupported_shapes_and_cpu_tensors_take_cin_math():
    rng = np.random.default_rng(2)
    # dim 6 is no multiple of 4; 65 feature maps are beyond the kernels
    for m, D, sizes in ((3, 6, (4,)), (3, 8, (65, 2))):
        x = torch.from_numpy(rng.standard_normal((5, m * D)).astype(F32)).to(DEV)
        ws, Hp = [], m
        for H in sizes:
            ws.append(torch.from_numpy(rng.standard_normal((H, Hp, m)).astype(F32)).to(DEV))
            Hp = H
        assert not all(ops.cin_supported(m, a.shape[1], a.shape[0], D) for a in ws)
        before = ops.cin_calls
        assert _same_bits(ops.cin(x, m, D, ws), ops.cin_math(x, m, D, ws)) and ops.cin_calls == before
    x = torch.from_numpy(rng.standard_normal((5, 24)).astype(F32))
    ws = [torch.from_numpy(rng.standard_normal((4, 3, 3)).astype(F32))]
    assert _same_bits(ops.cin(x, 3, 8, ws), ops.cin_math(x, 3, 8, ws))
    lib = _lib.load()
    assert lib.nrx_cin_supported(26, 32, 32, 16) == 1 and lib.nrx_cin_supported(3, 3, 65, 8) == 0 and lib.nrx_cin_supported(3, 3, 4, 6) == 0
    xg, wg, out = x.to(DEV), ws[0].to(DEV), torch.full((5, 65), float("nan"), device=DEV)
    rc = lib.nrx_cin_layer_fwd(xg.data_ptr(), 24, _off_arr([0, 8, 16]), 3, 8, None, 0, 3, wg.data_ptr(), 65, 5, None, 0, out.data_ptr(), 65, _stream())
    torch.cuda.synchronize()
    assert rc == _lib.NRX_ERR_UNSUPPORTED and torch.isnan(out).all()          # nothing enqueued


def test_graph_replay_matches_eager():
    m, D, sizes, B = 33, 12, (33, 5), 19
    offs, xh, ws = _op_data(m, D, sizes, B, "interleaved")
    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    w = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in ws]
    g = torch.randn((B, sum(sizes)), device=DEV)

    def step():
        z = ops.cin(x, offs, D, w)
        return (z,) + torch.autograd.grad(z, [x] + w, g)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = [t.detach().clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.detach().zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want):
        assert _same_bits(a.detach(), b)          # (the weight gradients too: g_W replays to the same bits)


def test_allocator_peak_holds_no_outer_product():
    """Forward + backward at B = 2048, m = 26, D = 16, layers [32, 32] hold the result, the saved X^1, the gradient buffers (g_x, g_X^1, the two
    g_W) and the weight gradient's workspace -- nothing of size B * Hp * m * D (109 MB a layer)."""
    m, D, sizes, B = 26, 16, (32, 32), 2048
    offs, xh, ws = _op_data(m, D, sizes, B)
    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    w = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in ws]
    g = torch.randn((B, sum(sizes)), device=DEV)
    ops.cin(x, offs, D, w).backward(g)          # (warm: library, allocator)
    x.grad = None
    for a in w:
        a.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z = ops.cin(x, offs, D, w)
    z.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    blk = lambda n: (n + (2 << 20) - 1) // (2 << 20) * (2 << 20)          # the caching allocator hands out large blocks in multiples of 2 MiB
    slack = 1 << 20
    lib = _lib.load()
    wsp = max(lib.nrx_cin_layer_bwd_workspace(B, m, Hp, H, D) for Hp, H in ((m, 32), (32, 32)))
    allowed = (blk(4 * B * 64) + blk(4 * B * 32 * D) + blk(4 * B * m * D) + blk(4 * B * 32 * D) + blk(4 * 32 * m * m) + blk(4 * 32 * 32 * m) + blk(wsp)
               + slack)
    assert peak <= allowed, (peak, allowed)
    assert 4 * B * 32 * m * D > 3 * allowed          # ... so a materialised outer product could not have hidden in the rounding and the slack
