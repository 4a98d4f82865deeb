"""The pairwise dot-product interaction kernels of csrc/nrx_dot_interact.hip alone, through the C ABI (nrx_dot_interact_fwd / _bwd), at the edges
of their launch arithmetic (tests/dot_interact_ref.py lists them: one / two tile rows of fields, half-filled tiles, 8- and 16-byte loads and
every count of them, one / two column tiles in the backward, 1 / 2 / 5 / 67 samples and a batch that wraps the sample loop), with adjacent,
permuted, interleaved and padded field layouts, z in a buffer of its own (tight, at an odd column start, with a wider stride) and inside the
buffer its fields live in (the in-place cat form), both flag settings, the backward storing and accumulating -- against the float64 restatement
and the bounds derived there (asserted as derived; each test prints its worst error / bound, pytest -s shows them).
Every buffer is the head of a larger allocation filled with NaN, gaps between fields included: a read outside a field would poison a result, and
every float that is not a result must hold the very bits it held before the call.
Then: small-integer inputs, where every sum is exact and the result must EQUAL the float64 one (the lane and register maps of the matrix
instruction, exactly); the kernels' bits against an exact-rational emulation of the header's fma chains; inputs at +-1e4; the same bits run to run, alone or inside a batch, replayed from a graph, and from both op forms;
autograd through both ops against float64; and the allocator's peak: outputs plus one gradient buffer, no [B, F, F]."""
import ctypes

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd._lib import NRX_DOT_SELF, NRX_OK
from tests import dot_interact_ref as R

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
    print(f"dot_interact gpu worst error / bound: {key} {r:.4f}")


def _off_arr(offs):
    return (ctypes.c_int32 * len(offs))(*offs)


class Arena:
    """[rows, ld] floats starting `off` floats into a NaN-filled device allocation that goes on for more than a row past the last one."""

    def __init__(self, rows, ld, off=0):
        self.rows, self.ld, self.off = rows, ld, off
        self.host = np.full(off + rows * ld + ld + 67, np.nan, F32)

    def body(self, host=None):
        host = self.host if host is None else host
        return host[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)

    def upload(self):
        self.t = torch.from_numpy(self.host).to(DEV)
        return self

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


def _z_arena(kind, B, P, inside=None, width=0):
    """(arena, first column, stride) of the P pair columns: own = tight, odd = an odd column start and an odd stride, wide = stride P + 5,
    cat = columns [width, width + P) of `inside`."""
    if kind == "cat":
        return inside, width, inside.ld
    if kind == "own":
        return Arena(B, max(P, 1)), 0, max(P, 1)
    if kind == "odd":
        return Arena(B, P + 1 + P % 2, off=1), 0, P + 1 + P % 2
    assert kind == "wide"
    return Arena(B, P + 5), 0, P + 5


def _field_cols(offs, D):
    return np.concatenate([np.arange(o, o + D) for o in offs])


def run_fwd(e, offs, width, zkind, self_i):
    B, F, D = e.shape
    P = R.n_pairs(F, self_i)
    ld = _round4(width + P) + 4 if zkind == "cat" else _round4(width)
    xa = Arena(B, ld)
    xa.body()[:, :width] = R.place(e, offs, width)
    za, zcol, z_ld = _z_arena(zkind, B, P, xa, width)
    xa.upload()
    if za is not xa:
        za.upload()
    _ok(_lib.load().nrx_dot_interact_fwd(xa.ptr, ld, _off_arr(offs), F, D, B, NRX_DOT_SELF if self_i else 0, za.ptr + 4 * zcol, z_ld, _stream()),
        "nrx_dot_interact_fwd")
    z = za.take(np.arange(zcol, zcol + P))
    if za is not xa:
        xa.take(np.arange(0))          # x itself: unchanged
    return z


def run_bwd(e, offs, width, zkind, self_i, g_z, up=None):
    """g_e [B, F, D]: stored (up None) or added onto `up`."""
    B, F, D = e.shape
    P = R.n_pairs(F, self_i)
    ld = _round4(width)
    xa = Arena(B, ld)
    xa.body()[:, :width] = R.place(e, offs, width)
    gx_ld = _round4(width + P) + 4 if zkind == "cat" else _round4(width)
    ga = Arena(B, gx_ld)
    if up is not None:
        ga.body()[:, :width] = R.place(up, offs, width)          # (the off-field columns keep their sentinels)
    za, zcol, gz_ld = _z_arena(zkind, B, P, ga, width)
    za.body()[:, zcol:zcol + P] = g_z
    xa.upload()
    ga.upload()
    if za is not ga:
        za.upload()
    _ok(_lib.load().nrx_dot_interact_bwd(xa.ptr, ld, _off_arr(offs), F, D, B, NRX_DOT_SELF if self_i else 0, za.ptr + 4 * zcol, gz_ld, ga.ptr, gx_ld,
                                         0 if up is None else 1, _stream()), "nrx_dot_interact_bwd")
    g = ga.take(_field_cols(offs, D)).reshape(B, F, D)
    xa.take(np.arange(0))
    if za is not ga:
        za.take(np.arange(0))
    return g


def check_case(c, key, scale=1.0, seed=0):
    offs, width, e, g_z, up = R.case_data(c, seed=seed, scale=scale)
    x = R.place(e, offs, width)
    z = run_fwd(e, offs, width, c["z"], c["self_i"])
    ref, bound = R.fwd(x, offs, c["D"], c["self_i"])
    r = [_ratio(z, ref, bound)]
    for u in (None, up):
        g = run_bwd(e, offs, width, c["z"], c["self_i"], g_z, u)
        gref, gb = R.bwd(x, offs, c["D"], g_z, c["self_i"], up=u)
        r.append(_ratio(g, gref, gb))
    _note(key, max(r))
    return r


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_launch_shape_edges(c):
    check_case(c, R.case_id(c))


def test_the_sample_loop_wraps():
    c = dict(F=3, D=4, B=R.WRAP_BATCH, fields="interleaved", z="wide", self_i=False)
    check_case(c, "wrap")
    check_case(dict(c, z="cat", self_i=True), "wrap-cat")


@pytest.mark.parametrize("F, D", [(26, 16), (33, 20), (64, 64), (3, 4)])
def test_inputs_at_1e4(F, D):
    for self_i in (False, True):
        check_case(dict(F=F, D=D, B=5, fields="permuted", z="odd", self_i=self_i), f"1e4-F{F}-D{D}", scale=1e4, seed=3)


@pytest.mark.parametrize("F, D", [(3, 4), (17, 12), (26, 16), (32, 8), (33, 20), (40, 32), (64, 64)])
@pytest.mark.parametrize("self_i", [False, True], ids=["strict", "self"])
def test_small_integers_are_exact(F, D, self_i):
    """Every product and every partial sum is a small integer: no rounding anywhere, so the kernels must give the float64 result exactly -- a lane
    or register of the matrix instruction's maps read wrongly cannot hide inside a bound."""
    rng = np.random.default_rng(F * 100 + D)
    B = 5
    offs, width = R.layout(F, D, "interleaved", seed=F)
    e = rng.integers(-3, 4, (B, F, D)).astype(F32)
    g_z = rng.integers(-3, 4, (B, R.n_pairs(F, self_i))).astype(F32)
    up = rng.integers(-9, 10, (B, F, D)).astype(F32)
    x = R.place(e, offs, width)
    assert np.array_equal(run_fwd(e, offs, width, "cat", self_i).astype(np.float64), R.fwd(x, offs, D, self_i)[0])
    assert np.array_equal(run_bwd(e, offs, width, "own", self_i, g_z).astype(np.float64), R.bwd(x, offs, D, g_z, self_i)[0])
    assert np.array_equal(run_bwd(e, offs, width, "cat", self_i, g_z, up).astype(np.float64), R.bwd(x, offs, D, g_z, self_i, up=up)[0])


@pytest.mark.parametrize("F, D, self_i", [(5, 8, True), (3, 20, False), (17, 4, False), (33, 12, True)])
def test_bits_are_the_headers_fma_chains(F, D, self_i):
    """include/nrx_embed.h spells both results as fp32 fma chains (the forward over k = s, D/2 + s, the backward over ascending j): the kernels'
    bits against an exact-rational emulation of those chains (tests/dot_interact_ref.py), one and two tiles, 8- and 16-byte loads, odd F."""
    c = dict(F=F, D=D, B=2, fields="permuted", z="own", self_i=self_i)
    offs, width, e, g_z, up = R.case_data(c, seed=11)
    x = R.place(e, offs, width)
    assert np.array_equal(_bits(run_fwd(e, offs, width, "own", self_i)), _bits(R.fwd_chain(x, offs, D, self_i)))
    assert np.array_equal(_bits(run_bwd(e, offs, width, "own", self_i, g_z)), _bits(R.bwd_chain(x, offs, D, g_z, self_i)))
    assert np.array_equal(_bits(run_bwd(e, offs, width, "cat", self_i, g_z, up)), _bits(R.bwd_chain(x, offs, D, g_z, self_i, up=up)))


@pytest.mark.parametrize("F, D", [(26, 16), (40, 20)])
def test_same_bits_run_to_run_and_alone_or_in_a_batch(F, D):
    c = dict(F=F, D=D, B=67, fields="permuted", z="own", self_i=False)
    offs, width, e, g_z, up = R.case_data(c)
    z0, z1 = (run_fwd(e, offs, width, "own", False) for _ in range(2))
    g0, g1 = (run_bwd(e, offs, width, "own", False, g_z, up) for _ in range(2))
    assert np.array_equal(_bits(z0), _bits(z1)) and np.array_equal(_bits(g0), _bits(g1))
    for k in (0, 13, 66):
        assert np.array_equal(_bits(run_fwd(e[k:k + 1], offs, width, "wide", False)), _bits(z0[k:k + 1]))
        assert np.array_equal(_bits(run_bwd(e[k:k + 1], offs, width, "cat", False, g_z[k:k + 1], up[k:k + 1])), _bits(g0[k:k + 1]))


# ------------------------------------------------------------------------------------------------- the ops
def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _op_inputs(F=26, D=16, B=37, seed=5, pad=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, F * D + pad)).astype(F32)).to(DEV)
    return x


@pytest.mark.parametrize("self_i", [False, True], ids=["strict", "self"])
def test_both_op_forms_give_the_same_bits(self_i):
    F, D, B = 26, 16, 37
    x = _op_inputs(F, D, B)
    W, P = F * D, R.n_pairs(F, self_i)
    before = ops.dot_interaction_calls
    z = ops.dot_interaction(x, F, D, self_interaction=self_i)
    ld = _round4(W + P)
    buf = torch.full((B, ld), float("nan"), device=DEV)
    buf[:, :W] = x
    out = ops.dot_interaction_cat_(buf, W, F, D, self_interaction=self_i)
    assert ops.dot_interaction_calls == before + 2
    assert out.data_ptr() == buf.data_ptr() and _same_bits(out[:, :W].contiguous(), x) and _same_bits(out[:, W:W + P].contiguous(), z)
    assert torch.isnan(out[:, W + P:]).all()          # the pad columns are never written
    ref, bound = R.fwd(x.cpu().numpy(), [f * D for f in range(F)], D, self_i)
    _note(f"ops-{self_i}", _ratio(z.cpu().numpy(), ref, bound))
    # a row-strided, aligned view is read in place; a misaligned one through a copy: the same bits
    big = torch.zeros((B, W + 8), device=DEV)
    big[:, 4:4 + W] = x
    assert ops._rows16(big[:, 4:4 + W], "x").data_ptr() == big.data_ptr() + 16
    assert _same_bits(ops.dot_interaction(big[:, 4:4 + W], F, D, self_interaction=self_i), z)
    big[:, 1:1 + W] = x
    assert _same_bits(ops.dot_interaction(big[:, 1:1 + W], F, D, self_interaction=self_i), z)


def test_a_width_that_is_no_multiple_of_4_goes_through_a_padded_copy():
    """Fields at 16-byte aligned offsets inside a contiguous x of 50 columns (and a single row of it): no row stride the kernels take, so the
    one copy pads the rows; the same bits as the same fields in a 52-column x, and the gradient has the shape of x."""
    F, D, B, W = 3, 16, 7, 50
    rng = np.random.default_rng(9)
    xh = rng.standard_normal((B, W)).astype(F32)
    g = torch.from_numpy(rng.standard_normal((B, 3)).astype(F32)).to(DEV)
    wide = torch.zeros((B, 52), device=DEV)
    wide[:, :W] = torch.from_numpy(xh).to(DEV)
    wide.requires_grad_(True)
    zw = ops.dot_interaction(wide, F, D)
    zw.backward(g)
    for rows in (slice(0, B), slice(2, 3)):
        x = torch.from_numpy(xh[rows]).to(DEV).requires_grad_(True)
        z = ops.dot_interaction(x, F, D)
        z.backward(g[rows])
        assert _same_bits(z.detach(), zw.detach()[rows].contiguous())
        assert x.grad.shape == x.shape and _same_bits(x.grad, wide.grad[rows, :W].contiguous())
        assert not x.grad[:, 48:].any()


def test_graph_replay_matches_eager():
    F, D, B = 33, 12, 19
    offs = [int(o) for o in R.layout(F, D, "interleaved", seed=2)[0]]
    width = max(offs) + D
    x = torch.randn((B, _round4(width)), device=DEV).requires_grad_(True)
    g = torch.randn((B, R.n_pairs(F)), device=DEV)

    def step():
        z = ops.dot_interaction(x, offs, D)
        return (z,) + torch.autograd.grad(z, (x,), g)

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
        assert _same_bits(a.detach(), b)


@pytest.mark.parametrize("F, D, kind, self_i", [(26, 16, "adjacent", False), (5, 8, "interleaved", True), (40, 20, "permuted", False)])
def test_autograd_through_both_ops_against_float64(F, D, kind, self_i):
    B = 9
    rng = np.random.default_rng(F + D)
    offs, width = R.layout(F, D, kind, seed=1)
    W, P = _round4(width), R.n_pairs(F, self_i)
    xh = rng.standard_normal((B, W)).astype(F32)
    wz = rng.standard_normal((B, P)).astype(F32)
    wx = rng.standard_normal((B, W)).astype(F32)
    gref, gb = R.bwd(xh, offs, D, wz, self_i)
    cols = _field_cols(offs, D)

    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    z = ops.dot_interaction(x, offs, D, self_interaction=self_i)
    (z * torch.from_numpy(wz).to(DEV)).sum().backward()
    got = x.grad.cpu().numpy()
    r = _ratio(got[:, cols].reshape(B, F, D), gref, gb)
    rest = got.copy()
    rest[:, cols] = 0
    assert not rest.any()          # columns outside every field: gradient 0

    ld = _round4(W + P)
    base = torch.zeros((B, ld), device=DEV)
    base[:, :W] = torch.from_numpy(xh).to(DEV)
    base.requires_grad_(True)
    out = ops.dot_interaction_cat_(base * 1.0, W, offs, D, self_interaction=self_i)
    w_all = torch.cat([torch.from_numpy(wx), torch.from_numpy(wz)], dim=1).to(DEV)
    (out[:, :W + P] * w_all).sum().backward()
    got = base.grad.cpu().numpy()
    up = wx[:, cols].reshape(B, F, D)
    gref2, gb2 = R.bwd(xh, offs, D, wz, self_i, up=up)
    r = max(r, _ratio(got[:, cols].reshape(B, F, D), gref2, gb2))
    rest = got[:, :W].copy()
    assert np.array_equal(np.delete(rest, cols, axis=1), np.delete(wx, cols, axis=1))          # foreign concat columns: the upstream gradient, untouched
    assert not got[:, W:].any()                                                                  # the pair and pad columns were never read
    _note(f"autograd-F{F}-D{D}", r)


def test_allocator_peak_is_outputs_plus_one_gradient_buffer():
    """Forward + backward hold z, g_x and the one upstream gradient: nothing of size B * F * F (4 B F F bytes = 2 x the bytes of z here)."""
    F, D, B = 26, 16, 8192
    P, W = R.n_pairs(F), F * D
    x = torch.randn((B, W), device=DEV).requires_grad_(True)
    g = torch.randn((B, P), device=DEV)
    ops.dot_interaction(x, F, D).backward(g)          # (warm: library, allocator)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z = ops.dot_interaction(x, F, D)
    z.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    blk = lambda n: (n + (2 << 20) - 1) // (2 << 20) * (2 << 20)          # the caching allocator hands out large blocks in multiples of 2 MiB
    slack = 1 << 20
    assert peak <= blk(4 * B * P) + blk(4 * B * W) + slack, (peak, 4 * B * P, 4 * B * W)
    assert 4 * B * F * F > 8 * slack          # ... so a [B, F, F] intermediate could not have hidden in the rounding and the slack
    # the in-place form: the buffer exists already; the backward holds the upstream gradient (given) and the one it returns
    ld = _round4(W + P)
    base_t = torch.randn((B, ld), device=DEV).requires_grad_(True)
    gg = torch.randn((B, ld), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    buf = base_t * 1.0
    out = ops.dot_interaction_cat_(buf, W, F, D)
    out.backward(gg)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    # buf, the returned gradient, base_t.grad (MulBackward's product)
    assert peak <= 3 * blk(4 * B * ld) + slack, (peak, 4 * B * ld)
