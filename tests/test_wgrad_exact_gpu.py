"""The batch-split weight-gradient kernels of csrc/nrx_dcn2_bwd.hip at their launch-shape edges, through the C entry points themselves:
nrx_linear_wgrad (float atomics), nrx_linear_wgrad_ordered and nrx_dcn_v2_layer_bwd over the case lists of tests/wgrad_cases.py.

The operands are small integers, so every summation order -- atomics, ordered slices, the fp32 and the bf16x3 MFMA chains -- must give the int64
reference WORD FOR WORD; one dropped or doubled batch row at a slice boundary changes a word (tests/test_wgrad_cases.py shows it on the CPU).
Operands sit inside wider NaN-filled allocations, outputs start as NaN between guard words, the workspace is exactly the advertised size with
guard bytes behind it.  One randn companion per (tile, path, mode) checks rounding against float64 with a bound that holds for any order.

Run as a script (`python tests/test_wgrad_exact_gpu.py`) it sends both full case lists through the same check functions and exits non-zero on the
first mismatch: the tests of the switches that the library reads once per process start it as a child with the variable set."""
import collections
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib
from tests import wgrad_cases as wc

DEV = "cuda:0"
LINEAR = wc.linear_cases()
DCN2 = wc.dcn2_cases()
NAN = float("nan")
GUARD = 64                       # guard words on either side of an output (256 bytes: the output itself stays 256-byte aligned)
GUARD_WORD = 0x7FC5A5A5          # a NaN with a payload no kernel produces
WS_GUARD = 256                   # guard bytes behind (and, with an offset, in front of) a workspace
WS_GUARD_BYTE = 0xA5
# wc.wgrad_shape restates the library's launch shape at its defaults; with a switch or a tuning variable set (the children below) the library's
# own workspace functions are still the size that is allocated exactly, only the comparison with the restatement is off
DEFAULT_SHAPE = os.environ.get("NRX_WGRAD_XCD", "1") == "1" and not any(os.environ.get(v) for v in ("NRX_WGRAD_TILE", "NRX_WGRAD_BLOCKS", "NRX_WGRAD_MIN_ROWS"))


def _lib_splits(lib, batch, M, N):
    """The slice count the library uses, from its workspace function (= splits * (M N + M) * 4 + 512)."""
    q, r = divmod(lib.nrx_linear_wgrad_ordered_workspace(batch, M, N) - 512, (M * N + M) * 4)
    assert r == 0 and q >= 1
    return q


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _place(arr, ld, off, tail=16):
    """arr [rows, w] inside a NaN-filled allocation: `off` floats in front, rows of `ld` floats, `tail` floats behind.  -> (allocation, base pointer)"""
    rows, w = arr.shape
    buf = torch.full((off + rows * ld + tail,), NAN, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    if rows:
        buf[off:off + rows * ld].view(rows, ld)[:, :w] = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)
    return buf, buf.data_ptr() + 4 * off


def _inner(buf, ld, off, rows, w):
    return buf[off:off + rows * ld].view(rows, ld)[:, :w]


def _guarded(*sizes):
    """NaN-filled outputs of `sizes` floats, one behind the other, between guard words.  -> (allocation, [views])"""
    n = sum(sizes)
    buf = torch.full((GUARD + n + GUARD,), GUARD_WORD, dtype=torch.int32, device=DEV)
    body = buf[GUARD:GUARD + n].view(torch.float32)
    body.fill_(NAN)
    views, at = [], 0
    for s in sizes:
        views.append(body[at:at + s])
        at += s
    return buf, views


def _guards_intact(buf):
    return bool((buf[:GUARD] == GUARD_WORD).all()) and bool((buf[-GUARD:] == GUARD_WORD).all())


def _workspace(nbytes, off):
    """A workspace of exactly `nbytes` (0xFF inside: NaN), `off` bytes into its allocation, guard bytes around it.  -> (allocation, pointer)"""
    buf = torch.full((off + nbytes + WS_GUARD,), WS_GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[off:off + nbytes] = 0xFF
    return buf, buf.data_ptr() + off


def _ws_guards_intact(buf, nbytes, off):
    return bool((buf[:off] == WS_GUARD_BYTE).all()) and bool((buf[off + nbytes:] == WS_GUARD_BYTE).all())


def _same_words(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_exact(got, want_i64, what, name):
    """got (float32, device) equals the int64 reference word for word."""
    want = torch.from_numpy(want_i64.astype(np.float32)).to(DEV).reshape(got.shape)
    if _same_words(got, want):
        return
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    first = tuple(bad[0].tolist())
    raise AssertionError(f"{name}: {what} differs from the int64 reference in {bad.shape[0]} of {got.numel()} words; first at {first}: "
                         f"got {got[first].item()!r}, want {want[first].item()!r}")


def _call_linear(lib, case, gptr, aptr, gW, gb, wsptr):
    gbp = gb.data_ptr() if gb is not None else None
    if case.mode == "ordered":
        return lib.nrx_linear_wgrad_ordered(gptr, case.g_ld, aptr, case.a_ld, case.batch, case.M, case.N, gW.data_ptr(), gbp, wsptr, _stream())
    return lib.nrx_linear_wgrad(gptr, case.g_ld, aptr, case.a_ld, case.batch, case.M, case.N, gW.data_ptr(), gbp, _stream())


def run_linear(lib, case, g, a):
    """One call of the case's entry point on operands g [batch, M], a [batch, N] (numpy float32) laid out as the case says.  Checks the return code,
    guards, operand allocations and, in ordered mode, that a second call gives the same words.  -> (g_W [M, N], g_b [M] or None) on the device."""
    gbuf, gptr = _place(g, case.g_ld, case.g_off)
    abuf, aptr = _place(a, case.a_ld, case.a_off)
    g0, a0 = gbuf.clone(), abuf.clone()
    obuf, (gW, gb) = _guarded(case.M * case.N, case.M)
    if not case.bias:
        gb = None
    wsz, ws_off, wsbuf, wsptr = 0, 64 * (case.index % 2), None, None
    if case.mode == "ordered":
        wsz = lib.nrx_linear_wgrad_ordered_workspace(case.batch, case.M, case.N)
        assert not DEFAULT_SHAPE or wsz == wc.linear_workspace_bytes(case.batch, case.M, case.N), case.name
        wsbuf, wsptr = _workspace(wsz, ws_off)
    rc = _call_linear(lib, case, gptr, aptr, gW, gb, wsptr)
    torch.cuda.synchronize()
    assert rc == 0, (case.name, rc, lib.nrx_last_error())
    assert _guards_intact(obuf), f"{case.name}: guard words around g_W / g_b overwritten"
    if not case.bias:
        assert bool(torch.isnan(obuf[GUARD + case.M * case.N:GUARD + case.M * case.N + case.M].view(torch.float32)).all()), f"{case.name}: wrote past g_W"
    assert _same_words(gbuf, g0) and _same_words(abuf, a0), f"{case.name}: an operand allocation (values or NaN padding) was written"
    gW1, gb1 = gW.clone(), gb.clone() if gb is not None else None
    if case.mode == "ordered":
        assert _ws_guards_intact(wsbuf, wsz, ws_off), f"{case.name}: wrote outside the {wsz}-byte workspace"
        gW.fill_(NAN)
        if gb is not None:
            gb.fill_(NAN)
        rc = _call_linear(lib, case, gptr, aptr, gW, gb, wsptr)
        torch.cuda.synchronize()
        assert rc == 0, (case.name, rc, lib.nrx_last_error())
        assert _same_words(gW, gW1) and (gb is None or _same_words(gb, gb1)), f"{case.name}: the ordered mode gave other words on a second call"
        assert _guards_intact(obuf) and _ws_guards_intact(wsbuf, wsz, ws_off), case.name
    return gW1.view(case.M, case.N), gb1


def check_linear(lib, case):
    ops = wc.int_operands(case, wc.case_rng(case))
    ref = wc.exact_reference(case, ops)
    gW, gb = run_linear(lib, case, ops["g"], ops["a"])
    _assert_exact(gW, ref["g_W"], "g_W", case.name)
    if case.bias:
        _assert_exact(gb, ref["g_b"], "g_b", case.name)


def check_dcn2(lib, case):
    """One nrx_dcn_v2_layer_bwd call: g_xl, g_x0, g_W, g_b word for word the int64 reference; pad columns, guards and inputs untouched."""
    B, D, name = case.batch, case.dim, case.name
    ops = wc.int_operands(case, wc.case_rng(case))
    ref = wc.exact_reference(case, ops)
    relu = case.flags & 1
    bufs = {k: _place(ops[k], case.ld, 0) for k in ("x0", "xl", "lin")}
    bufs["g"] = _place(ops["g"], case.g_ld, 0)
    bufs["W"] = _place(ops["W"], D, 0, tail=0)
    out_ptr = None                                    # without ReLU `out` is not read: NaN, or no pointer at all
    if relu or case.index % 2 == 0:
        bufs["out"] = _place(ops["out"] if relu else np.full((B, D), np.nan, np.float32), case.ld, 0)
        out_ptr = bufs["out"][1]
    before = {k: v[0].clone() for k, v in bufs.items()}
    # g_x0: its old value where it is accumulated (bit 0), NaN where it is overwritten; g_xl: NaN
    gx0buf, gx0ptr = _place(ops["gx0"] if case.acc & 1 else np.full((B, D), np.nan, np.float32), case.ld, 0)
    gxlbuf, gxlptr = _place(np.full((B, D), np.nan, np.float32), case.gxl_ld, 0)
    if case.index % 4 < 2:                            # g_b right behind g_W (what the Python layer allocates: one fill launch) or apart
        obufs, (gW, gb) = _guarded(D * D, D)
        obufs = [obufs]
    else:
        (o1, (gW,)), (o2, (gb,)) = _guarded(D * D), _guarded(D)
        obufs = [o1, o2]
    wsz, ws_off = lib.nrx_dcn_v2_layer_bwd_workspace(B, D), 64 * (case.index % 2)
    assert not DEFAULT_SHAPE or wsz == wc.dcn2_workspace_bytes(B, D), name
    wsbuf, wsptr = _workspace(wsz, ws_off)
    rc = lib.nrx_dcn_v2_layer_bwd(bufs["x0"][1], bufs["xl"][1], case.ld, bufs["lin"][1], out_ptr, case.flags, B, D, bufs["W"][1], bufs["g"][1], case.g_ld,
                                  gxlptr, case.gxl_ld, gx0ptr, case.ld, case.acc, gW.data_ptr(), gb.data_ptr(), wsptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, lib.nrx_last_error())
    assert all(_guards_intact(o) for o in obufs), f"{name}: guard words around g_W / g_b overwritten"
    assert _ws_guards_intact(wsbuf, wsz, ws_off), f"{name}: wrote outside the {wsz}-byte workspace"
    for k, (buf, _) in bufs.items():
        assert _same_words(buf, before[k]), f"{name}: the allocation of input {k} was written"
    for what, buf, ld in (("g_xl", gxlbuf, case.gxl_ld), ("g_x0", gx0buf, case.ld)):
        _assert_exact(_inner(buf, ld, 0, B, D), ref[what], what, name)
        assert bool(torch.isnan(buf[B * ld:]).all()), f"{name}: wrote behind the last row of {what}"
        if ld > D:
            assert bool(torch.isnan(buf[:B * ld].view(B, ld)[:, D:]).all()), f"{name}: pad columns of {what} written"
    _assert_exact(gW.view(D, D), ref["g_W"], "g_W", name)
    _assert_exact(gb, ref["g_b"], "g_b", name)


# ---- the integer cases --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", LINEAR, ids=lambda c: c.name)
def test_linear_wgrad_equals_int64_reference_word_for_word(case):
    check_linear(_lib.load(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DCN2, ids=lambda c: c.name)
def test_dcn_v2_layer_bwd_equals_int64_reference_word_for_word(case):
    check_dcn2(_lib.load(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", wc.MODES)
@pytest.mark.parametrize("bias", [True, False])
def test_linear_wgrad_of_an_empty_batch_is_zero(mode, bias):
    lib = _lib.load()
    case = wc.LinearCase(0, 12, 8, 0, 16, 12, 0, 4, bias, mode)
    gW, gb = run_linear(lib, case, np.zeros((0, 12), np.float32), np.zeros((0, 8), np.float32))
    assert _same_words(gW, torch.zeros_like(gW)) and (gb is None or _same_words(gb, torch.zeros_like(gb)))


# ---- rounding: one randn companion per (tile, path, mode) ---------------------------------------------------------------------------------------------
def _companions():
    picked = {}
    for c in LINEAR:
        k = (c.key["tile"], c.path, c.mode)
        if c.bias and (k not in picked or (picked[k].key["slices"] < 2 <= c.key["slices"])):
            picked[k] = c
    return [picked[k] for k in sorted(picked)]


def any_order_bound(batch, splits, abs_products):
    """|fl(sum) - sum| of `batch` fp32 products summed in ANY order, with `splits` partial sums combined on top: each product is rounded once and takes
    part in fewer than batch + splits additions, each with relative error 2^-24 -- elementwise (batch + splits + 2) 2^-24 sum_b |g[b, i] a[b, j]|.
    Derived, not measured, and loose on purpose: the integer cases are the sharp check."""
    return (batch + splits + 2) * 2.0 ** -24 * abs_products


@pytest.mark.gpu
@pytest.mark.parametrize("case", _companions(), ids=lambda c: c.name)
def test_linear_wgrad_randn_within_the_any_order_bound_of_float64(case):
    assert len(_companions()) == 2 * len(wc.PATHS) * len(wc.MODES)
    rng = np.random.default_rng([wc.SEED, 2, case.index])
    g, a = rng.standard_normal((case.batch, case.M)).astype(np.float32), rng.standard_normal((case.batch, case.N)).astype(np.float32)
    gW, gb = run_linear(_lib.load(), case, g, a)
    g64, a64 = g.astype(np.float64), a.astype(np.float64)
    splits = _lib_splits(_lib.load(), case.batch, case.M, case.N)
    err_W = np.abs(gW.cpu().numpy().astype(np.float64) - g64.T @ a64)
    bound_W = any_order_bound(case.batch, splits, np.abs(g64).T @ np.abs(a64))
    err_b = np.abs(gb.cpu().numpy().astype(np.float64) - g64.sum(0))
    bound_b = any_order_bound(case.batch, splits, np.abs(g64).sum(0))
    print(f"{case.name}: g_W max err / bound {np.max(err_W / bound_W):.3g}, g_b {np.max(err_b / bound_b):.3g}")
    assert (err_W <= bound_W).all() and (err_b <= bound_b).all()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_name_the_function_and_leave_the_outputs_alone():
    lib = _lib.load()
    M, N, B, D = 8, 12, 40, 8
    rng = np.random.default_rng(wc.SEED)
    st = _stream()
    (gbuf, g), (abuf, a) = _place(rng.standard_normal((B, M)).astype(np.float32), M, 0), _place(rng.standard_normal((B, N)).astype(np.float32), N, 0)
    obuf, (gW, gb) = _guarded(M * N, M)
    wsbuf, ws = _workspace(lib.nrx_linear_wgrad_ordered_workspace(B, M, N), 0)
    o0, w0 = obuf.clone(), wsbuf.clone()
    W, b = gW.data_ptr(), gb.data_ptr()
    calls = [
        ("nrx_linear_wgrad", lambda: lib.nrx_linear_wgrad(g, M - 1, a, N, B, M, N, W, b, st)),                    # leading dimension below the width
        ("nrx_linear_wgrad", lambda: lib.nrx_linear_wgrad(g, M, a, N - 1, B, M, N, W, b, st)),
        ("nrx_linear_wgrad", lambda: lib.nrx_linear_wgrad(g, M, a, N, B, M, N, None, b, st)),                     # no g_W
        ("nrx_linear_wgrad", lambda: lib.nrx_linear_wgrad(g, M, a, N, -1, M, N, W, b, st)),                       # negative batch
        ("nrx_linear_wgrad_ordered", lambda: lib.nrx_linear_wgrad_ordered(g, M - 1, a, N, B, M, N, W, b, ws, st)),
        ("nrx_linear_wgrad_ordered", lambda: lib.nrx_linear_wgrad_ordered(g, M, a, N - 1, B, M, N, W, b, ws, st)),
        ("nrx_linear_wgrad_ordered", lambda: lib.nrx_linear_wgrad_ordered(g, M, a, N, B, M, N, None, b, ws, st)),
        ("nrx_linear_wgrad_ordered", lambda: lib.nrx_linear_wgrad_ordered(g, M, a, N, -1, M, N, W, b, ws, st)),
        ("nrx_linear_wgrad_ordered", lambda: lib.nrx_linear_wgrad_ordered(g, M, a, N, B, M, N, W, b, None, st)),   # the ordered entry without a workspace
    ]
    for fn, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc != 0 and (fn + ":").encode() in lib.nrx_last_error(), (fn, rc, lib.nrx_last_error())
        assert _same_words(obuf, o0) and torch.equal(wsbuf, w0), fn
    # the DCN-v2 layer
    t = {k: _place(rng.standard_normal((B, D)).astype(np.float32), D, 0) for k in ("x0", "xl", "lin", "out", "g")}
    Wm = _place(rng.standard_normal((D, D)).astype(np.float32), D, 0)[0]
    gxl, gx0 = torch.full((B * D,), NAN, device=DEV), torch.full((B * D,), NAN, device=DEV)
    obuf, (gW, gb) = _guarded(D * D, D)
    wsbuf, ws = _workspace(lib.nrx_dcn_v2_layer_bwd_workspace(B, D), 0)
    o0, w0, g0 = obuf.clone(), wsbuf.clone(), t["g"][0].clone()

    def layer(ld=D, batch=B, gW_ptr=gW.data_ptr(), gxl_ptr=gxl.data_ptr(), g_ld=D, ws_ptr=ws):
        return lib.nrx_dcn_v2_layer_bwd(t["x0"][1], t["xl"][1], ld, t["lin"][1], t["out"][1], 1, batch, D, Wm.data_ptr(), t["g"][1], g_ld,
                                        gxl_ptr, D, gx0.data_ptr(), D, 0, gW_ptr, gb.data_ptr(), ws_ptr, st)
    for kw in (dict(ld=D - 1), dict(g_ld=D - 1), dict(gW_ptr=None), dict(batch=-1), dict(ws_ptr=None), dict(gxl_ptr=t["g"][1])):      # last: g_xl == g_out
        rc = layer(**kw)
        torch.cuda.synchronize()
        assert rc != 0 and b"nrx_dcn_v2_layer_bwd:" in lib.nrx_last_error(), (kw, rc, lib.nrx_last_error())
        assert _same_words(obuf, o0) and torch.equal(wsbuf, w0) and _same_words(t["g"][0], g0), kw
        assert bool(torch.isnan(gxl).all()) and bool(torch.isnan(gx0).all()), kw


# ---- the atomic entry at the Python level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("batch,in_f,out_f", [(257, 416, 128), (777, 37, 19)])
def test_ops_linear_atomic_mode_takes_the_atomic_entry_and_matches_float64(batch, in_f, out_f, bias, monkeypatch):
    from news_recsys_amd import ops
    lib = _lib.load()
    taken = collections.Counter()

    def spy(name):
        real = getattr(lib, name)

        def wrapped(*args):
            taken[name] += 1
            return real(*args)
        monkeypatch.setattr(lib, name, wrapped)
    spy("nrx_linear_wgrad")
    spy("nrx_linear_wgrad_ordered")
    monkeypatch.setattr(ops, "WGRAD_ATOMIC", True)
    monkeypatch.setattr(ops, "WGRAD_ORDERED", False)
    gen = torch.Generator(device=DEV).manual_seed(batch + in_f + out_f)
    a = torch.randn(batch, in_f, device=DEV, generator=gen)
    W = (torch.randn(out_f, in_f, device=DEV, generator=gen) / in_f ** 0.5).requires_grad_()
    b = torch.randn(out_f, device=DEV, generator=gen, requires_grad=True) if bias else None
    up = torch.randn(batch, out_f, device=DEV, generator=gen)
    ops.linear(a, W, b).backward(up)
    torch.cuda.synchronize()
    assert taken == {"nrx_linear_wgrad": 1}
    splits = _lib_splits(lib, batch, out_f, in_f)
    up64, a64 = up.double(), a.double()
    assert bool(((W.grad.double() - up64.t() @ a64).abs() <= any_order_bound(batch, splits, up64.abs().t() @ a64.abs())).all())
    if bias:
        assert bool(((b.grad.double() - up64.sum(0)).abs() <= any_order_bound(batch, splits, up64.abs().sum(0))).all())


# ---- the switches the library reads once per process ------------------------------------------------------------------------------------------------------
def run_all():
    """Both full case lists through the check functions above; the first mismatch raises."""
    from tests import _poison
    lib = _lib.load()
    done = collections.Counter()
    for i, case in enumerate(LINEAR):
        if i % 16 == 0:
            _poison.poison()
        check_linear(lib, case)
        done["nrx_linear_wgrad" + ("_ordered" if case.mode == "ordered" else "")] += 1
    for i, case in enumerate(DCN2):
        if i % 16 == 0:
            _poison.poison()
        check_dcn2(lib, case)
        done["nrx_dcn_v2_layer_bwd"] += 1
    assert sum(done.values()) == len(LINEAR) + len(DCN2)
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["NRX_DCN2_PANEL", "NRX_DCN2_NARROW_ORDERED", "NRX_WGRAD_XCD"])
def test_every_case_with_a_once_per_process_switch_off(switch):
    """NRX_DCN2_PANEL=0: narrow layers take the three launches; NRX_DCN2_NARROW_ORDERED=0: they take float atomics (and the split form) unless bit 2
    asks; NRX_WGRAD_XCD=0: the fp32 wgrad's tile-fastest block order and the unbalanced slice count.  One fresh child per switch runs every case."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child with {switch}=0 ended with status {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-8000:]}"
    assert f"all {len(LINEAR) + len(DCN2)} cases equal" in r.stdout, r.stdout[-4000:]


if __name__ == "__main__":
    counts = run_all()
    print(f"all {sum(counts.values())} cases equal the int64 reference word for word: {dict(counts)}")
