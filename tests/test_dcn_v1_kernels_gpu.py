"""The DCN-v1 kernels of csrc/nrx_interact.hip alone, through the C ABI (nrx_dcn_v1_fwd, nrx_dcn_v1_bwd, nrx_dcn_v1_bwd_ordered, nrx_embed_dcn_v1_fwd),
at the edges of their launch arithmetic, against tests/dcn_v1_ref.py (held to oracle/ref_np.py, the goldens and float64 autograd by
tests/test_dcn_v1_ref.py, which also asserts that the case lists reach every launch form):
  * integer inputs under the exactness condition: every output equal to the int64 definition bit for bit -- every body of the backward with and
    without a separate x0, float atomics and the block-order sum, blocks of 1 / rpb - 1 / rpb / rpb + 1 / 3 rpb + 5 rows, three trips of each
    pipelined row loop, padded and unaligned leading dimensions (the scalar forms with up to 32 chunks per lane), the cat form, the largest stacks;
  * real-valued inputs: every output inside the bound derived in dcn_v1_ref.bounds, and a row's out / g_x / g_x0 the same bits wherever it sits;
  * refusals that return their code, set nrx_last_error and write nothing;
  * the fused gather + cross: all 28 grouped instantiations and the general kernel at each R / S, a second tile of the persistent blocks.
Every operand is the head of a NaN-filled allocation (Buf of the FM / pooling file): a read past an input would poison a result, and every
float that is not a result must still be NaN after the call.

Each test prints its worst error / bound (pytest -s shows them); those figures are for the record, the asserts are the bounds themselves."""

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib
from news_recsys_amd._lib import NRX_ERR_BAD_ARG, NRX_ERR_UNSUPPORTED, NRX_OK, NRX_SPARSE, NrxFeature
from tests import dcn_v1_ref as P
from tests.test_fm_pool_kernels_gpu import Buf, _ok, _ratio, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
OPERANDS = ("x", "x0", "out", "g", "g_x", "g_x0")


def _note(key, r):
    print(f"dcn_v1 gpu worst error / bound: {key} {r:.4f}")


def _buf(rows, D, lay=None, data=None):
    """The one place a [rows, D] operand gets its allocation: sized from (rows, ld, off) by Buf, ld = D + pad."""
    pad, off = lay or (0, 0)
    ld = D + pad
    assert rows >= 1 and D >= 1 and ld >= D and off >= 0
    return Buf(rows, D, ld, off, None if data is None else np.asarray(data, F32))


_WS = {}


def _workspace(D, NL):
    n = int(_lib.load().nrx_dcn_v1_bwd_ordered_workspace(D, NL))
    assert n > 0
    if n not in _WS:
        _WS.clear()
        _WS[n] = torch.empty(n, dtype=torch.uint8, device=DEV)
    return _WS[n]


def _nan_everywhere(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert np.isnan(b.t.cpu().numpy()).all()


def fwd(i, sep, lay=None, expect=NRX_OK, dims=None, null=()):
    """nrx_dcn_v1_fwd on inputs i; lay: operand -> (pad, off).  dims = (B, D, NL) declared to the library when they are not the arrays' own
    (refusals: the buffers are still sized for what is declared)."""
    lay = lay or {}
    B, D, NL = dims or (i["x"].shape[0], i["x"].shape[1], i["w"].shape[0])
    rows = max(B, 1)
    xb = _buf(rows, D, lay.get("x"), i["x"][:rows] if dims is None else None)
    x0b = _buf(rows, D, lay.get("x0"), i["x0"][:rows] if dims is None else None) if sep else None
    ob = _buf(rows, D, lay.get("out"))
    wb, bb = _buf(max(NL, 1), D, data=i["w"] if NL and dims is None else None), _buf(max(NL, 1), D, data=i["b"] if NL and dims is None else None)
    rc = _lib.load().nrx_dcn_v1_fwd(xb.ptr, xb.ld, x0b.ptr if sep else None, x0b.ld if sep else 0, B, D, NL, None if "w" in null else wb.ptr,
                                    None if "b" in null else bb.ptr, ob.ptr, ob.ld, _stream())
    if expect != NRX_OK or B == 0:
        assert rc == expect, (rc, _lib.load().nrx_last_error())
        assert expect == NRX_OK or b"nrx_dcn_v1_fwd" in _lib.load().nrx_last_error()
        _nan_everywhere(ob)
        return None
    _ok(rc, "nrx_dcn_v1_fwd")
    return ob.read()


def bwd(i, sep, ordered, lay=None, expect=NRX_OK, dims=None, null=(), x_at=None):
    """nrx_dcn_v1_bwd (g_w / g_b zero-filled: it adds into them) or nrx_dcn_v1_bwd_ordered (NaN-filled: it overwrites them).  x_at = (ptr, ld):
    read x from another buffer (the cat form)."""
    lay = lay or {}
    B, D, NL = dims or (i["x"].shape[0], i["x"].shape[1], i["w"].shape[0])
    rows = max(B, 1)
    own = dims is None
    xb = _buf(rows, D, lay.get("x"), i["x"][:rows] if own else None)
    x0b = _buf(rows, D, lay.get("x0"), i["x0"][:rows] if own else None) if sep or "g_x0" in null else None
    gb = _buf(rows, D, lay.get("g"), i["g"][:rows] if own else None)
    gx = _buf(rows, D, lay.get("g_x"))
    gx0 = _buf(rows, D, lay.get("g_x0")) if sep or "x0" in null else None
    wb, bb = _buf(max(NL, 1), D, data=i["w"] if NL and own else None), _buf(max(NL, 1), D, data=i["b"] if NL and own else None)
    fill = np.zeros((NL, D), F32) if NL and not ordered and expect == NRX_OK and B > 0 else None
    gw, gbias = _buf(max(NL, 1), D, data=fill), _buf(max(NL, 1), D, data=fill)
    xp, xld = x_at or (xb.ptr, xb.ld)
    args = [xp, xld, x0b.ptr if x0b is not None and "x0" not in null else None, x0b.ld if x0b is not None else 0, B, D, NL,
            None if "w" in null else wb.ptr, bb.ptr, gb.ptr, gb.ld, gx.ptr, gx.ld, gx0.ptr if gx0 is not None and "g_x0" not in null else None,
            gx0.ld if gx0 is not None else 0, None if "g_w" in null else gw.ptr, gbias.ptr]
    lib = _lib.load()
    if ordered:
        rc = lib.nrx_dcn_v1_bwd_ordered(*args, None if "ws" in null else _workspace(D, min(NL, P.MAX_LAYERS)).data_ptr(), _stream())
    else:
        rc = lib.nrx_dcn_v1_bwd(*args, _stream())
    if expect != NRX_OK or B == 0:
        assert rc == expect, (rc, lib.nrx_last_error())
        assert expect == NRX_OK or b"nrx_dcn_v1_bwd" in lib.nrx_last_error()
        _nan_everywhere(gx, *([gx0] if gx0 is not None else []))
        if not (ordered and B == 0 and NL and expect == NRX_OK):
            _nan_everywhere(gw, gbias)
        else:                                   # the ordered mode overwrites g_w / g_b: an empty batch's gradient is 0
            assert not gw.read().any() and not gbias.read().any()
        return None
    _ok(rc, "nrx_dcn_v1_bwd")
    res = dict(g_x=gx.read(), g_x0=gx0.read() if sep else None)
    if NL:
        res.update(g_w=gw.read(), g_b=gbias.read())
    else:
        _nan_everywhere(gw, gbias)
        res.update(g_w=np.zeros((0, D), F32), g_b=np.zeros((0, D), F32))
    return res


def _exact(got, want, tag):
    for key, v in got.items():
        if v is not None:
            assert P.same_bits(v, np.asarray(want[key], np.float64).astype(F32)), (key,) + tuple(tag)


def _check_int(D, NL, B, density, sep, lay=None, modes=(False, True), forward=True):
    i = P.int_inputs(D, NL, B, density)
    want = P.dcn(i["x"], i["w"], i["b"], i["g"], i["x0"] if sep else None)
    if forward:
        _exact(dict(out=fwd(i, sep, lay)), want, (D, NL, B, sep, lay))
    for ordered in modes:
        if ordered and not P.ordered_takes(D, NL):
            bwd(i, sep, True, lay, expect=NRX_ERR_UNSUPPORTED)
        else:
            _exact(bwd(i, sep, ordered, lay), want, (D, NL, B, sep, ordered, lay))


def _ids(cases):
    return [f"D{c[0]}-L{c[1]}-{'v' if c[2] else 's'}" for c in cases]


# ------------------------------------------------------------------------------------------------- a. integer-exact, every launch form
@pytest.mark.parametrize("D,NL,vec,density", P.INT_CASES, ids=_ids(P.INT_CASES))
def test_forward_and_backward_bit_for_bit_at_the_block_edges(D, NL, vec, density):
    """vec: everything aligned.  Scalar cases are odd widths, so they need no help to leave the vector path."""
    assert vec == (D % 4 == 0)
    for sep in (False, True):
        for B in sorted(set(P.edge_batches(P.bwd_form(D, NL, vec, sep)["rpb"])) | set(P.edge_batches(P.fwd_form(D, NL, vec)["rpb"]))):
            _check_int(D, NL, B, density, sep)


@pytest.mark.parametrize("sep", [False, True], ids=["x", "x0"])
@pytest.mark.parametrize("D,NL,vec,density", P.PIPE_CASES, ids=_ids(P.PIPE_CASES))
def test_backward_three_trips_of_the_pipelined_row_loop(D, NL, vec, density, sep):
    _check_int(D, NL, P.pipe_batch(D, NL, vec, sep), density, sep)


@pytest.mark.parametrize("D,NL,vec,density", P.FWD_PIPE_CASES, ids=_ids(P.FWD_PIPE_CASES))
def test_forward_three_trips_of_the_row_loop(D, NL, vec, density):
    B = P.fwd_pipe_batch(D, NL, vec)
    i = P.int_inputs(D, NL, B, density)
    for sep in (False, True):
        _exact(dict(out=fwd(i, sep)), P.dcn(i["x"], i["w"], i["b"], x0=i["x0"] if sep else None), (D, NL, B, sep))


# ------------------------------------------------------------------------------------------------- b. layout variants
@pytest.mark.parametrize("D,NL,density", P.LAYOUT_CASES, ids=[f"D{d}-L{nl}" for d, nl, _ in P.LAYOUT_CASES])
def test_padded_and_unaligned_operands_give_the_same_bits(D, NL, density):
    """D % 4 == 0.  Every leading dimension padded by 4: still the vector form.  Padded by 3, or the pointer one float on -- all operands, or one
    alone while the rest stay aligned: the scalar form, R = 2 / 8 / 16 / 32 chunks per lane.  Only loads and stores change: the int64 bits."""
    every = lambda lay: {k: lay for k in OPERANDS}           # noqa: E731
    lays = [every((4, 0)), every((3, 0)), every((0, 1)), every((3, 1))] + [{k: (0, 1)} for k in OPERANDS] + [{"x": (3, 0)}, {"g_x": (1, 0)}]
    for B in (37, 101):
        for lay in lays:
            for sep in (False, True):
                if not sep and set(lay) <= {"x0", "g_x0"}:
                    continue
                _check_int(D, NL, B, density, sep, lay, modes=tuple(sorted({False, P.ordered_takes(D, NL)})) if len(lay) > 1 else (False,),
                           forward=len(lay) > 1 or set(lay) <= {"x", "x0", "out"})


@pytest.mark.parametrize("D,NL,density", P.LAYOUT_CASES, ids=[f"D{d}-L{nl}" for d, nl, _ in P.LAYOUT_CASES])
def test_cat_form_forward_and_the_backward_reading_x_from_it(D, NL, density):
    """out = x + D with ld = 2 D (ops.dcn_v1_cat_), then the backward with x_ld = 2 D."""
    B = 37
    i = P.int_inputs(D, NL, B, density)
    want = P.dcn(i["x"], i["w"], i["b"], i["g"])
    cat = Buf(B, 2 * D, data=np.concatenate([i["x"].astype(F32), np.full((B, D), np.nan, F32)], axis=1))
    wb, bb = _buf(NL, D, data=i["w"]), _buf(NL, D, data=i["b"])
    assert cat.ld == 2 * D
    _ok(_lib.load().nrx_dcn_v1_fwd(cat.ptr, cat.ld, None, 0, B, D, NL, wb.ptr, bb.ptr, cat.ptr + 4 * D, cat.ld, _stream()), "nrx_dcn_v1_fwd(cat)")
    both = cat.read()
    assert P.same_bits(both[:, :D], i["x"].astype(F32)) and P.same_bits(both[:, D:], want["out"].astype(F32))
    for ordered in (False, True):
        if not ordered or P.ordered_takes(D, NL):
            _exact(bwd(i, False, ordered, x_at=(cat.ptr, cat.ld)), want, (D, NL, ordered))


# ------------------------------------------------------------------------------------------------- c. real-valued inputs
@pytest.mark.parametrize("D,NL,vec", P.REAL_CASES, ids=_ids(P.REAL_CASES))
def test_real_inputs_inside_the_bounds_and_rows_independent_of_their_place(D, NL, vec):
    B = P.REAL_BATCH
    i = P.real_inputs(D, NL, B)
    rev = {k: (v[::-1] if k in ("x", "x0", "g") else v) for k, v in i.items()}
    for sep in (False, True):
        ref, bnd = P.bounds(i["x"], i["w"], i["b"], i["g"], i["x0"] if sep else None, P.dot_roundings(D, vec))
        got = dict(out=fwd(i, sep), **bwd(i, sep, False))
        for key in P.OUTPUTS:
            if ref[key] is not None:
                r = _ratio(got[key], ref[key], bnd[key])
                _note(f"{key} D={D} NL={NL} sep={sep}", r)
                assert r <= 1.0, (key, sep, r)
        if P.ordered_takes(D, NL):
            o = bwd(i, sep, True)
            for key in ("g_w", "g_b"):
                r = _ratio(o[key], ref[key], bnd[key])
                _note(f"{key} ordered D={D} NL={NL} sep={sep}", r)
                assert r <= 1.0, (key, sep, r)
            assert P.same_bits(o["g_x"], got["g_x"]) and (not sep or P.same_bits(o["g_x0"], got["g_x0"]))
        # the rows reversed (another wavefront, another block), one row fewer (the other half of the wavefront once reversed)
        rows = [k for k in ("out", "g_x", "g_x0") if got[k] is not None]
        r1 = dict(out=fwd(rev, sep), **bwd(rev, sep, False))
        short = {k: (v[:B - 1] if k in ("x", "x0", "g") else v) for k, v in i.items()}
        r2 = dict(out=fwd(short, sep), **bwd(short, sep, False))
        srev = {k: (v[::-1] if k in ("x", "x0", "g") else v) for k, v in short.items()}
        r3 = dict(out=fwd(srev, sep), **bwd(srev, sep, False))
        for key in rows:
            assert P.same_bits(r1[key][::-1], got[key]), (key, sep)
            assert P.same_bits(r2[key], got[key][:B - 1]), (key, sep)
            assert P.same_bits(r3[key][::-1], got[key][:B - 1]), (key, sep)


# ------------------------------------------------------------------------------------------------- d. the block-order sum
@pytest.mark.parametrize("blocks", P.REDUCE_BLOCKS)
def test_block_order_sum_bit_for_bit_at_its_loop_edges(blocks):
    """dcn_v1_reduce_kernel: 16 threads per output, each a stride of 32 blocks and a tail of 16."""
    D, NL = P.REDUCE_D, P.REDUCE_NL
    B = 16 * blocks - 5
    assert -(-B // P.bwd_form(D, NL, True, False)["rpb"]) == blocks
    _check_int(D, NL, B, P.REDUCE_DENSITY, False, modes=(True,), forward=False)


def test_block_order_sum_real_valued_in_bound_and_reproducible():
    D, NL, B = P.REDUCE_D, P.REDUCE_NL, 16 * 49 - 5
    i = P.real_inputs(D, NL, B)
    ref, bnd = P.bounds(i["x"], i["w"], i["b"], i["g"], None, P.dot_roundings(D, True))
    runs = [bwd(i, False, True) for _ in range(3)]
    for key in ("g_x", "g_w", "g_b"):
        r = _ratio(runs[0][key], ref[key], bnd[key])
        _note(f"{key} ordered 49 blocks", r)
        assert r <= 1.0, (key, r)
        assert P.same_bits(runs[1][key], runs[0][key]) and P.same_bits(runs[2][key], runs[0][key]), key


@pytest.mark.parametrize("D,NL,density", P.REDUCE_SHAPES, ids=[f"{d * nl}-outputs" for d, nl, _ in P.REDUCE_SHAPES])
def test_block_order_sum_output_counts(D, NL, density):
    for sep in (False, True):
        _check_int(D, NL, 101, density, sep, modes=(True,), forward=False)


# ------------------------------------------------------------------------------------------------- e. limits and refusals
def test_largest_stacks_each_entry_point_takes():
    B = 37
    for D, NL, vec in P.FWD_LARGEST:
        i = P.int_inputs(D, NL, B, P.LARGEST_DENSITY[(D, NL)])
        for sep in (False, True):
            _exact(dict(out=fwd(i, sep)), P.dcn(i["x"], i["w"], i["b"], x0=i["x0"] if sep else None), (D, NL, sep))
    for D, NL, vec in P.BWD_LARGEST:
        for sep in (False, True):
            _check_int(D, NL, B, P.LARGEST_DENSITY[(D, NL)], sep, forward=False)


def test_smallest_stacks_refused_and_bad_arguments_write_nothing():
    B = 3
    for D, NL in P.FWD_REFUSED:
        fwd(None, False, expect=NRX_ERR_BAD_ARG, dims=(B, D, NL))
        fwd(None, True, expect=NRX_ERR_BAD_ARG, dims=(B, D, NL))
    for D, NL in P.BWD_REFUSED:
        for sep in (False, True):
            bwd(None, sep, False, expect=NRX_ERR_BAD_ARG, dims=(B, D, NL))
    bwd(None, False, True, expect=NRX_ERR_BAD_ARG, dims=(B, 2049, 1))
    bwd(None, False, True, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 9))
    for D, NL in ((1000, 8), (2048, 4), (2048, 5), (1368, 2)):       # the ordered mode: beyond its LDS slabs
        for sep in (False, True):
            bwd(None, sep, True, expect=NRX_ERR_UNSUPPORTED, dims=(B, D, NL))
    fwd(None, False, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("w",))
    fwd(None, False, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("b",))
    for ordered in (False, True):
        bwd(None, False, ordered, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("w",))
        bwd(None, False, ordered, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("g_w",))
        bwd(None, False, ordered, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("g_x0",))      # x0 without g_x0
        bwd(None, False, ordered, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("x0",))        # g_x0 without x0
    bwd(None, False, True, expect=NRX_ERR_BAD_ARG, dims=(B, 16, 2), null=("ws",))
    i = P.int_inputs(16, 2, B, 1.0)                                    # the same shape with good arguments goes through
    _check_int(16, 2, B, 1.0, True)
    assert fwd(i, False) is not None


def test_empty_batch_is_ok_and_writes_nothing():
    for D, NL in ((16, 2), (37, 0), (320, 5)):
        for sep in (False, True):
            fwd(None, sep, dims=(0, D, NL))
            bwd(None, sep, False, dims=(0, D, NL))
            bwd(None, sep, True, dims=(0, D, NL))


# ------------------------------------------------------------------------------------------------- f. fused gather + cross
def fused(i, dims, B, bits, ld_pad=0):
    """nrx_embed_dcn_v1_fwd: returns (gathered half, cross half, status words)."""
    NL, W = i["w"].shape[0], sum(dims)
    tt = [torch.from_numpy(t.astype(F32)).to(DEV) for t in i["tables"]]
    ii = [torch.from_numpy(k.astype(np.int64 if bits == 64 else np.int32)).to(DEV) for k in i["ids"]]
    w, b = torch.from_numpy(i["w"].astype(F32)).to(DEV), torch.from_numpy(i["b"].astype(F32)).to(DEV)
    status = torch.zeros(8, dtype=torch.int32, device=DEV)
    feats = (NrxFeature * len(dims))()
    col = 0
    for f, t, k, d in zip(feats, tt, ii, dims):
        assert t.shape[1] == d and k.shape[0] == B and t.data_ptr() % 16 == 0
        f.table, f.index, f.weight, f.rows, f.dim, f.bag_len, f.kind = t.data_ptr(), k.data_ptr(), None, t.shape[0], d, 0, NRX_SPARSE
        f.index_bits, f.out_col, f.wide_col, f.fm_field, f.flags = bits, col, -1, 0, 0
        col += d
    assert col == W and 2 * NL * W * 4 <= P.LDS_FWD
    out = _buf(B, 2 * W, (ld_pad, 0))
    assert out.ld % 4 == 0 and out.ptr % 16 == 0
    _ok(_lib.load().nrx_embed_dcn_v1_fwd(feats, len(dims), B, W, out.ptr, out.ld, NL, w.data_ptr(), b.data_ptr(), status.data_ptr(), _stream()),
        "nrx_embed_dcn_v1_fwd")
    both = out.read()
    return both[:, :W], both[:, W:], status.cpu().numpy()


def _check_fused(dims, NL, B, bits, density, ld_pad=0, bad=None):
    i = P.fused_inputs(dims, NL, B, density, bad)
    x, cross, status = fused(i, dims, B, bits, ld_pad)
    tag = (dims, NL, B, bits)
    assert P.same_bits(x, i["x"].astype(F32)), tag
    assert P.same_bits(cross, P.dcn(i["x"], i["w"], i["b"])["out"].astype(F32)), tag
    if bad is None:
        assert not status.any(), tag
    else:
        assert list(status[:4]) == [1, bad[0], bad[1], bad[2]], (tag, status)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("D0", P.GROUPED_D0)
@pytest.mark.parametrize("N", P.GROUPED_N)
def test_fused_grouped_kernel_every_instantiation(N, D0, bits):
    dims = [D0] * N
    assert P.fused_form(dims)["kernel"] == "group_persist"
    for B in P.grouped_batches(D0):
        _check_fused(dims, P.grouped_layers(N), B, bits, P.GROUPED_DENSITY.get((D0, N), 1.0), ld_pad=8 if B % 2 else 0)


@pytest.mark.parametrize("D0,bits,B", P.GROUPED_WRAPS)
def test_fused_grouped_kernel_second_tile(D0, bits, B):
    """More rows than 4096 resident blocks hold: load_ids(b + stride) runs, and a few blocks take a second, ragged tile."""
    _check_fused([D0] * 2, P.grouped_layers(2), B, bits, 1.0)


@pytest.mark.parametrize("case", range(len(P.GENERAL_CASES)), ids=[f"W{sum(d)}" for d, _ in P.GENERAL_CASES])
def test_fused_general_kernel_widths_and_tails(case):
    dims, NL = P.GENERAL_CASES[case]
    assert P.fused_form(dims)["kernel"] == "general"
    for B in P.general_batches(dims):
        _check_fused(dims, NL, B, 64 if B % 2 else 32, P.GENERAL_DENSITY[case], ld_pad=4 if B % 3 == 0 else 0)


def test_fused_general_kernel_wraps():
    dims, NL, B = P.GENERAL_WRAP
    _check_fused(dims, NL, B, 32, 1.0)


@pytest.mark.parametrize("dims,bits", [([128, 64, 32, 16, 16], 64), ([32] * 3, 32), ([64] * 5, 64)], ids=["general", "grouped32", "grouped64"])
def test_fused_out_of_range_id_is_reported_and_reads_row_0(dims, bits):
    """(The one-tile-per-block grouped kernel is reachable only through the NRX_EDCN_VARIANT measurement knob, read once per process: not run.)"""
    rows1 = 40 + 3 * 1
    for bad_id in (rows1, rows1 + 7, -1):
        _check_fused(dims, 2, 40, bits, 1.0, bad=(1, 5, bad_id))
