"""tests/dcn_v1_ref.py held to account on the CPU, so that the GPU tests (tests/test_dcn_v1_kernels_gpu.py) compare the kernels with something that has
itself been checked:
  * its definition is oracle/ref_np.py's dcn_v1, dcn_v1_reference_form and dcn_v1_bwd, reproduces the committed dcn1/a..d goldens, and its backward
    is float64 torch autograd of its forward, with and without a separate x0;
  * the launch arithmetic gives the rows per pass read off the source, and the case lists reach what their comments say: every body at one and two
    rows per wavefront, every block size, every R of the vector and of the scalar form, both LDS limits, a third trip of each pipelined body;
  * every integer case meets the exactness condition (so bit equality with int64 is owed, not hoped for);
  * a float32 restatement in the kernels' own order, fused or not, lies inside the bounds (they are not too tight), and every mutant leaves them
    on the real-valued inputs and differs on the integer ones (they are not so loose that they hide a structural mistake)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_np as R
from tests import dcn_v1_ref as P
from tests.conftest import GOLDEN

F32 = np.float32
KEYS = ("x", "w", "b", "g")


def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


def _int_batches(D, NL, vec):
    bs = set(P.edge_batches(P.fwd_form(D, NL, vec)["rpb"]))
    for sep in (False, True):
        bs |= set(P.edge_batches(P.bwd_form(D, NL, vec, sep)["rpb"]))
    return sorted(bs)


# ------------------------------------------------------------------------------------------------- launch arithmetic and case lists
def test_rows_per_pass_as_read_off_the_source():
    assert P.fwd_form(128, 3, True)["pass_rows"] == 16384 and P.fwd_form(4, 1, True)["pass_rows"] == 16384
    assert {P.fwd_form(d, 1, v)["pass_rows"] for d, v in ((132, True), (128, False), (2048, True), (1, False))} == {8192}
    for nl in (1, 2, 3, 4):
        assert P.bwd_form(112, nl, True, False)["pass_rows"] == 8192 and P.bwd_form(112, nl, True, False)["body"] == "reg"
        assert P.bwd_form(320, nl, True, False)["pass_rows"] == 4096 and P.bwd_form(320, nl, True, False)["body"] == "reg"
    assert P.bwd_form(112, 1, True, True) == P.bwd_form(112, 1, True, False) and P.bwd_form(320, 1, True, True)["body"] == "reg"
    for nl, sep in ((5, False), (0, False), (2, True), (8, True)):
        assert P.bwd_form(112, nl, True, sep)["pass_rows"] == 4096 and P.bwd_form(112, nl, True, sep)["body"] == "slab"
        assert P.bwd_form(320, nl, True, sep)["pass_rows"] == 2048 and P.bwd_form(320, nl, True, sep)["body"] == "slab"
    assert P.bwd_form(1000, 8, True, False)["pass_rows"] == 4096 and P.bwd_form(1000, 8, True, False)["body"] == "atomic"
    assert [P.bwd_form(320, nl, True, False)["threads"] for nl in (1, 2, 3, 4, 5)] == [1024, 1024, 512, 512, 256]
    assert [P.bwd_form(320, nl, True, False)["rpb"] for nl in (1, 2, 3, 4, 5)] == [16, 16, 8, 8, 4]
    assert [P.bwd_form(112, nl, True, False)["rpb"] for nl in (1, 2, 3, 4, 5)] == [32, 32, 16, 16, 8]
    assert P.fused_form([64] * 5)["pass_rows"] == 65536 and P.fused_form([32] * 5)["pass_rows"] == 131072
    assert [(P.fused_form([w])["R"], P.fused_form([w])["S"]) for w in (256, 260, 512, 516, 1024, 1028)] == [(1, 8), (2, 8), (2, 8), (4, 4), (4, 4), (8, 2)]
    assert P.fused_form([16], 65545)["pass_rows"] == 65536 and P.fused_form([1024, 4], 9)["pass_rows"] == 8


def test_case_lists_reach_what_they_claim():
    vec_w = {d for d, _, v, _ in P.INT_CASES if v}
    sca_w = {d for d, _, v, _ in P.INT_CASES if not v}
    assert vec_w == {4, 124, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048}
    assert sca_w == {1, 3, 63, 65, 127, 129, 255, 257, 513, 1001, 1025, 2047}
    assert {nl for _, nl, _, _ in P.INT_CASES} == {0, 1, 2, 3, 4, 5, 8}
    fwd = [P.fwd_form(d, nl, v) for d, nl, v, _ in P.INT_CASES]
    bwd = [P.bwd_form(d, nl, v, sep) for d, nl, v, _ in P.INT_CASES for sep in (False, True)]
    assert all(f["ok"] for f in fwd + bwd)
    for forms in (fwd, bwd):
        assert {f["R"] for f in forms if f["V"] == 4 and not f["half"]} == {1, 2, 4, 8} and any(f["half"] for f in forms)
        assert {f["R"] for f in forms if f["V"] == 1} == {1, 2, 4, 8, 16, 32}
    # every body at every block size it has, one and two rows per wavefront, vector and scalar, with and without a separate x0
    assert {(f["body"], f["threads"], f["half"]) for f in bwd} == {("reg", 1024, True), ("reg", 512, True), ("slab", 256, True),
                                                                  ("reg", 1024, False), ("reg", 512, False), ("slab", 256, False), ("atomic", 512, False)}
    for v in (4, 1):
        assert {(f["body"], f["threads"]) for f in bwd if f["V"] == v and not f["half"]} == {("reg", 1024), ("reg", 512), ("slab", 256), ("atomic", 512)}
    sepf = [P.bwd_form(d, nl, v, True) for d, nl, v, _ in P.INT_CASES]
    assert {(f["body"], f["half"]) for f in sepf} == {("reg", True), ("slab", True), ("reg", False), ("slab", False), ("atomic", False)}
    # register accumulation at R = 1 and R = 2, every layer count it has
    assert {(f["R"], nl) for (d, nl, v, _) in P.INT_CASES for f in [P.bwd_form(d, nl, v, False)] if f["body"] == "reg" and not f["half"]} >= \
        {(1, 1), (1, 3), (2, 2), (2, 3), (2, 4)}
    # both LDS limits, to the byte
    assert [P.fwd_form(*c)["smem"] for c in P.FWD_LARGEST] == [P.LDS_FWD, P.LDS_FWD]
    big = [P.bwd_form(d, nl, v, False) for d, nl, v in P.BWD_LARGEST]
    assert [(f["body"], f["ok"]) for f in big] == [("atomic", True), ("atomic", True), ("reg", True), ("reg", True)]
    assert big[0]["smem"] == 128000 and big[1]["smem"] == P.LDS_BWD and big[2]["smem"] > 64 * 1024 and big[3]["smem"] > 64 * 1024
    assert all(c[:2] in [k for k in P.LARGEST_DENSITY] for c in P.FWD_LARGEST + P.BWD_LARGEST)
    assert not P.fwd_form(1028, 8, True)["ok"] and not P.bwd_form(2048, 5, True, False)["ok"] and (1028, 8) in P.FWD_REFUSED and (2048, 5) in P.BWD_REFUSED
    assert not P.ordered_takes(1000, 8) and not P.ordered_takes(2048, 4) and P.ordered_takes(512, 4) and P.ordered_takes(344, 7)
    for d, nl, v, _ in P.INT_CASES + P.PIPE_CASES:           # the ordered mode refuses exactly the atomic body
        for vv in {v, False}:
            assert P.ordered_takes(d, nl) == (P.bwd_form(d, nl, vv, False)["body"] != "atomic"), (d, nl, vv)
            assert P.ordered_takes(d, nl) == (P.bwd_form(d, nl, vv, True)["body"] != "atomic"), (d, nl, vv)
    # a third trip of each pipelined body
    seen = set()
    for d, nl, v, _ in P.PIPE_CASES:
        for sep in (False, True):
            f, B = P.bwd_form(d, nl, v, sep), P.pipe_batch(d, nl, v, sep)
            assert -(-B // f["pass_rows"]) == 3 and B % f["rpb"] == 3 and B * d * 4 <= 16 << 20
            seen.add((f["body"], f["threads"], f["half"], sep))
    assert seen >= {(b, t, h, s) for b, t, h in (("slab", 256, True), ("slab", 256, False), ("atomic", 512, False)) for s in (False, True)}
    assert seen >= {("reg", 1024, True, False), ("reg", 1024, True, True), ("reg", 512, True, False), ("reg", 1024, False, False),
                    ("reg", 1024, False, True), ("reg", 512, False, False)}
    # layout variants: D % 4 == 0 down the scalar path
    assert [d for d, _, _ in P.LAYOUT_CASES] == [112, 320, 1000, 2044]
    assert [P.lanes(d, False)[2] for d, _, _ in P.LAYOUT_CASES] == [2, 8, 16, 32] and all(d % 4 == 0 for d, _, _ in P.LAYOUT_CASES)
    assert {P.bwd_form(d, nl, False, False)["body"] for d, nl, _ in P.LAYOUT_CASES} == {"reg", "slab", "atomic"}
    # real-valued inputs: every body, the production shapes
    assert {(112, 3, True), (320, 2, True), (640, 3, True)} <= set(P.REAL_CASES)
    real = {(P.bwd_form(d, nl, v, sep)["body"], P.bwd_form(d, nl, v, sep)["half"]) for d, nl, v in P.REAL_CASES for sep in (False, True)}
    assert real == {("reg", True), ("slab", True), ("reg", False), ("slab", False), ("atomic", False)}
    # the block-order sum
    f = P.bwd_form(P.REDUCE_D, P.REDUCE_NL, True, False)
    assert (f["body"], f["rpb"], f["cap"]) == ("reg", 16, 256) and P.REDUCE_BLOCKS == [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 256]
    assert [d * nl for d, nl, _ in P.REDUCE_SHAPES] == [4, 222, 2728] and all(P.ordered_takes(d, nl) for d, nl, _ in P.REDUCE_SHAPES)
    assert not P.ordered_takes(1365, 2) and not P.ordered_takes(1368, 2)          # 2728 outputs: the most a two-layer stack gets through
    # the fused forward: 28 grouped instantiations, the general kernel at each R and around each width switch
    assert len([(n, d0, i) for n in P.GROUPED_N for d0 in P.GROUPED_D0 for i in (32, 64)]) == 28
    assert all(P.fused_form([d0] * n)["kernel"] == "group_persist" for n in P.GROUPED_N for d0 in P.GROUPED_D0)
    assert [P.fused_form([d0] * 2)["TB"] for d0 in P.GROUPED_D0] == [32, 16]
    gen = [P.fused_form(dims) for dims, _ in P.GENERAL_CASES]
    assert all(f["kernel"] == "general" for f in gen) and [sum(dims) for dims, _ in P.GENERAL_CASES] == [16, 256, 260, 512, 516, 1024, 1028, 2048]
    assert [(f["R"], f["S"]) for f in gen] == [(1, 8), (1, 8), (2, 8), (2, 8), (4, 4), (4, 4), (8, 2), (8, 2)]
    assert all(2 * nl * sum(dims) * 4 <= P.LDS_FWD for dims, nl in P.GENERAL_CASES) and any(len(set(dims)) > 2 for dims, _ in P.GENERAL_CASES)
    assert any(2 * nl * sum(dims) * 4 == P.LDS_FWD for dims, nl in P.GENERAL_CASES)


# ------------------------------------------------------------------------------------------------- the definition
SHAPES = [(1, 4, 1), (100, 320, 2), (65, 37, 3), (31, 1000, 8), (9, 6, 0), (41, 96, 6), (33, 640, 2)]


@pytest.mark.parametrize("B,D,NL", SHAPES)
def test_definition_is_ref_np(B, D, NL):
    """ref_np.dcn_v1 evaluates in float32 (numpy's pairwise row sums: fewer roundings per term than the D + 6 allowed here, whatever the blocking);
    dcn_v1_bwd evaluates in float64 and rounds its results once."""
    i = P.real_inputs(D, NL, B)
    ref, bnd = P.bounds(i["x"], i["w"], i["b"], i["g"], n_dot=D + 6)
    assert _ratio(R.dcn_v1(i["x"], i["w"], i["b"]), ref["out"], bnd["out"]) <= 1.0
    gx, gw, gb = R.dcn_v1_bwd(i["x"], i["w"], i["b"], i["g"])
    for key, got in (("g_x", gx), ("g_w", gw), ("g_b", gb)):
        np.testing.assert_allclose(got, ref[key], rtol=1e-6, atol=1e-6 * max(1.0, np.abs(ref[key]).max(initial=0)))
    if D <= 96:
        assert _ratio(R.dcn_v1_reference_form(i["x"], i["w"], i["b"]), ref["out"], P.gamma(D + 8) / P.gamma(D + 6) * 4 * bnd["out"] + 1e-30) <= 1.0
    if NL == 0:
        assert np.array_equal(ref["out"], i["x"]) and np.array_equal(ref["g_x"], i["g"]) and ref["g_w"].shape == (0, D)
        sep = P.dcn(i["x"], i["w"], i["b"], i["g"], i["x0"])
        assert np.array_equal(sep["g_x"], i["g"]) and not sep["g_x0"].any()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_definition_reproduces_the_goldens(tag):
    g = dict(np.load(os.path.join(GOLDEN, "ops.npz"), allow_pickle=False))
    x, w, b, up = (g[f"dcn1/{tag}/{k}"] for k in ("x", "w", "b", "up"))
    got = P.dcn(x, w, b, up)
    for key, name in (("out", "out"), ("g_x", "gx"), ("g_w", "gw"), ("g_b", "gb")):
        want = g[f"dcn1/{tag}/{name}"]
        np.testing.assert_allclose(got[key], want, rtol=1e-4, atol=2e-6 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("B,D,NL", [(7, 5, 1), (12, 37, 3), (9, 64, 8)])
@pytest.mark.parametrize("sep", [False, True])
def test_backward_is_float64_autograd_of_the_forward(B, D, NL, sep):
    i = P.real_inputs(D, NL, B)
    t = {k: torch.from_numpy(i[k].astype(np.float64)).requires_grad_(k != "g") for k in KEYS + ("x0",)}
    z = t["x0"] if sep else t["x"]
    xl = t["x"]
    for l in range(NL):
        xl = z * (xl * t["w"][l]).sum(1, keepdim=True) + t["b"][l] + xl
    got = P.dcn(i["x"], i["w"], i["b"], i["g"], i["x0"] if sep else None)
    np.testing.assert_allclose(got["out"], xl.detach().numpy(), rtol=1e-13, atol=1e-13)
    (xl * t["g"]).sum().backward()
    for key, name in (("g_x", "x"), ("g_w", "w"), ("g_b", "b")) + ((("g_x0", "x0"),) if sep else ()):
        np.testing.assert_allclose(got[key], t[name].grad.numpy(), rtol=1e-12, atol=1e-12, err_msg=key)


# ------------------------------------------------------------------------------------------------- the exactness condition
def _margins(D, NL, B, density):
    i = P.int_inputs(D, NL, B, density)
    return [P.int_exact_margin(i["x"], i["w"], i["b"], i["g"], x0) for x0 in (None, i["x0"])]


@pytest.mark.parametrize("D,NL,vec,density", P.INT_CASES, ids=[f"D{d}-L{nl}-{'v' if v else 's'}" for d, nl, v, _ in P.INT_CASES])
def test_integer_cases_meet_the_exactness_condition(D, NL, vec, density):
    worst = max(m for B in _int_batches(D, NL, vec) for m in _margins(D, NL, B, density))
    print(f"dcn_v1_ref largest sum of |terms|: D={D} NL={NL} density={density} {worst:.3g}")
    assert worst < P.EXACT


def test_integer_cases_of_the_other_lists_meet_the_exactness_condition():
    for D, NL, vec, density in P.PIPE_CASES:
        for B in sorted({P.pipe_batch(D, NL, vec, sep) for sep in (False, True)}):
            assert max(_margins(D, NL, B, density)) < P.EXACT, (D, NL, B)
    for D, NL, vec, density in P.FWD_PIPE_CASES:
        B = P.fwd_pipe_batch(D, NL, vec)
        assert -(-B // P.fwd_form(D, NL, vec)["pass_rows"]) == 3 and max(_margins(D, NL, B, density)) < P.EXACT, (D, NL, B)
    assert {(P.fwd_form(d, nl, v)["half"], v) for d, nl, v, _ in P.FWD_PIPE_CASES} == {(True, True), (False, True), (False, False)}
    for D, NL, density in P.LAYOUT_CASES:
        for B in (37, 101):
            assert max(_margins(D, NL, B, density)) < P.EXACT, (D, NL, B)
    for k in P.REDUCE_BLOCKS:
        assert max(_margins(P.REDUCE_D, P.REDUCE_NL, 16 * k - 5, P.REDUCE_DENSITY)) < P.EXACT, k
    for D, NL, density in P.REDUCE_SHAPES:
        assert max(_margins(D, NL, 101, density)) < P.EXACT, (D, NL)
    for (D, NL), density in P.LARGEST_DENSITY.items():
        assert max(_margins(D, NL, 37, density)) < P.EXACT, (D, NL)


def test_fused_integer_cases_meet_the_exactness_condition():
    def margin(dims, NL, B, density):
        i = P.fused_inputs(dims, NL, B, density)
        assert i["x"].shape == (B, sum(dims)) and all(0 <= k.min() and k.max() < t.shape[0] for k, t in zip(i["ids"], i["tables"]))
        return P.int_exact_margin(i["x"], i["w"], i["b"], np.zeros_like(i["x"]))

    for (dims, NL), density in zip(P.GENERAL_CASES, P.GENERAL_DENSITY):
        assert max(margin(dims, NL, B, density) for B in P.general_batches(dims)) < P.EXACT, dims
    for D0 in P.GROUPED_D0:
        for N in P.GROUPED_N:
            density = P.GROUPED_DENSITY.get((D0, N), 1.0)
            assert max(margin([D0] * N, P.grouped_layers(N), B, density) for B in P.grouped_batches(D0)) < P.EXACT, (D0, N)
    for D0, _, B in P.GROUPED_WRAPS:
        assert B > P.fused_form([D0] * 2)["pass_rows"] and margin([D0] * 2, P.grouped_layers(2), B, 1.0) < P.EXACT
    dims, NL, B = P.GENERAL_WRAP
    assert B > P.fused_form(dims, B)["pass_rows"] == 65536 and margin(dims, NL, B, 1.0) < P.EXACT
    bad = P.fused_inputs([32] * 3, 2, 40, 1.0, bad=(1, 5, 50))
    assert bad["ids"][1][5] == 50 >= bad["tables"][1].shape[0] and np.array_equal(bad["x"][5, 32:64], bad["tables"][1][0])


def test_exactness_checker_refuses_what_would_round():
    i = P.int_inputs(2048, 4, 9, 1.0)                      # dense +-1 at the widest, deepest stack: the dot products leave 2^24
    assert P.int_exact_margin(i["x"], i["w"], i["b"], i["g"]) >= P.EXACT
    x = np.full((1, 4), 4096, np.int64)                    # one product of 2^12 x 2^12 is enough
    assert P.int_exact_margin(x, x, x * 0, x * 0) >= P.EXACT


# ------------------------------------------------------------------------------------------------- a float32 restatement in the kernels' order
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _row_dot32(a, b, V, fma):
    """row_dot: lane = chunk % 64 chains its chunks r = 0.. and the V floats of each in order, then the wavefront's tree."""
    B, D = a.shape
    n = -(-D // (64 * V)) * 64 * V
    pa, pb = np.zeros((B, n), F32), np.zeros((B, n), F32)
    pa[:, :D], pb[:, :D] = a, np.broadcast_to(b, a.shape)
    pa, pb = pa.reshape(B, -1, 64, V), pb.reshape(B, -1, 64, V)
    s = np.zeros((B, 64), F32)
    for r in range(pa.shape[1]):
        for j in range(V):
            s = _fma(pa[:, r, :, j], pb[:, r, :, j], s) if fma else s + (pa[:, r, :, j] * pb[:, r, :, j]).astype(F32)
    lanes = np.arange(64)
    for perm in (lanes ^ 1, lanes ^ 2, (lanes & ~7) | (7 - (lanes & 7)), (lanes & ~15) | (15 - (lanes & 15))):
        s = s + s[:, perm]
    return ((s[:, 0] + s[:, 16]) + (s[:, 32] + s[:, 48]))[:, None]


def _dcn32(i, sep, V, fma):
    """The kernels' float32 arithmetic, every multiply next to an add fused or none; the batch sums of g_w / g_b row by row."""
    x, w, b, g = (i[k] for k in KEYS)
    z = i["x0"] if sep else x
    NL = w.shape[0]
    mad = (lambda p, q, c: _fma(p, q, c)) if fma else (lambda p, q, c: (p * q).astype(F32) + c)
    xs, ss = [x], []
    for l in range(NL):
        s = _row_dot32(xs[-1], w[l], V, fma)
        xs.append(mad(z, s, np.broadcast_to(b[l], x.shape)) + xs[-1])
        ss.append(s)
    gx0 = np.zeros_like(x)
    gw, gb = np.zeros_like(w), np.zeros_like(w)
    for l in reversed(range(NL)):
        gs = _row_dot32(g, z, V, fma)
        for r in range(x.shape[0]):
            gb[l] = gb[l] + g[r]
            gw[l] = mad(np.broadcast_to(gs[r], xs[l][r].shape), xs[l][r], gw[l])
        gx0 = mad(g, ss[l], gx0)
        g = mad(np.broadcast_to(gs, g.shape), np.broadcast_to(w[l], g.shape), g)
    return dict(out=xs[-1], g_x=g if sep else g + gx0, g_x0=gx0 if sep else None, g_w=gw, g_b=gb)


@pytest.mark.parametrize("D,NL,vec", P.REAL_CASES, ids=[f"D{d}-L{nl}-{'v' if v else 's'}" for d, nl, v in P.REAL_CASES])
def test_restatement_lies_inside_the_bounds_and_mutants_leave_them(D, NL, vec):
    """Worst |restatement - float64| / bound over REAL_CASES (this run, numpy on the CPU): out 0.44, g_x 0.30, g_x0 0.078, g_w 0.016, g_b 0.023 --
    the roundings mostly cancel where the bound adds them up (the MI355X gave 0.44, 0.30, 0.074, 0.012, 0.012).  Every mutant lands outside the
    bound of the output it is meant to show in, by a factor of at least 26 at its worst element (the smallest: the last of 101 rows missing from g_w), and --
    where the output has rows -- on a majority of the rows it touches."""
    B = P.REAL_BATCH
    i = P.real_inputs(D, NL, B)
    for sep in (False, True):
        ref, bnd = P.bounds(i["x"], i["w"], i["b"], i["g"], i["x0"] if sep else None, P.dot_roundings(D, vec))
        for fma in (False, True):
            got = _dcn32(i, sep, 4 if vec else 1, fma)
            for key in P.OUTPUTS:
                if ref[key] is not None:
                    r = _ratio(got[key], ref[key], bnd[key])
                    print(f"dcn_v1_ref worst error / bound: {key} sep={sep} fma={fma} {r:.4f}")
                    assert r <= 1.0, (key, sep, fma, r)
        for mut in P.MUTANTS:
            if not P.mutant_applies(mut, D, NL, B, sep):
                continue
            bad = P.dcn(i["x"], i["w"], i["b"], i["g"], i["x0"] if sep else None, mut=mut)
            shows = [k for k in P.MUTANT_SHOWS[mut] if ref[k] is not None][:1]
            for key in shows:
                r = _ratio(bad[key], ref[key], bnd[key])
                print(f"dcn_v1_ref mutant error / bound: {mut} {key} sep={sep} {r:.3g}")
                assert r > 1.0, (mut, key, sep, r)
                if key != "g_w":                                   # ... and on a majority of the rows it touches
                    rows = (np.abs(bad[key] - ref[key]) > bnd[key]).any(1)
                    rows = rows[1::2] if mut == "pair_scalar" else rows
                    assert rows.sum() * 2 > rows.size, (mut, key, sep)


@pytest.mark.parametrize("D,NL,vec,density", P.INT_CASES[::3] + P.PIPE_CASES[::3])
def test_mutants_differ_on_the_integer_inputs(D, NL, vec, density):
    for sep in (False, True):
        B = P.edge_batches(P.bwd_form(D, NL, vec, sep)["rpb"])[-1]
        i = P.int_inputs(D, NL, B, density)
        x0 = i["x0"] if sep else None
        ref = P.dcn(i["x"], i["w"], i["b"], i["g"], x0)
        for mut in P.MUTANTS:
            if P.mutant_applies(mut, D, NL, B, sep) and not (D == 1 and mut == "xl_in_hadamard"):
                bad = P.dcn(i["x"], i["w"], i["b"], i["g"], x0, mut=mut)
                assert any(ref[k] is not None and not np.array_equal(ref[k], bad[k]) for k in P.MUTANT_SHOWS[mut]), (mut, sep)
