"""CPU checks of tests/wgrad_cases.py: its restatement of wgrad_shape() against the built library's workspace functions (they load without a
device), the forms its case lists cover -- a condition, so a list that stops reaching a form fails here --, its int64 reference against a naive
triple loop, and that the generator is deterministic."""
import itertools

import numpy as np
import pytest

from news_recsys_amd import _lib
from tests import wgrad_cases as wc

LINEAR = wc.linear_cases()
DCN2 = wc.dcn2_cases()


def _implied_splits(ws_bytes, M, N):
    """The slice count the library's wgrad_shape chose, from nrx_linear_wgrad_ordered_workspace = splits * (M N + M) * 4 + 512."""
    q, r = divmod(ws_bytes - 512, (M * N + M) * 4)
    assert r == 0 and q >= 1, (ws_bytes, M, N)
    return q


def test_wgrad_shape_equals_the_librarys_for_every_case_and_a_seeded_sweep():
    lib = _lib.load()
    shapes = {(c.M, c.N, c.batch) for c in LINEAR} | {(c.dim, c.dim, c.batch) for c in DCN2}
    rng = np.random.default_rng(wc.SEED)
    edge = [1, 2, 63, 64, 65, 127, 128, 129, 383, 384, 385, 388, 512, 513, 640, 700]
    for _ in range(3000):
        M = int(rng.choice(edge)) if rng.random() < 0.5 else int(rng.integers(1, 701))
        N = int(rng.choice(edge)) if rng.random() < 0.5 else int(rng.integers(1, 701))
        batch = int(rng.choice([1, 31, 32, 33, 255, 256, 257, 511, 512, 513])) if rng.random() < 0.3 else int(2 ** rng.uniform(0, 18.2))
        shapes.add((M, N, max(batch, 1)))
    assert len(shapes) > 3000
    for M, N, batch in sorted(shapes):
        got = lib.nrx_linear_wgrad_ordered_workspace(batch, M, N)
        small, nt, splits, kslice = wc.wgrad_shape(M, N, batch)
        assert _implied_splits(got, M, N) == splits and got == wc.linear_workspace_bytes(batch, M, N), (M, N, batch)
        assert kslice % 32 == 0 and (splits - 1) * kslice < batch <= splits * kslice, (M, N, batch)
    for D, batch in sorted({(c.dim, c.batch) for c in DCN2}):
        assert lib.nrx_dcn_v2_layer_bwd_workspace(batch, D) == wc.dcn2_workspace_bytes(batch, D), (D, batch)


def test_workspace_functions_reject_bad_sizes_and_handle_an_empty_batch():
    lib = _lib.load()
    assert lib.nrx_linear_wgrad_ordered_workspace(-1, 8, 8) == -1
    assert lib.nrx_linear_wgrad_ordered_workspace(5, 0, 8) == -1
    assert lib.nrx_linear_wgrad_ordered_workspace(5, 8, 0) == -1
    assert lib.nrx_linear_wgrad_ordered_workspace(5, -3, 8) == -1
    assert lib.nrx_linear_wgrad_ordered_workspace(0, 8, 8) == 256 == wc.linear_workspace_bytes(0, 8, 8)
    assert lib.nrx_dcn_v2_layer_bwd_workspace(-1, 8) == -1 and lib.nrx_dcn_v2_layer_bwd_workspace(4, 0) == -1


def test_the_issues_slice_counts():
    """The shapes were chosen for these launch shapes; a change of wgrad_shape that moves them has to move the lists too."""
    slices = lambda M, N, b: wc.wgrad_shape(M, N, b)[2]
    assert [slices(8, 8, b) for b in (255, 256, 257, 4096, 4097, 8192, 8193, 12545)] == [1, 1, 2, 16, 17, 32, 33, 50]
    assert wc.wgrad_shape(8, 8, 300)[3] == 256
    assert wc.wgrad_shape(64, 72, 1025)[1:] == (2, 3, 512) and wc.wgrad_shape(68, 8, 513)[1:] == (2, 2, 512)
    assert wc.wgrad_shape(384, 8, 600)[0] and not wc.wgrad_shape(388, 8, 600)[0]
    assert wc.wgrad_shape(388, 68, 2000)[:3] == (False, 8, 8)
    assert slices(16, 16, 300000) == 1172
    assert [slices(132, 132, b) for b in (513, 1025)] == [2, 3] and slices(388, 388, 257) == 2


def _values(cases, name):
    return {c.key[name] for c in cases}


def test_linear_cases_cover_every_form():
    assert _values(LINEAR, "tile") == {64, 128}
    assert _values(LINEAR, "path") == set(wc.PATHS)
    assert _values(LINEAR, "mode") == set(wc.MODES)
    assert _values(LINEAR, "bias") == {True, False}
    for name in ("partial_slab", "short_last", "ragged"):
        assert _values(LINEAR, name) == {True, False}, name
    # the slice counts at which wgrad_reduce_kernel changes behaviour (a loop in steps of 32 with a 16-wide tail), in the mode that runs it
    ordered = [c for c in LINEAR if c.mode == "ordered"]
    assert {1, 2, 16, 17, 32, 33} <= _values(ordered, "slices") and any(48 <= s < 64 for s in _values(ordered, "slices"))
    assert max(_values(ordered, "slices")) > 1024 and max(_values([c for c in LINEAR if c.mode == "atomic"], "slices")) > 1024
    assert {1, 2, 16, 17, 32, 33, 50} <= _values([c for c in LINEAR if c.mode == "atomic"], "slices")
    # several tiles, in rows and in columns
    assert any(c.key["tiles"] > 1 and c.N > 64 for c in LINEAR) and any(c.key["tiles"] > 1 and c.M > 64 for c in LINEAR)
    # every mode x bias for each tile and for each path
    have = {(c.key["tile"], c.path, c.mode, c.bias) for c in LINEAR}
    want = set(itertools.product((64, 128), wc.PATHS, wc.MODES, (True, False)))
    assert want <= have, sorted(want - have)
    # padding behind the rows (poisoned by the GPU test) and none, for both operands; aligned and unaligned non-zero pointer offsets
    assert any(c.g_ld > c.M for c in LINEAR) and any(c.g_ld == c.M for c in LINEAR)
    assert any(c.a_ld > c.N for c in LINEAR) and any(c.a_ld == c.N for c in LINEAR)
    assert any(c.path == "vec" and (c.g_off or c.a_off) for c in LINEAR)
    assert any(c.path == "scalar-by-pointer" and c.g_off % 4 and not c.a_off % 4 for c in LINEAR)
    assert any(c.path == "scalar-by-pointer" and c.a_off % 4 and not c.g_off % 4 for c in LINEAR)
    assert any(c.path == "scalar-by-ld" and c.g_ld % 4 and not c.a_ld % 4 for c in LINEAR)
    assert any(c.path == "scalar-by-ld" and c.a_ld % 4 and not c.g_ld % 4 for c in LINEAR)
    # a slice shorter than a slab on the float4 path and on the scalar one
    assert {c.path for c in LINEAR if c.key["short_last"]} >= {"vec", "scalar-by-ld", "scalar-by-pointer"}
    assert len({c.name for c in LINEAR}) == len(LINEAR) and [c.index for c in LINEAR] == list(range(len(LINEAR)))
    assert all(c.batch * max(c.g_ld, c.a_ld) * 4 <= 24 << 20 for c in LINEAR)          # operands stay small


def test_dcn2_cases_cover_every_form():
    assert {c.dim for c in DCN2} == {8, 112, 116, 37, 132, 388}
    assert {1, 7, 8, 63, 64, 65} <= {c.batch for c in DCN2}
    assert _values(DCN2, "tile") == {64, 128} and _values(DCN2, "path") == {"vec", "scalar"}
    assert _values(DCN2, "form") == {"panel", "three-launch"}
    assert _values(DCN2, "dgrad") == {"panel", "split", "fp32"}
    assert _values(DCN2, "wgrad") == {"ordered", "split-atomic", "atomic"}
    assert {1, 2, 3, 17} <= _values(DCN2, "slices")
    for dim in (8, 112, 116, 37, 132, 388):
        mine = [c for c in DCN2 if c.dim == dim]
        assert {c.flags for c in mine} == set(range(8)) and {c.acc for c in mine} == set(wc.ACCS) and {c.pad for c in mine} == set(wc.PADS), dim
        assert {(c.flags, c.pad) for c in mine} == set(itertools.product(range(8), wc.PADS)), dim
        assert {(c.flags & 1, c.acc) for c in mine} == set(itertools.product((0, 1), wc.ACCS)), dim
        assert max(c.key["slices"] for c in mine) >= 2, dim
        for batch in {c.batch for c in mine}:
            assert {c.flags for c in mine if c.batch == batch} == set(range(8)), (dim, batch)
    assert {(c.acc, c.pad) for c in DCN2} == set(itertools.product(wc.ACCS, wc.PADS))
    # the forms per width, as the issue names them
    forms = lambda dim: {(c.key["form"], c.key["path"], c.key["wgrad"]) for c in DCN2 if c.dim == dim}
    assert ("panel", "vec", "ordered") in forms(8) and ("panel", "vec", "ordered") in forms(112)
    assert forms(116) == {("three-launch", "vec", "ordered"), ("three-launch", "scalar", "ordered")}
    assert forms(37) == {("three-launch", "scalar", "ordered")}
    for dim, tile in ((132, 64), (388, 128)):
        assert forms(dim) >= {("three-launch", "vec", w) for w in ("atomic", "split-atomic", "ordered")} | {("three-launch", "scalar", "atomic")}
        assert {c.key["tile"] for c in DCN2 if c.dim == dim} == {tile}
        # the split form on either side of its batch >= 8 condition, and with more than one slice
        assert {c.batch for c in DCN2 if c.dim == dim and c.key["wgrad"] == "split-atomic"} >= {8, 63, 64, 65}
        assert any(c.key["wgrad"] == "split-atomic" and c.key["slices"] >= 2 for c in DCN2 if c.dim == dim)
        assert any(c.batch == 7 and c.flags & 2 and not c.flags & 4 and c.key["wgrad"] == "atomic" and c.key["path"] == "vec" for c in DCN2 if c.dim == dim)
    assert len({c.name for c in DCN2}) == len(DCN2) and [c.index for c in DCN2] == list(range(len(DCN2)))


def _naive(case, ops):
    """The definitions of nrx_dcn2_bwd.hip's header comment as plain Python loops over integers."""
    I = lambda x: [[int(v) for v in row] for row in x]
    if isinstance(case, wc.LinearCase):
        g, a = I(ops["g"]), I(ops["a"])
        gW = [[sum(g[b][i] * a[b][j] for b in range(case.batch)) for j in range(case.N)] for i in range(case.M)]
        return dict(g_W=gW, g_b=[sum(g[b][i] for b in range(case.batch)) for i in range(case.M)])
    B, D = case.batch, case.dim
    x0, xl, lin, g, gx0, W = (I(ops[k]) for k in ("x0", "xl", "lin", "g", "gx0", "W"))
    on = [[(not case.flags & 1) or float(ops["out"][b, j]) > 0.0 for j in range(D)] for b in range(B)]
    gm = [[g[b][j] if on[b][j] else 0 for j in range(D)] for b in range(B)]
    glin = [[gm[b][j] * x0[b][j] for j in range(D)] for b in range(B)]
    g_x0 = [[gm[b][j] * lin[b][j] + (gx0[b][j] if case.acc & 1 else 0) for j in range(D)] for b in range(B)]
    g_xl = [[gm[b][j] + sum(glin[b][k] * W[k][j] for k in range(D)) + (g_x0[b][j] if case.acc & 2 else 0) for j in range(D)] for b in range(B)]
    g_W = [[sum(glin[b][i] * xl[b][j] for b in range(B)) for j in range(D)] for i in range(D)]
    return dict(g_xl=g_xl, g_x0=g_x0, g_W=g_W, g_b=[sum(glin[b][i] for b in range(B)) for i in range(D)])


@pytest.mark.parametrize("case", [wc.LinearCase(0, 5, 3, 9, 6, 3, 0, 0, True, "atomic"), wc.Dcn2Case(0, 5, 6, 1, 3, 0), wc.Dcn2Case(1, 4, 3, 6, 1, 4)],
                         ids=lambda c: c.name)
def test_exact_reference_equals_a_naive_triple_loop(case):
    ops = wc.int_operands(case, wc.case_rng(case))
    ref, naive = wc.exact_reference(case, ops), _naive(case, ops)
    assert sorted(ref) == sorted(naive)
    for k in ref:
        assert ref[k].tolist() == naive[k], k


def test_operands_are_small_integers_and_the_relu_pattern_is_mixed():
    for case in (LINEAR[0], LINEAR[-1], DCN2[0], DCN2[-1], next(c for c in DCN2 if c.dim == 132 and c.batch == 1025)):
        ops = wc.int_operands(case, wc.case_rng(case))
        for k, v in ops.items():
            assert v.dtype == np.float32, k
            if k != "out":
                assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= wc.VMAX, k
        if "out" in ops and case.batch >= 63:
            out = ops["out"]
            neg_zero = (out == 0) & np.signbit(out)
            pos_zero = (out == 0) & ~np.signbit(out)
            assert neg_zero.any() and pos_zero.any() and (out < 0).any() and (out > 0).any()
            assert abs((out > 0).mean() - 0.5) > 0.02          # not half on


def test_the_generator_is_deterministic():
    assert wc.linear_cases() == LINEAR and wc.dcn2_cases() == DCN2
    for case in (LINEAR[3], LINEAR[70], DCN2[5], DCN2[200]):
        a, b = wc.int_operands(case, wc.case_rng(case)), wc.int_operands(case, wc.case_rng(case))
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    other = wc.int_operands(LINEAR[4], wc.case_rng(LINEAR[4]))          # (same shape as LINEAR[3]'s neighbour: another seed, other numbers)
    assert not np.array_equal(other["g"], wc.int_operands(LINEAR[5], wc.case_rng(LINEAR[5]))["g"])


@pytest.mark.parametrize("case", [c for c in LINEAR if (c.M, c.N, c.batch) in ((8, 8, 4097), (388, 68, 2000), (4, 12, 7)) and c.path == "vec" and c.bias],
                         ids=lambda c: c.name)
def test_a_single_dropped_or_doubled_batch_row_changes_an_output_word(case):
    """What the equality assertion of the GPU test can see: drop (or add twice) ONE batch row -- the first and the last of every slice -- and at
    least one float32 word of g_W and of g_b differs from the reference.  (A tolerance of sqrt(batch) * eps * max cannot see this.)"""
    ops = wc.int_operands(case, wc.case_rng(case))
    ref = wc.exact_reference(case, ops)
    f32 = lambda x: x.astype(np.float32).view(np.int32)
    _, _, splits, kslice = wc.wgrad_shape(case.M, case.N, case.batch)
    rows = sorted({0, case.batch - 1} | {s * kslice - 1 for s in range(1, splits)} | {s * kslice for s in range(1, splits)})
    g, a = ops["g"].astype(np.int64), ops["a"].astype(np.int64)
    for r in rows:
        for sign in (-1, 1):
            gW = ref["g_W"] + sign * np.outer(g[r], a[r])
            gb = ref["g_b"] + sign * g[r]
            assert (f32(gW) != f32(ref["g_W"])).any() and (f32(gb) != f32(ref["g_b"])).any(), (r, sign)
