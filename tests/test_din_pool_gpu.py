"""GPU checks of the fused target-attention pooling (csrc/nrx_din.hip, ops.din_pool) against the float64 restatement
tests/din_pool_ref.py within its bounds, at the cases of tests/din_pool_cases.py: the two entry points called directly (padded strides with
sentinels, lse, g_rows), the autograd operator (g_query, the table gradient in the dense, COO and sink modes), out-of-range ids, large
scores, bit equality run to run / sample alone / graph replay, and the allocator's peak."""
import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from tests import din_pool_cases as cases
from tests import din_pool_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -77.25
DN_MAX_BLOCKS, DN_WAVES = 2048, 4                    # csrc/nrx_din.hip: din_grid()'s cap, samples (waves) per workgroup


def _dev_case(c, table=None):
    t = torch.from_numpy(c["table"] if table is None else table).to(DEV)
    if c["bf16"]:
        t = t.to(torch.bfloat16)
    mask = None if c["mask_arr"] is None else torch.from_numpy(c["mask_arr"]).to(DEV)
    return t, torch.from_numpy(c["ids"]).to(DEV), mask


def _padded(a, pad):
    """[B, D] array in a [B, D + pad] device buffer full of sentinels; returns (buffer, the [B, D] view)."""
    B, D = a.shape
    buf = torch.full((B, D + pad), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, :D] = torch.from_numpy(a).to(DEV) if isinstance(a, np.ndarray) else a
    return buf, buf[:, :D]


def _pads_untouched(buf, D):
    return bool((buf[:, D:] == SENTINEL).all())


def make_buffers(c, pad=0, table=None):
    """Device inputs and sentinel-filled outputs of one case, query / out / g_out / g_query in row strides of D + pad floats."""
    t, ids, mask = _dev_case(c, table)
    B, L = ids.shape
    D = t.shape[1]
    qb, _ = _padded(c["query"], pad)
    gb, _ = _padded(c["g_out"], pad)
    return dict(t=t, ids=ids, mask=mask, q=qb, g=gb, ld=D + pad, scale=c["scale"],
                out=torch.full((B, D + pad), SENTINEL, dtype=torch.float32, device=DEV),
                g_query=torch.full((B, D + pad), SENTINEL, dtype=torch.float32, device=DEV),
                lse=torch.empty(B, dtype=torch.float32, device=DEV), g_rows=torch.empty((B * L, D), dtype=torch.float32, device=DEV))


def launch(b, status=None):
    """nrx_din_pool_fwd + _bwd through the C ABI on the current stream: two launches, nothing else."""
    lib = _lib.load()
    t, ids, ld = b["t"], b["ids"], b["ld"]
    B, L = ids.shape
    D = t.shape[1]
    flags = 1 if t.dtype is torch.bfloat16 else 0
    st = torch.cuda.current_stream().cuda_stream
    mp = None if b["mask"] is None else b["mask"].data_ptr()
    sp = None if status is None else status.data_ptr()
    _lib.check(lib.nrx_din_pool_fwd(t.data_ptr(), t.shape[0], D, flags, ids.data_ptr(), ids.element_size() * 8, mp, b["q"].data_ptr(), ld, B, L,
                                    b["scale"], b["out"].data_ptr(), ld, b["lse"].data_ptr(), sp, st), "nrx_din_pool_fwd")
    _lib.check(lib.nrx_din_pool_bwd(t.data_ptr(), t.shape[0], D, flags, ids.data_ptr(), ids.element_size() * 8, mp, b["q"].data_ptr(), ld, B, L,
                                    b["scale"], b["out"].data_ptr(), ld, b["lse"].data_ptr(), b["g"].data_ptr(), ld, b["g_query"].data_ptr(), ld,
                                    b["g_rows"].data_ptr(), st), "nrx_din_pool_bwd")
    return b


def run_kernels(c, pad=0, table=None, status=None):
    return launch(make_buffers(c, pad, table), status)


def check_against_ref(c, got, ref, bnd, D, label):
    B, L = ref["p"].shape
    ratios = dict(out=R.worst_ratio(got["out"][:, :D].cpu().numpy(), ref["out"], bnd["out"]),
                  lse=R.worst_ratio(got["lse"].cpu().numpy(), ref["lse"], bnd["lse"]),
                  g_query=R.worst_ratio(got["g_query"][:, :D].cpu().numpy(), ref["g_query"], bnd["g_query"]),
                  g_rows=R.worst_ratio(got["g_rows"].cpu().numpy().reshape(B, L, D), ref["g_rows"], bnd["g_rows"]))
    print(label, {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


@pytest.mark.parametrize("i", range(cases.N_CASES), ids=cases.case_id)
def test_kernels_match_the_float64_reference(i):
    c = cases.make_case(i)
    D = c["D"]
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    bnd = R.bounds(ref, c["table"], c["query"], c["scale"])
    pad = (0, 4, 12)[i % 3]
    got = run_kernels(c, pad)
    torch.cuda.synchronize()
    check_against_ref(c, got, ref, bnd, D, cases.case_id(i))
    assert _pads_untouched(got["out"], D) and _pads_untouched(got["g_query"], D)
    empty = np.isinf(ref["lse"])
    if empty.any():                                     # a sample with no kept entry: exact zeros, lse -inf, zero gradients
        e = torch.from_numpy(empty).to(DEV)
        assert bool((got["out"][e][:, :D] == 0).all()) and bool((got["lse"][e] == float("-inf")).all())
        assert bool((got["g_query"][e][:, :D] == 0).all())
        assert bool((got["g_rows"].view(len(empty), -1)[e] == 0).all())
    not_kept = torch.from_numpy(~ref["keep"].reshape(-1)).to(DEV)
    assert bool((got["g_rows"][not_kept] == 0).all())


@pytest.mark.parametrize("pad", [4, 12])
def test_padded_strides_at_the_history_shape(pad):
    c = cases.make_case(6)                              # L 50, prefix mask
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    got = run_kernels(c, pad)
    plain = run_kernels(c, 0)
    D = c["D"]
    assert torch.equal(got["out"][:, :D], plain["out"]) and torch.equal(got["g_query"][:, :D], plain["g_query"])
    assert torch.equal(got["g_rows"], plain["g_rows"]) and torch.equal(got["lse"], plain["lse"])
    assert _pads_untouched(got["out"], D) and _pads_untouched(got["g_query"], D)
    check_against_ref(c, got, ref, R.bounds(ref, c["table"], c["query"], c["scale"]), D, f"pad{pad}")


@pytest.mark.parametrize("i", [6, 3])
def test_scores_of_the_order_of_1e4(i):
    c = cases.make_case(i, amp=100.0)                   # |q . e| * scale ~ 1e4: exp() of the raw score overflows, the running maximum must not
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    assert np.abs(np.where(np.isinf(ref["lse"]), 0, ref["lse"])).max() > 3e3
    got = run_kernels(c, 0)
    assert bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["g_rows"]).all())
    check_against_ref(c, got, ref, R.bounds(ref, c["table"], c["query"], c["scale"]), c["D"], f"amp100-{i}")
    c["query"] = -c["query"]                            # the scores at -1e4
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    check_against_ref(c, run_kernels(c, 0), ref, R.bounds(ref, c["table"], c["query"], c["scale"]), c["D"], f"amp-100-{i}")


@pytest.mark.parametrize("idx64", [False, True])
def test_out_of_range_ids(idx64):
    """-1 and `rows`: IndexError in sync mode; the entry takes part as row 0 (here a row of data, to see it) and its g_rows row is 0."""
    c = cases.make_case(5 if idx64 else 10)             # L 17 / L 64, no mask; cases 5 and 10 have the id width asked for
    assert c["idx64"] == idx64 and c["mask_arr"] is None
    table = c["table"].copy()
    table[0] = np.random.default_rng(3).standard_normal(c["D"]).astype(np.float32)
    if c["bf16"]:
        table = cases.bf16_round(table)
    c["ids"][0, 0] = -1
    c["ids"][-1, -1] = cases.ROWS
    ref = R.din_pool_ref(table, c["ids"], None, c["query"], c["scale"], c["g_out"])
    assert ref["bad"].sum() == 2
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    got = run_kernels(c, 0, table=table, status=status)
    check_against_ref(c, got, ref, R.bounds(ref, table, c["query"], c["scale"]), c["D"], "oob")
    st = status.tolist()
    assert st[0] == 2 and st[1] == 0 and st[3] in (-1, cases.ROWS)
    assert bool((got["g_rows"][0] == 0).all()) and bool((got["g_rows"][-1] == 0).all())
    t, ids, _ = _dev_case(c, table)
    with pytest.raises(IndexError):
        ops.din_pool(t, ids, torch.from_numpy(c["query"]).to(DEV), index_check="sync")
    out = ops.din_pool(t, ids, torch.from_numpy(c["query"]).to(DEV), index_check="off")
    assert torch.equal(out, got["out"])


def test_bits_run_to_run_sample_alone_and_graph_replay():
    c = cases.make_case(11)                             # L 256, D 20, B 67, prefix mask
    assert c["B"] == 67
    a, b = run_kernels(c, 0), run_kernels(c, 0)
    for k in ("out", "lse", "g_query", "g_rows"):
        assert torch.equal(a[k], b[k]), k
    L = c["L"]
    for s in (0, 3, 66):                                # the sample alone: another batch size, another place in the batch
        one = dict(c, ids=c["ids"][s:s + 1], mask_arr=c["mask_arr"][s:s + 1], query=c["query"][s:s + 1], g_out=c["g_out"][s:s + 1])
        g = run_kernels(one, 0)
        assert torch.equal(g["out"][0], a["out"][s]) and torch.equal(g["lse"][0], a["lse"][s])
        assert torch.equal(g["g_query"][0], a["g_query"][s]) and torch.equal(g["g_rows"], a["g_rows"][s * L:(s + 1) * L])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    g = make_buffers(c, 0)
    with torch.cuda.graph(graph):
        launch(g)
    for k in ("out", "lse", "g_query", "g_rows"):       # the captured launches have not run: poison the outputs, replay twice
        g[k].fill_(float("nan"))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for k in ("out", "lse", "g_query", "g_rows"):
        assert torch.equal(a[k], g[k]), k


@pytest.mark.parametrize("i,over", [(14, {}), (17, dict(bf16=True, mask="holes"))], ids=["L3-D4", "L17-D16-bf16-holes"])
def test_a_wave_that_strides_to_a_second_sample(i, over):
    """din_grid() caps a launch at DN_MAX_BLOCKS = 2048 workgroups of 4 waves: from batch 8193 on a wave takes a second sample, whose ids it
    requested BEFORE it consumed the first (nxt = dn_load_ids(b + stride); cur = nxt) -- in the forward and in the backward kernel.
    B = 8192 + 4 + 3: seven waves take a second trip, four of them in one whole workgroup, three in a workgroup whose fourth wave is done.
    Against the float64 reference within its bounds, like every case; and samples 0..6 (first trip) and 8192..8198 (second trip, produced by
    the strided pass alone) give the same bits when each is run alone."""
    B = DN_MAX_BLOCKS * DN_WAVES + 4 + 3
    c = cases.make_case(i, B=B, **over)
    assert c["ids"].shape == (B, c["L"]) and (c["L"], c["D"]) in ((3, 4), (17, 16))
    D, L = c["D"], c["L"]
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    bnd = R.bounds(ref, c["table"], c["query"], c["scale"])
    got = run_kernels(c, 4)
    torch.cuda.synchronize()
    check_against_ref(c, got, ref, bnd, D, f"stride-{cases.case_id(i)}-B{B}")
    assert _pads_untouched(got["out"], D) and _pads_untouched(got["g_query"], D)
    second = slice(DN_MAX_BLOCKS * DN_WAVES, B)                          # what only the second trip produces, held to the reference on its own
    tail = {k: (v[second] if k != "g_rows" else v[second.start * L:]) for k, v in got.items() if k in ("out", "lse", "g_query", "g_rows")}
    check_against_ref(c, tail, {k: v[second] for k, v in ref.items()}, {k: v[second] for k, v in bnd.items()}, D, "second trip")
    plain = run_kernels(c, 0)
    for s in list(range(7)) + list(range(second.start, B)):
        one = dict(c, ids=c["ids"][s:s + 1], mask_arr=None if c["mask_arr"] is None else c["mask_arr"][s:s + 1], query=c["query"][s:s + 1],
                   g_out=c["g_out"][s:s + 1])
        g = run_kernels(one, 0)
        assert torch.equal(g["out"][0], plain["out"][s]) and torch.equal(g["lse"][0], plain["lse"][s]), s
        assert torch.equal(g["g_query"][0], plain["g_query"][s]) and torch.equal(g["g_rows"], plain["g_rows"][s * L:(s + 1) * L]), s


def _sink_dense(sink, rows, D):
    """The dense gradient the sink's entries add up to (host side)."""
    g = torch.zeros((rows, D), dtype=torch.float64)
    for ent in sink.pending:
        uniq, vals = ent["uniq"].cpu(), ent["values"].cpu().double()
        sel = uniq >= 0 if ent.get("filler") else torch.arange(len(uniq)) < int(ent["counts"][0])
        g.index_add_(0, uniq[sel] & ((1 << 40) - 1), vals[sel])
    return g.numpy()


@pytest.fixture(scope="module")
def grad_case():
    """B = 67, L = 17, D = 16 with holes and kept id-0 entries; the float64 table gradient and its bound."""
    rng = np.random.default_rng(77)
    B, L, D = 67, 17, 16
    table = rng.standard_normal((cases.ROWS, D)).astype(np.float32)
    table[0] = 0
    ids = np.where(rng.random((B, L)) < 0.1, 0, rng.integers(1, cases.ROWS, (B, L))).astype(np.int64)
    mask = (rng.random((B, L)) < 0.8).astype(np.float32)
    mask[5] = 0
    c = dict(table=table, ids=ids, mask_arr=mask, query=rng.standard_normal((B, D)).astype(np.float32),
             g_out=rng.standard_normal((B, D)).astype(np.float32), scale=D ** -0.5, bf16=False, B=B, L=L, D=D)
    ref = R.din_pool_ref(table, ids, mask, c["query"], c["scale"], c["g_out"])
    bnd = R.bounds(ref, table, c["query"], c["scale"])
    c["ref"], c["bnd"] = ref, bnd
    c["g_table"], c["g_table_bound"] = R.table_grad_ref(ref, ids, cases.ROWS, bnd)
    return c


def _apply(c, sparse_grad, table=None):
    t, ids, mask = _dev_case(c, table)
    t = t.clone().requires_grad_(True)
    q = torch.from_numpy(c["query"]).to(DEV).requires_grad_(True)
    out = ops.din_pool(t, ids, q, mask, sparse_grad=sparse_grad, index_check="sync")
    out.backward(torch.from_numpy(c["g_out"]).to(DEV))
    return t, q, out


def test_table_gradient_dense_mode(grad_case):
    c = grad_case
    before = ops.din_pool_calls
    t, q, out = _apply(c, False)
    assert ops.din_pool_calls == before + 1
    assert t.grad is not None and not t.grad.is_sparse and bool((t.grad[0] == 0).all())
    r = R.worst_ratio(t.grad.cpu().numpy(), c["g_table"], c["g_table_bound"])
    rq = R.worst_ratio(q.grad.cpu().numpy(), c["ref"]["g_query"], c["bnd"]["g_query"])
    print("dense table grad", round(r, 4), "g_query", round(rq, 4))
    assert r <= 1.0 and rq <= 1.0
    # din_pool_math + torch's autograd on the same device: the same numbers within the bounds
    t2 = torch.from_numpy(c["table"]).to(DEV).requires_grad_(True)
    q2 = torch.from_numpy(c["query"]).to(DEV).requires_grad_(True)
    o2 = ops.din_pool_math(t2, torch.from_numpy(c["ids"]).to(DEV), q2, torch.from_numpy(c["mask_arr"]).to(DEV))
    o2.backward(torch.from_numpy(c["g_out"]).to(DEV))
    g2 = t2.grad.cpu().numpy()
    g2[0] = 0                                                     # (torch gives the padding row a gradient; the library never does)
    assert R.worst_ratio(g2, c["g_table"], c["g_table_bound"]) <= 1.0
    assert R.worst_ratio(o2.detach().cpu().numpy(), c["ref"]["out"], c["bnd"]["out"]) <= 1.0
    assert R.worst_ratio(out.detach().cpu().numpy(), c["ref"]["out"], c["bnd"]["out"]) <= 1.0


def test_table_gradient_coo_mode(grad_case):
    c = grad_case
    t, q, _ = _apply(c, True)
    assert t.grad is not None and t.grad.is_sparse
    g = t.grad.coalesce().to_dense().cpu().numpy()
    assert not g[0].any()
    assert R.worst_ratio(g, c["g_table"], c["g_table_bound"]) <= 1.0


def test_table_gradient_sink_and_one_fused_adam_step(grad_case):
    from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
    c = grad_case
    sink = ops.SparseGradSink()
    t, q, _ = _apply(c, sink)
    assert t.grad is None and sink.pending
    g = _sink_dense(sink, cases.ROWS, c["D"])
    assert not g[0].any()
    assert R.worst_ratio(g, c["g_table"], c["g_table_bound"]) <= 1.0
    before = t.detach().clone()
    FusedSparseAdam(sink, lr=1e-2, params=[t]).step()
    torch.cuda.synchronize()
    moved = (t.detach() != before).any(dim=1).cpu().numpy()
    touched = np.zeros(cases.ROWS, dtype=bool)
    touched[np.unique(c["ids"])] = True
    touched[0] = False
    assert not moved[~touched].any() and not moved[0]
    assert moved[np.abs(c["g_table"]).max(axis=1) > 1e-3].all()
    # the first Adam step moves an element by lr * g / (|g| + eps): lr where the gradient is well away from 0
    big = np.abs(c["g_table"]) > 1e-3
    step = (before - t.detach()).cpu().numpy()
    np.testing.assert_allclose(step[big], 1e-2 * np.sign(c["g_table"][big]), rtol=1e-3)


def test_bf16_table_trains_through_the_sink_only(grad_case):
    c = dict(grad_case, bf16=True)
    table = cases.bf16_round(c["table"])
    ref = R.din_pool_ref(table, c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    bnd = R.bounds(ref, table, c["query"], c["scale"])
    want, want_b = R.table_grad_ref(ref, c["ids"], cases.ROWS, bnd)
    with pytest.raises(NotImplementedError, match="bf16"):
        _apply(c, False, table)
    with pytest.raises(NotImplementedError, match="bf16"):
        _apply(c, True, table)
    sink = ops.SparseGradSink()
    t, q, out = _apply(c, sink, table)
    assert t.dtype is torch.bfloat16 and t.grad is None
    assert R.worst_ratio(out.detach().cpu().numpy(), ref["out"], bnd["out"]) <= 1.0
    assert R.worst_ratio(q.grad.cpu().numpy(), ref["g_query"], bnd["g_query"]) <= 1.0
    assert R.worst_ratio(_sink_dense(sink, cases.ROWS, c["D"]), want, want_b) <= 1.0
    # frozen bf16 table: no sink needed, the query still gets its gradient
    tt, ids, mask = _dev_case(c, table)
    q2 = torch.from_numpy(c["query"]).to(DEV).requires_grad_(True)
    ops.din_pool(tt, ids, q2, mask).backward(torch.from_numpy(c["g_out"]).to(DEV))
    assert torch.equal(q2.grad, q.grad)


def test_query_as_a_column_slice_is_read_in_place_and_gets_its_gradient(grad_case):
    c = grad_case
    t, ids, mask = _dev_case(c)
    D = c["D"]
    wide = torch.randn(c["B"], 8 + D + 4, device=DEV)
    wide[:, 8:8 + D] = torch.from_numpy(c["query"]).to(DEV)
    wide.requires_grad_(True)
    out = ops.din_pool(t, ids, wide[:, 8:8 + D], mask)
    out.backward(torch.from_numpy(c["g_out"]).to(DEV))
    q = torch.from_numpy(c["query"]).to(DEV).requires_grad_(True)
    o2 = ops.din_pool(t, ids, q, mask)
    o2.backward(torch.from_numpy(c["g_out"]).to(DEV))
    assert torch.equal(out, o2) and torch.equal(wide.grad[:, 8:8 + D], q.grad)
    assert bool((wide.grad[:, :8] == 0).all()) and bool((wide.grad[:, 8 + D:] == 0).all())
    odd = torch.randn(c["B"], D + 3, device=DEV)[:, 3:]               # misaligned slice: a contiguous copy, the same result
    odd.copy_(q.detach())
    assert torch.equal(ops.din_pool(t, ids, odd, mask), o2)


def test_unsupported_shapes_raise():
    t = torch.zeros(9, 6, device=DEV)
    with pytest.raises(_lib.NrxError, match="unsupported"):
        ops.din_pool(t, torch.zeros(2, 3, dtype=torch.long, device=DEV), torch.zeros(2, 6, device=DEV))
    t = torch.zeros(9, 8, device=DEV)
    with pytest.raises(_lib.NrxError, match="unsupported"):
        ops.din_pool(t, torch.zeros(2, 257, dtype=torch.long, device=DEV), torch.zeros(2, 8, device=DEV))


def test_allocator_peak_of_forward_and_backward():
    """B = 4096, L = 64, D = 16: g_rows [B L, D] is 16.8 MB.  With the table frozen the peak rise of forward + backward stays below g_rows + the
    [B, D] tensors (out, g_query and autograd's copy of it: 3 x 262 KB) + lse, with 64 KB of slack for the allocator's 512-byte rounding and
    1 MiB for its large pool (a cached block above 1 MiB is handed out whole when the rest of it would be under 1 MiB, and counts whole; g_rows
    is the one allocation of that size): no second [B, L, D] tensor and no [B, L] score tensor exists.  With the table trained in the default mode the embedding backward adds what
    any single-valued feature of B L lookups costs it: its planning workspace over the flat ids -- the library reports the size, about 107 bytes per
    lookup here -- and the 97-row dense gradient; nothing else may appear."""
    B, L, D = 4096, 64, 16
    gen = torch.Generator(device="cpu").manual_seed(5)
    table = torch.randn(cases.ROWS, D, generator=gen).to(DEV)
    ids = torch.randint(1, cases.ROWS, (B, L), generator=gen).to(DEV)
    mask = (torch.rand(B, L, generator=gen) < 0.8).float().to(DEV)
    g = torch.randn(B, D, generator=gen).to(DEV)
    g_rows_bytes = B * L * D * 4
    small = 3 * B * D * 4 + B * 4 + 512

    def peak_rise(train_table):
        t = table.clone().requires_grad_(train_table)
        q = torch.randn(B, D, device=DEV).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.din_pool(t, ids, q, mask, index_check="off")
        out.backward(g)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak_rise(False)                                               # (first call: library load, stream objects)
    rise = peak_rise(False)
    slack = (64 << 10) + (1 << 20)
    print("peak rise, frozen table:", rise, "bound:", g_rows_bytes + small + slack)
    assert rise <= g_rows_bytes + small + slack
    lib = _lib.load()
    plan = ops.EmbedPlan([ops.Slot("din_pool", _lib.NRX_SPARSE, 0, D, 0, 0)], out_width=D)
    arr = ops._fill_features(plan, 0, 1, [table], [ids.view(-1)], [None])
    ws = max(lib.nrx_embed_bwd_dense_sorted_workspace(arr, 1, B * L, D, 1), lib.nrx_embed_bwd_dense_planned_workspace(arr, 1, B * L, D, 1),
             lib.nrx_embed_bwd_sorted_workspace(B * L, D) + lib.nrx_sparse_plan_workspace(B * L))
    peak_rise(True)
    rise = peak_rise(True)
    bound = g_rows_bytes + small + ws + 2 * cases.ROWS * D * 4 + slack + (1 << 20)      # (the workspace: a second large allocation)
    print("peak rise, trained table:", rise, "bound:", bound, "(workspace", ws, ")")
    assert rise <= bound                                           # (beyond the planner's own workspace: again no second [B, L, D] tensor)
