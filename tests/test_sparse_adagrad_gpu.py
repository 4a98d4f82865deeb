"""Fused row-sparse Adagrad (nrx_sparse_adagrad_step + optim.FusedSparseAdagrad) on the GPU.

  element-wise form   against torch.optim.Adagrad(lr_decay=0) fed the COO gradients of the sparse_grad=True path
  row-wise form       against a float64 restatement built from the same COO gradients: s += mean(g^2); w -= lr * g / (sqrt(s) + eps)
  the kernel alone    through ctypes: hand-made key lists (fillers, row 0, a table out of range, a device-side count, consecutive rows), every
                      lane-group width and the scalar form; rows that are not named keep their bits, in the tables and in the state
  order               a shuffled list and a list split over two launches leave the same bits (the row-wise sum has ONE order per dim)
  bf16 tables         the stored patterns are tests/sr_bf16_ref.py's rounding of the fp32 kernel's result, the state is the fp32 run's, an arena's
                      row map draws the full table's bits
  and the optimizer class through merging, checkpoints, graph capture, the model classes and the bound sharded step at world 1.

Tolerances: rtol 2e-5 / atol 2e-6 are the ones tests/test_fused_sparse_adam_gpu.py uses for the same comparison of an fp32 update (a handful of
fp32 roundings, 6e-8 each, on weights of order 1) with a float64 / torch restatement; everything called "the same bits" is compared as integers."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from news_recsys_amd import _lib, ops, shard_step
from news_recsys_amd._lib import NRX_ADAGRAD_ROWWISE, NRX_ADAGRAD_TABLE_BF16, NRX_FEAT_TABLE_BF16, NRX_SPARSE
from news_recsys_amd.model.model_utils.optim import FusedSparseAdagrad, SparseDenseAdam
from tests import sr_bf16_ref as SR
from tests.row_optim_ref import key_list as _key_list          # (n, rng): three tables of ROWS = 40 rows
from tests.test_fused_sparse_adam_gpu import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = torch.iinfo(torch.int64).max
RTOL, ATOL = 2e-5, 2e-6


def _i32(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype is torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype is b.dtype and torch.equal(_i32(a), _i32(b))


def _coo(t):
    g = t.grad.coalesce()
    return g.indices()[0], g.values()


# ------------------------------------------------------------------------------------------------ 1, 2: against torch / float64
@pytest.mark.parametrize("shared", [False, True])
def test_elementwise_matches_torch_adagrad_on_the_coo_gradients(shared):
    plan, tables, batch = _setup(5, shared)
    ref = [t.clone().requires_grad_(True) for t in tables]
    fus = [t.clone().requires_grad_(True) for t in tables]
    opt_ref = torch.optim.Adagrad(ref, lr=0.05, lr_decay=0, eps=1e-10, initial_accumulator_value=0)
    sink = ops.SparseGradSink()
    opt_fus = FusedSparseAdagrad(sink, lr=0.05, eps=1e-10, rowwise=False)
    for step in range(4):
        ins, ws, up = batch()
        opt_ref.zero_grad()
        (ops.embed_apply(plan, ref, ins, ws, sparse_grad=True)[0] * up).sum().backward()
        assert all(t.grad.is_sparse for t in ref)
        opt_ref.step()
        (ops.embed_apply(plan, fus, ins, ws, sparse_grad=sink)[0] * up).sum().backward()
        assert all(t.grad is None for t in fus) and len(sink.pending) == 2        # one entry per embedding dim
        opt_fus.step()
        assert not sink.pending
    moved = 0
    for a, b, t0 in zip(ref, fus, tables):
        torch.testing.assert_close(b.detach(), a.detach(), rtol=RTOL, atol=ATOL)
        assert torch.equal(b[0], torch.zeros_like(b[0]))                         # the padding row is exactly zero
        moved += int((b.detach() != t0).any(1).sum())
    assert moved > 100
    for a, s in zip(ref, [opt_fus.sums[opt_fus._index[id(t)]] for t in fus]):
        assert s.shape == a.shape
        torch.testing.assert_close(s, opt_ref.state[a]["sum"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("shared", [False, True])
def test_rowwise_matches_the_float64_restatement(shared):
    lr, eps = 0.05, 1e-10
    plan, tables, batch = _setup(5, shared)
    ref = [t.clone().requires_grad_(True) for t in tables]        # (only to form the COO gradients: they do not depend on the weights)
    fus = [t.clone().requires_grad_(True) for t in tables]
    w64 = [t.double().cpu() for t in tables]
    s64 = [torch.zeros(t.shape[0], dtype=torch.float64) for t in tables]
    sink = ops.SparseGradSink()
    opt = FusedSparseAdagrad(sink, lr=lr, eps=eps, rowwise=True)
    touched = 0
    for step in range(4):
        ins, ws, up = batch()
        for t in ref:
            t.grad = None
        (ops.embed_apply(plan, ref, ins, ws, sparse_grad=True)[0] * up).sum().backward()
        for t, w, s in zip(ref, w64, s64):
            rows, g = _coo(t)
            rows, g = rows.cpu(), g.double().cpu()
            live = rows != 0
            rows, g = rows[live], g[live]
            ssq = (g * g).sum(1)
            # the division by sqrt(s) + eps is well conditioned only if no touched row's gradient vanishes: asserted, not skipped
            assert float(ssq.min()) >= 1e-12, f"a touched row has a sum of squares of {float(ssq.min()):.3e}: pick another seed"
            s[rows] += ssq / g.shape[1]
            w[rows] -= lr * g / (s[rows].sqrt() + eps)[:, None]
            touched += rows.numel()
        (ops.embed_apply(plan, fus, ins, ws, sparse_grad=sink)[0] * up).sum().backward()
        opt.step()
    assert touched > 400
    for b, w, s in zip(fus, w64, s64):
        torch.testing.assert_close(b.detach().cpu().double(), w, rtol=RTOL, atol=ATOL)
        assert torch.equal(b[0], torch.zeros_like(b[0]))
        got = opt.sums[opt._index[id(b)]]
        assert got.shape == (b.shape[0],) and got.dtype is torch.float32
        torch.testing.assert_close(got.cpu().double(), s, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ 3: the kernel alone
ROWS = 40


def _call(tables, state, dim, keys, grads, flags, n_dev=None, lr=0.05, eps=1e-10, decay=0.0, seed=0, step=1, maps=None, n=None):
    lib = _lib.load()
    k = len(tables)
    tp = (C.c_void_p * k)(*[t.data_ptr() for t in tables])
    sp = (C.c_void_p * k)(*[s.data_ptr() for s in state])
    rmul = radd = None
    if maps is not None:
        rmul, radd = (C.c_int64 * k)(*[m for m, _ in maps]), (C.c_int64 * k)(*[a for _, a in maps])
    ops.check(lib.nrx_sparse_adagrad_step(tp, sp, k, dim, keys.data_ptr(), grads.data_ptr(), keys.numel() if n is None else n,
                                          n_dev.data_ptr() if n_dev is not None else None, lr, None, eps, decay, flags, seed, step, None, rmul, radd,
                                          torch.cuda.current_stream().cuda_stream), "nrx_sparse_adagrad_step")
    torch.cuda.synchronize()


def _restate(w, s, keys, g, rowwise, lr, eps, decay, n_tables=3):
    """float64: the update of every live key of the list."""
    w, s = [x.copy() for x in w], [x.copy() for x in s]
    named = [set() for _ in w]
    for i, k in enumerate(keys):
        t, r = int(k) >> 40, int(k) & ((1 << 40) - 1)
        if k < 0 or k == BIG or r == 0 or t >= n_tables:
            continue
        gi = g[i].astype(np.float64)
        if rowwise:
            s[t][r] += (gi * gi).sum() / gi.size
            den = np.sqrt(s[t][r]) + eps
        else:
            s[t][r] += gi * gi
            den = np.sqrt(s[t][r]) + eps
        w[t][r] = (w[t][r] - w[t][r] * decay) - lr * gi / den
        named[t].add(r)
    return w, s, named


@pytest.mark.parametrize("rowwise", [True, False])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("dim", [1, 6, 8, 16, 32, 112, 320])
def test_kernel_alone_on_hand_made_key_lists(dim, n, rowwise):
    rng = np.random.default_rng([dim, n, int(rowwise)])
    lr, eps, decay = 0.05, 1e-10, 1e-3
    keys, n_dev = _key_list(n, rng)
    g = rng.standard_normal((n, dim)).astype(np.float32)
    w0 = [rng.standard_normal((ROWS, dim)).astype(np.float32) for _ in range(3)]
    s0 = [(0.1 + rng.random((ROWS,) if rowwise else (ROWS, dim))).astype(np.float32) for _ in range(3)]
    tables = [torch.from_numpy(x).to(DEV) for x in w0]
    state = [torch.from_numpy(x).to(DEV) for x in s0]
    live_keys = keys if n_dev is None else keys[:n_dev]
    want_w, want_s, named = _restate([x.astype(np.float64) for x in w0], [x.astype(np.float64) for x in s0], live_keys, g, rowwise, lr, eps, decay)
    _call(tables, state, dim, torch.from_numpy(keys).to(DEV), torch.from_numpy(g).to(DEV), NRX_ADAGRAD_ROWWISE if rowwise else 0,
          n_dev=None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device=DEV), lr=lr, eps=eps, decay=decay)
    assert sum(len(x) for x in named) >= (90 if n == 257 else 1)
    if n_dev is not None:                    # the entry past the device-side count names a row no live entry names
        assert (int(keys[-1]) & 0xFFFFFFFFFF) not in named[int(keys[-1]) >> 40]
    for t in range(3):
        got_w, got_s = tables[t].cpu().numpy(), state[t].cpu().numpy()
        rows = np.array(sorted(named[t]), dtype=np.int64)
        rest = np.ones(ROWS, bool)
        rest[rows] = False
        # every row that is not named keeps its bits: the tables, and the state -- the neighbours in a named row's 128-byte line included
        assert np.array_equal(got_w[rest].view(np.int32), w0[t][rest].view(np.int32)), (t, "table rows that no key names moved")
        assert np.array_equal(got_s[rest].view(np.int32), s0[t][rest].view(np.int32)), (t, "state of rows that no key names moved")
        if rows.size:
            np.testing.assert_allclose(got_w[rows], want_w[t][rows], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(got_s[rows], want_s[t][rows], rtol=RTOL, atol=ATOL)
            assert not np.array_equal(got_w[rows], w0[t][rows])


@pytest.mark.parametrize("rowwise", [True, False])
@pytest.mark.parametrize("dim", [16, 320])
def test_misaligned_buffers_take_the_scalar_form_and_leave_the_same_bits(dim, rowwise):
    """The order of the row-wise sum depends on dim only: gradients that start 4 bytes off a 16-byte boundary go through the element-by-element form,
    whose lanes own the same columns."""
    rng = np.random.default_rng([77, dim])
    n = 37
    keys = torch.from_numpy(np.array([((i % 3) << 40) | (1 + i) for i in range(n)], dtype=np.int64)).to(DEV)
    g = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).to(DEV)
    buf = torch.zeros(n * dim + 1, device=DEV)
    g_off = buf[1:].view(n, dim)
    g_off.copy_(g)
    assert g_off.data_ptr() % 16 == 4
    outs = []
    for grads in (g, g_off):
        gen = torch.Generator(device=DEV).manual_seed(dim)
        tables = [torch.randn(ROWS, dim, device=DEV, generator=gen) for _ in range(3)]
        state = [torch.rand((ROWS,) if rowwise else (ROWS, dim), device=DEV, generator=gen) for _ in range(3)]
        _call(tables, state, dim, keys, grads, NRX_ADAGRAD_ROWWISE if rowwise else 0, decay=1e-3)
        outs.append(tables + state)
    for a, b in zip(*outs):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 4: order independence
def _fresh(dim, rowwise, bf16, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tables = [torch.randn(ROWS, dim, device=DEV, generator=gen) for _ in range(3)]
    if bf16:
        tables = [t.to(torch.bfloat16) for t in tables]
    state = [torch.rand((ROWS,) if rowwise else (ROWS, dim), device=DEV, generator=gen) for _ in range(3)]
    return tables, state


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("rowwise", [True, False])
@pytest.mark.parametrize("dim", [16, 320])
def test_a_shuffled_list_and_a_split_list_leave_the_same_bits(dim, rowwise, bf16):
    rng = np.random.default_rng([4, dim, int(rowwise), int(bf16)])
    real = [(t << 40) | r for t in range(3) for r in range(1, ROWS)]
    keys = np.array([real[i] for i in rng.permutation(len(real))[:90]] + [-1] * 5 + [BIG] * 5, dtype=np.int64)
    keys = keys[rng.permutation(keys.size)]
    n = keys.size
    g = rng.standard_normal((n, dim)).astype(np.float32)
    flags = (NRX_ADAGRAD_ROWWISE if rowwise else 0) | (NRX_ADAGRAD_TABLE_BF16 if bf16 else 0)
    kw = dict(decay=1e-3, seed=0x1234ABCD, step=7)
    perm = rng.permutation(n)
    runs = []
    for lists in ([(keys, g)], [(keys[perm], g[perm])], [(keys[: n // 2], g[: n // 2]), (keys[n // 2:], g[n // 2:])]):
        tables, state = _fresh(dim, rowwise, bf16, 40 + dim)
        for k, v in lists:
            _call(tables, state, dim, torch.from_numpy(np.ascontiguousarray(k)).to(DEV), torch.from_numpy(np.ascontiguousarray(v)).to(DEV), flags, **kw)
        runs.append(tables + state)
    t0, _ = _fresh(dim, rowwise, bf16, 40 + dim)
    assert not _same_bits(runs[0][0], t0[0])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 5: bf16 tables
def _bits16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("rowwise", [True, False])
@pytest.mark.parametrize("dim", [6, 16, 320])
def test_bf16_patterns_are_the_restated_rounding_of_the_fp32_result(dim, rowwise):
    rng = np.random.default_rng([5, dim, int(rowwise)])
    seed, step = 0xDEADBEEF12345, 3
    keys = np.array([(t << 40) | r for t in range(3) for r in range(1, ROWS, 2)] + [-1, (1 << 40) | 0, BIG], dtype=np.int64)
    keys = keys[rng.permutation(keys.size)]
    g = rng.standard_normal((keys.size, dim)).astype(np.float32) * 0.3
    t16, s16 = _fresh(dim, rowwise, True, 50 + dim)
    before = [_bits16(t) for t in t16]
    t32, s32 = [t.float() for t in t16], [s.clone() for s in s16]
    flags = NRX_ADAGRAD_ROWWISE if rowwise else 0
    kd, gd = torch.from_numpy(keys).to(DEV), torch.from_numpy(g).to(DEV)
    _call(t32, s32, dim, kd, gd, flags, decay=1e-3)
    _call(t16, s16, dim, kd, gd, flags | NRX_ADAGRAD_TABLE_BF16, decay=1e-3, seed=seed, step=step)
    cols = np.arange(dim)
    for t in range(3):
        assert _same_bits(s16[t], s32[t])                    # the state is the fp32 run's, bit for bit
        rows = np.arange(1, ROWS, 2)
        got = _bits16(t16[t])
        want = SR.sr_round(t32[t].cpu().numpy()[rows], SR.sr_bits(seed, step, t, rows, cols))
        assert SR.matches(got[rows], want), f"table {t}: bf16 patterns != (f32_bits(w_new) + bits16) >> 16"
        rest = np.ones(ROWS, bool)
        rest[rows] = False
        assert np.array_equal(got[rest], before[t][rest])
        assert not np.array_equal(got[rows], before[t][rows])


@pytest.mark.parametrize("rowwise", [True, False])
def test_bf16_arena_row_map_draws_the_full_tables_bits(rowwise):
    """row_mul / row_add of arena_row_map(1, 3): the arena of rank 1 at world 3, updated by its LOCAL rows, holds the patterns of the full table's
    rows 1::3 updated by their global rows."""
    rank, world, dim, R = 1, 3, 16, 100
    mul, add = shard_step.arena_row_map(rank, world)
    assert (mul, add) == (3, -2)
    gen = torch.Generator(device=DEV).manual_seed(6)
    full = [torch.randn(R, dim, device=DEV, generator=gen).to(torch.bfloat16) for _ in range(2)]
    arena = [shard_step.make_arena(R, dim, rank, world, DEV, full=f, dtype=torch.bfloat16) for f in full]
    local = torch.arange(1, arena[0].shape[0], device=DEV)            # arena row a >= 1 is global row (a - 1) * world + rank
    glob = (local - 1) * world + rank
    assert torch.equal(arena[0][local], full[0][glob])
    sf = [torch.rand((R,) if rowwise else (R, dim), device=DEV, generator=gen) for _ in range(2)]
    sa = [torch.zeros((a.shape[0],) if rowwise else tuple(a.shape), device=DEV) for a in arena]
    for a, f in zip(sa, sf):
        a[local] = f[glob]
    kf = torch.cat([(t << 40) | glob for t in range(2)])
    ka = torch.cat([(t << 40) | local for t in range(2)])
    g = torch.randn(kf.numel(), dim, device=DEV, generator=gen)
    flags = (NRX_ADAGRAD_ROWWISE if rowwise else 0) | NRX_ADAGRAD_TABLE_BF16
    arena_b, sa_b = [a.clone() for a in arena], [x.clone() for x in sa]
    _call(full, sf, dim, kf, g, flags, seed=99, step=2)
    _call(arena, sa, dim, ka, g, flags, seed=99, step=2, maps=[(mul, add)] * 2)
    _call(arena_b, sa_b, dim, ka, g, flags, seed=99, step=2)             # no map: the hash takes the arena's local rows
    for t in range(2):
        assert _same_bits(arena[t][local], full[t][glob])
        assert _same_bits(sa[t][local], sf[t][glob])
        assert not arena[t][0].any()
        assert _same_bits(sa_b[t], sa[t]) and not _same_bits(arena_b[t], arena[t])      # (so the test sees the map: same fp32 update, other bits)


# ------------------------------------------------------------------------------------------------ 6: two backward groups on one table
@pytest.mark.parametrize("rowwise", [True, False])
@pytest.mark.parametrize("pair_merge", [True, False])
def test_two_backward_groups_on_one_table_give_one_update_per_row(pair_merge, rowwise):
    """Two embed calls reading the SAME table in one step (DSSM's towers): one Adagrad update per row with the SUMMED gradient -- two updates would
    add the two squares separately and step twice."""
    lr, eps = 0.1, 1e-10
    g = torch.Generator(device=DEV).manual_seed(2)
    t0 = torch.randn(40, 16, device=DEV, generator=g)
    t1 = torch.randn(30, 16, device=DEV, generator=g)
    planA = ops.EmbedPlan([ops.Slot("x", NRX_SPARSE, 0, 16, 0, 0), ops.Slot("y", NRX_SPARSE, 1, 16, 0, 16)], out_width=32)
    planB = ops.EmbedPlan([ops.Slot("z", NRX_SPARSE, 0, 16, 0, 0)], out_width=16)
    ref = [t0.clone().requires_grad_(True), t1.clone().requires_grad_(True)]
    fus = [t0.clone().requires_grad_(True), t1.clone().requires_grad_(True)]
    w64 = [t0.double().cpu(), t1.double().cpu()]
    s64 = [torch.zeros(t.shape[0] if rowwise else tuple(t.shape), dtype=torch.float64) for t in (t0, t1)]
    sink = ops.SparseGradSink()
    opt = FusedSparseAdagrad(sink, lr=lr, eps=eps, rowwise=rowwise)
    opt.pair_merge = pair_merge              # True (default): nrx_rows_mark / nrx_rows_merge; False: the sort-based merge
    both = 0
    for _ in range(3):
        ia = [torch.randint(1, 40, (64,), device=DEV, generator=g), torch.randint(1, 30, (64,), device=DEV, generator=g)]
        ib = [torch.randint(1, 40, (64,), device=DEV, generator=g)]
        ua, ub = torch.randn(64, 32, device=DEV, generator=g), torch.randn(64, 16, device=DEV, generator=g)
        both += len(set(ia[0].tolist()) & set(ib[0].tolist()))
        for t in ref:
            t.grad = None
        loss = (ops.embed_apply(planA, ref, ia, [None, None], sparse_grad=True)[0] * ua).sum() + \
               (ops.embed_apply(planB, [ref[0]], ib, [None], sparse_grad=True)[0] * ub).sum()
        loss.backward()
        for t, w, s in zip(ref, w64, s64):   # the restatement on the COALESCED (summed) gradient
            rows, gr = _coo(t)
            rows, gr = rows.cpu(), gr.double().cpu()
            if rowwise:
                s[rows] += (gr * gr).mean(1)
                den = (s[rows].sqrt() + eps)[:, None]
            else:
                s[rows] += gr * gr
                den = s[rows].sqrt() + eps
            w[rows] -= lr * gr / den
        loss = (ops.embed_apply(planA, fus, ia, [None, None], sparse_grad=sink)[0] * ua).sum() + \
               (ops.embed_apply(planB, [fus[0]], ib, [None], sparse_grad=sink)[0] * ub).sum()
        loss.backward()
        assert len(sink.pending) == 2
        opt.step()
        assert all(int((m >= 0).sum()) == 0 for m in opt._maps)                   # the slot maps are clean between steps
    assert both > 20 and (len(opt._maps) > 0) == pair_merge
    for b, w, s in zip(fus, w64, s64):
        torch.testing.assert_close(b.detach().cpu().double(), w, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(opt.sums[opt._index[id(b)]].cpu().double(), s, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ 7: checkpoint
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["rowwise_adagrad", "adagrad"])
def test_checkpoint_resume_continues_bit_for_bit(name, bf16):
    """3 steps, save, load into a freshly built optimizer and model, 3 more steps == 6 uninterrupted steps: tables (bf16: the rounding stream goes on
    from the saved step count and seed), accumulators and the dense head."""
    plan, tables, batch = _setup(9, shared=True)
    if bf16:
        tables = [t.to(torch.bfloat16) for t in tables]
        plan = ops.EmbedPlan([dataclasses.replace(s, flags=s.flags | NRX_FEAT_TABLE_BF16) for s in plan.slots], out_width=plan.out_width)
    lin = torch.nn.Linear(56, 1).to(DEV)
    batches = [batch() for _ in range(6)]

    def build(tabs, lin_):
        sink = ops.SparseGradSink()
        ps = [t.clone().requires_grad_(True) for t in tabs]
        return ps, sink, SparseDenseAdam(ps, list(lin_.parameters()), lr=1e-2, fused_sink=sink, table_optimizer=name, table_lr=0.05, sr_seed=31)

    def run(ps, sink, opt, lin_, bs):
        for ins, ws, up in bs:
            opt.zero_grad()
            (lin_(ops.embed_apply(plan, ps, ins, ws, sparse_grad=sink)[0]) * up[:, :1]).sum().backward()
            opt.step()

    pa, sa, oa = build(tables, lin)
    run(pa, sa, oa, lin, batches[:3])
    sd = oa.state_dict()
    assert sd["sparse"]["t"] == 3 and sd["sparse"]["sr_seed"] == 31 and sorted(sd["sparse"]["tables"]) == [0, 1, 2] and sd["dense"]["state"]
    assert all(set(v) == {"sum"} for v in sd["sparse"]["tables"].values())
    sd = copy.deepcopy(sd)
    lin_b, lin_c = copy.deepcopy(lin), copy.deepcopy(lin)
    pb, sb, ob = build([p.detach() for p in pa], lin_b)          # restored
    ob.load_state_dict(sd)
    pc, sc, oc = build([p.detach() for p in pa], lin_c)          # weights only: the accumulators restart
    run(pa, sa, oa, lin, batches[3:])
    run(pb, sb, ob, lin_b, batches[3:])
    run(pc, sc, oc, lin_c, batches[3:])
    for a, b, c in zip(pa, pb, pc):
        assert _same_bits(a, b)
        assert not _same_bits(a, c)
    for k in range(3):
        ia, ib = oa._sparse._index[id(pa[k])], ob._sparse._index[id(pb[k])]
        assert _same_bits(oa._sparse.sums[ia], ob._sparse.sums[ib])
    assert oa._sparse.t == ob._sparse.t == 6
    assert torch.equal(lin.weight, lin_b.weight)


# ------------------------------------------------------------------------------------------------ 8, 9, 10: through the model classes
def _write_cfg(tmp_path, name, **emb):
    import os
    import yaml
    from tests.conftest import CONFIGS
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, name)))
    cfg["embeddings"].update(emb)
    cfg["train_hparams"]["lr_milestones"] = [2000, 5000]
    p = tmp_path / ("adagrad_" + "_".join(f"{k}-{v}" for k, v in sorted(emb.items())) + "_" + name)
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _bce_step(m, opt):
    def step(b):
        opt.zero_grad(set_to_none=False)
        loss = F.binary_cross_entropy(m(b).view(-1), b["label"][:, 0])
        loss.backward()
        opt.step()
        return loss
    return step


@pytest.mark.parametrize("bf16", [False, True])
def test_graphed_rowwise_adagrad_step_replays_like_eager(tmp_path, bf16):
    """GraphedStep(deterministic=True) over a small Deep model with table_optimizer: rowwise_adagrad: three replays == three eager steps, bit for bit
    (tables, accumulators, dense parameters, losses).  The step count of the rounding stream lives on the device: were it baked into the captured launch,
    the replays would round steps 3, 3, 3 where the eager loop rounds 3, 4, 5."""
    from news_recsys_amd.graph import GraphedStep
    from news_recsys_amd.model.sort.deep.model import Deep
    from tests.test_bf16_tables_gpu import make_batch
    emb = dict(table_optimizer="rowwise_adagrad", sparse_grad="fused")
    if bf16:
        emb.update(table_dtype="bf16", sr_seed=99)
    cfg = _write_cfg(tmp_path, "cf_deep_small.yaml", **emb)

    def build():
        torch.manual_seed(8)
        m = Deep(cfg).to(DEV)
        m._sparse_sink = ops.SparseGradSink()
        tabs = [e.weight for e in m.embedding_tables.values()]
        ids = {id(p) for p in tabs}
        opt = SparseDenseAdam(tabs, [p for p in m.parameters() if id(p) not in ids], lr=1e-2, fused_sink=m._sparse_sink, capturable=True, sr_seed=99,
                              table_optimizer=m.table_optimizer, table_lr=0.05)
        assert isinstance(opt._sparse, FusedSparseAdagrad) and opt._sparse.rowwise and opt._sparse.capturable
        return m, opt

    m_e, opt_e = build()
    m_g, opt_g = build()
    gen = torch.Generator(device=DEV).manual_seed(0)
    batches = [make_batch(m_e, 256, gen) for _ in range(4)]
    mode_before, sorted_before, wgrad_before = ops._INDEX_CHECK, ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED
    ops.set_index_check("off")
    try:
        # identical histories: GraphedStep runs its 2 warm-up steps eagerly on m_g (the capture itself only records), so m_e takes the same 2 first
        gs = GraphedStep(_bce_step(m_g, opt_g), batches[0], warmup=2, deterministic=True)
        assert int(opt_g._sparse._t_dev) == 2
        ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED = "det", True          # the eager loop in the modes the capture baked in
        step_e = _bce_step(m_e, opt_e)
        for _ in range(2):
            step_e(batches[0])
        before = [e.weight.detach().clone() for e in m_g.embedding_tables.values()]
        for b in batches[1:]:
            le, lg = step_e(b).item(), gs(b).item()
            assert le == lg, (le, lg)
        torch.cuda.synchronize()
    finally:
        ops.set_index_check(mode_before)
        ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED = sorted_before, wgrad_before
    assert int(opt_g._sparse._t_dev) == int(opt_e._sparse._t_dev) == 5          # the device count moved with every replay
    assert float(opt_g._sparse.lr_dev) == float(opt_e._sparse.lr_dev) == pytest.approx(0.05)
    for (k, p), q in zip(m_e.state_dict().items(), m_g.state_dict().values()):
        assert _same_bits(p, q), k
    for w, w0 in zip(m_g.embedding_tables.values(), before):
        assert w.weight.dtype is (torch.bfloat16 if bf16 else torch.float32) and not _same_bits(w.weight, w0)
    for e_, g_ in zip(m_e.embedding_tables.values(), m_g.embedding_tables.values()):
        se = opt_e._sparse.sums[opt_e._sparse._index[id(e_.weight)]]
        sg = opt_g._sparse.sums[opt_g._sparse._index[id(g_.weight)]]
        assert se.shape == (e_.weight.shape[0],) and _same_bits(se, sg) and bool(se.any())


@pytest.mark.parametrize("name", ["deep", "fm"])
def test_models_train_with_rowwise_adagrad(tmp_path, name):
    """`embeddings.table_optimizer: rowwise_adagrad` through a model class: configure_optimizers returns the composite optimizer, five steps on a repeated
    batch reduce the loss, the tables get no .grad."""
    from tests.test_bf16_tables_gpu import _model_classes, make_batch
    cls, cfg = _model_classes()[name]
    torch.manual_seed(0)
    m = cls(_write_cfg(tmp_path, cfg, table_optimizer="rowwise_adagrad", sparse_grad="fused", table_lr=0.05)).to(DEV)
    opt = m.configure_optimizers()["optimizer"]
    assert isinstance(opt._sparse, FusedSparseAdagrad) and opt._sparse.rowwise
    b = make_batch(m, 128, torch.Generator(device=DEV).manual_seed(1))
    before = {n: e.weight.detach().clone() for n, e in m.embedding_tables.items()}
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = F.binary_cross_entropy(m(b).view(-1), b["label"][:, 0])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    assert all(e.weight.grad is None for e in m.embedding_tables.values())
    assert all(not torch.equal(e.weight.detach(), before[n]) for n, e in m.embedding_tables.items())
    assert all(s.dim() == 1 for s in opt._sparse.sums) and len(opt._sparse.sums) == len(m.embedding_tables)
    with torch.no_grad():
        assert torch.isfinite(m(b)).all()


def _state_of(sp, weight):
    """The accumulator of the table stored at `weight` (the sharded step registers an arena by the tensor its bound step holds)."""
    hit = [i for i, t in enumerate(sp.tables) if t.data_ptr() == weight.data_ptr()]
    assert len(hit) == 1
    return sp.sums[hit[0]]


@pytest.mark.parametrize("bf16", [False, True])
def test_bound_sharded_model_at_world_1_leaves_the_unsharded_bits(tmp_path, bf16, monkeypatch):
    """shard_model_step_ at world 1 beside the unsharded fused model, both with table_optimizer: rowwise_adagrad, three steps on fresh batches (Deep on
    sparse features): arena rows 1.. hold the bits of the full table, the arenas' row-wise state [1 + local rows] the bits of the unsharded state; the
    dummy row 0 has no state.
    The unsharded model reduces its row gradients by the PLANNED reduction here (NRX_SPARSE_SMALL=0), the one the sharded step's owner runs: its
    (keys, values) are the sharded step's bit for bit ("Determinism and parity").  Left to itself a batch of 256 takes the one-launch form
    of small batches, which adds a row's 17 .. 32 upstream rows one after the other where the planned walk reduces a row of more than 16 by a
    wavefront tree: the same gradient to fp32 summation order, not to the bit (the 18-row tables of this config see ~15 lookups per row) -- which an
    fp32 table shows at once and a bf16 table only where a rounding flips."""
    from news_recsys_amd.model.sort.deep.model import Deep
    from tests.test_bf16_tables_gpu import make_batch
    monkeypatch.setattr(ops, "SPARSE_SMALL_DET", False)
    emb = dict(table_optimizer="rowwise_adagrad", sparse_grad="fused", table_lr=0.05)
    if bf16:
        emb.update(table_dtype="bf16", sr_seed=77)
    cfg = _write_cfg(tmp_path, "cf_deep_small.yaml", **emb)
    torch.manual_seed(0)
    ref = Deep(cfg).to(DEV)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    gen = torch.Generator(device=DEV).manual_seed(11)
    batches = [make_batch(ref, 256, gen) for _ in range(3)]
    shd = Deep(cfg).to(DEV)
    shd.load_state_dict(init)
    shard_step.shard_model_step_(shd, 0, 1, bf16_tables=bf16)
    opt_r, opt_s = ref.configure_optimizers()["optimizer"], shd.configure_optimizers()["optimizer"]
    assert isinstance(opt_s._sparse, FusedSparseAdagrad) and opt_s._sparse.rowwise
    if bf16:
        assert opt_s._sparse.row_maps == [shard_step.arena_row_map(0, 1)] * len(shd.embedding_tables)
    for m, opt in ((ref, opt_r), (shd, opt_s)):
        for b in batches:
            opt.zero_grad()
            F.binary_cross_entropy(m(b).view(-1), b["label"][:, 0]).backward()
            opt.step()
    assert opt_r._sparse.t == opt_s._sparse.t == 3
    for n, e in ref.embedding_tables.items():
        arena = shd.embedding_tables[n].weight
        assert arena.shape[0] == e.weight.shape[0] + 1 and arena.dtype is e.weight.dtype
        assert _same_bits(arena[1:], e.weight), n
        assert not _same_bits(e.weight, init[f"embedding_tables.{n}.weight"]), n
        s_r, s_s = _state_of(opt_r._sparse, e.weight), _state_of(opt_s._sparse, arena)
        assert s_s.shape == (arena.shape[0],) and s_r.shape == (e.weight.shape[0],)
        assert _same_bits(s_s[1:], s_r), n
        assert float(s_s[0]) == 0.0 and float(s_s[1]) == 0.0 and bool(s_r.any())
    for (k, p), q in zip(ref.state_dict().items(), shd.state_dict().values()):
        if not k.startswith("embedding_tables."):
            assert _same_bits(p, q), k
