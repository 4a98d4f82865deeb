"""Global-norm clipping of the row-sparse table gradients on the GPU (nrx_rows_sqnorm / nrx_rows_sqnorm_finish / nrx_rows_scale, the optimizers'
prepare / finish_norm / apply phases, train_hparams.max_grad_norm).

  the kernel alone    through ctypes on the hand-made key lists of tests/row_optim_ref.py: the 258 bins equal tests/grad_norm_ref.py WORD FOR WORD at
                      every lane-group width, in the scalar form, with rows that are not live poisoned by NaN; zero, denormal, overflowing and NaN rows
  order               a shuffled list, a list split over two calls and a buffer offset by 4 bytes leave the same words; the finish launch re-arms
  the scale launch    coef == 1 touches nothing; otherwise values * coef in fp32 bit for bit; nothing past n * dim moves
  against torch       ExactDenseAdamW / element-wise Adagrad with max_grad_norm beside torch's optimizers + torch.nn.utils.clip_grad_norm_
  and the optimizer classes through merging, bf16 tables, checkpoints, graph capture, the model classes and the bound sharded step at world 1.

Tolerances: rtol 2e-5 / atol 2e-6 are the ones tests/test_fused_sparse_adam_gpu.py uses for the unclipped comparison of an fp32 update with torch; the
norm against torch's (which sums in fp32) 1e-5 relative, against a float64 sum 1e-6 (one fp32 rounding per row, 6e-8); the finish launch's norm
within one unit in the last place of the double (its sqrt), its coefficient exactly the formula's float; everything called "the same" is compared
as integers."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from news_recsys_amd import _lib, ops, shard_step
from news_recsys_amd._lib import NRX_SPARSE
from news_recsys_amd.model.model_utils.optim import ExactDenseAdamW, FusedSparseAdagrad, FusedSparseAdam, SparseDenseAdam
from tests import grad_norm_ref as G
from tests.row_optim_ref import key_list, rows_for
from tests.test_fused_sparse_adam_gpu import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-5, 2e-6


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _sqnorm(keys, grads, n_tables, bins, n_dev=None, skip=0):
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device=DEV)
    ops.check(_lib.load().nrx_rows_sqnorm(keys.data_ptr(), grads.data_ptr(), keys.numel(), None if nd is None else nd.data_ptr(), n_tables,
                                          grads.shape[1], skip, bins.data_ptr(), _stream()), "nrx_rows_sqnorm")
    torch.cuda.synchronize()


def _finish(bins, max_norm, extra=None, rearm=0):
    norm = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    coef = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    ex = None if extra is None else torch.tensor([extra], dtype=torch.float64, device=DEV)
    ops.check(_lib.load().nrx_rows_sqnorm_finish(bins.data_ptr(), None if ex is None else ex.data_ptr(), max_norm, norm.data_ptr(), coef.data_ptr(),
                                                 rearm, _stream()), "nrx_rows_sqnorm_finish")
    torch.cuda.synchronize()
    return norm.item(), coef.cpu().numpy()[0]


def _new_bins():
    return torch.zeros(G.N_BINS, dtype=torch.int64, device=DEV)


def _words(bins):
    return bins.cpu().tolist()


def _grads(n, dim, rng):
    """Rows over forty binades, none of them zero."""
    return (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-14, 14, (n, 1)))).astype(np.float32)


def _check_finish(words, bins, max_norm, extra=None):
    want_norm, _ = G.finish(words, max_norm, extra)
    norm, coef = _finish(bins, max_norm, extra)
    assert abs(norm - want_norm) <= 2.0 ** -52 * want_norm, (norm, want_norm)
    assert coef == np.float32(min(1.0, max_norm / (norm + 1e-6)))
    return norm, coef


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 4099])
@pytest.mark.parametrize("dim", [1, 6, 8, 16, 32, 112, 320])
def test_bins_equal_the_restatement_word_for_word(dim, n):
    rng = np.random.default_rng([dim, n])
    keys, cnt = key_list(n, rng, rows=rows_for(n))
    g = _grads(n, dim, rng)
    live = np.array([G.is_live(k, 3) and (cnt is None or i < cnt) for i, k in enumerate(keys)])
    assert n < 3 or (live.any() and not live.all())
    poisoned = g.copy()
    poisoned[~live] = np.nan                                  # a row that is not live contributes nothing, whatever its values hold
    kd = torch.from_numpy(keys).to(DEV)
    want = G.bins_of(keys, g, 3, n_dev=cnt)
    for vals in (g, poisoned):
        bins = _new_bins()
        _sqnorm(kd, torch.from_numpy(vals).to(DEV), 3, bins, n_dev=cnt)
        assert _words(bins) == want
    assert want[0] == want[255] == want[256] == want[257] == 0 and (sum(want) > 0) == bool(live.any())
    if live.any():
        _check_finish(want, bins, 0.5 * G.finish(want, 1.0)[0])
    # a skipped table, and the list without the device-side count (its last entry is a real key)
    bins = _new_bins()
    _sqnorm(kd, torch.from_numpy(g).to(DEV), 3, bins, skip=1 << 1)
    assert _words(bins) == G.bins_of(keys, g, 3, skip_tables=1 << 1)
    if n >= 3:
        assert _words(bins) != want


@pytest.mark.parametrize("dim,n", [(16, 300001), (320, 17001)])
def test_more_rows_than_one_pass_of_the_bounded_grid(dim, n):
    """The grid is bounded (1024 blocks): past 262144 rows at dim 16 and 16384 at dim 320 a block walks several passes."""
    rng = np.random.default_rng(n)
    keys = ((np.arange(n) % 3) << 40 | (np.arange(n) + 1)).astype(np.int64)
    keys[::11] = -1
    keys[5::13] = G.BIG
    g = _grads(n, dim, rng)
    bins = _new_bins()
    _sqnorm(torch.from_numpy(keys).to(DEV), torch.from_numpy(g).to(DEV), 3, bins)
    want = G.bins_of(keys, g, 3)
    assert _words(bins) == want
    norm, _ = _check_finish(want, bins, 1.0)
    live = np.array([G.is_live(k, 3) for k in keys])
    exact = math.sqrt(math.fsum((g[live].astype(np.float64) ** 2).sum(1)))
    assert abs(norm - exact) <= 1e-6 * exact


@pytest.mark.parametrize("dim", [6, 8, 320])
def test_rows_at_the_edges_of_the_float_range(dim):
    keys = torch.arange(1, 9, dtype=torch.int64, device=DEV)
    g = np.zeros((8, dim), np.float32)
    g[1] = 1e-23                                              # the row's sum is a float denormal
    g[2, dim - 1] = 1e-20
    g[3] = 2.0
    want = G.bins_of(keys.cpu().numpy(), g, 1)
    assert want[1] > 0 and want[1] < 0x800000 * 2 and sum(want) == want[1] + want[G.row_word(g[3])[0]]
    bins = _new_bins()
    _sqnorm(keys, torch.from_numpy(g).to(DEV), 1, bins)
    assert _words(bins) == want
    _check_finish(want, bins, 1.0)
    # a row that overflows a float: counted as infinite, the norm is +inf, the coefficient 0
    g[5] = 3e19 if dim > 6 else 1e20
    want = G.bins_of(keys.cpu().numpy(), g, 1)
    assert want[256] == 1 and want[257] == 0
    bins = _new_bins()
    _sqnorm(keys, torch.from_numpy(g).to(DEV), 1, bins)
    assert _words(bins) == want
    norm, coef = _finish(bins, 1.0)
    assert norm == math.inf and coef == 0.0
    # a NaN element: counted, NaN out (as torch.nn.utils.clip_grad_norm_ leaves it)
    g[6, dim // 2] = np.nan
    want = G.bins_of(keys.cpu().numpy(), g, 1)
    assert want[256] == 1 and want[257] == 1
    bins = _new_bins()
    _sqnorm(keys, torch.from_numpy(g).to(DEV), 1, bins)
    assert _words(bins) == want
    norm, coef = _finish(bins, 1.0)
    assert math.isnan(norm) and math.isnan(coef)
    # the dense part: added after the bins; a NaN there is a NaN out
    bins = _new_bins()
    _sqnorm(keys[:5], torch.from_numpy(g[:5]).to(DEV), 1, bins)
    want = G.bins_of(keys[:5].cpu().numpy(), g[:5], 1)
    norm, coef = _check_finish(want, bins, 1.5, extra=7.25)
    assert norm == pytest.approx(math.sqrt(4.0 * dim + 7.25), rel=1e-12)
    norm, coef = _finish(bins, 1.5, extra=math.nan)
    assert math.isnan(norm) and math.isnan(coef)


# ------------------------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize("dim", [16, 112, 320])
def test_a_shuffled_a_split_and_a_misaligned_list_leave_the_same_words(dim):
    n = 1500
    rng = np.random.default_rng(dim)
    keys, _ = key_list(n, rng, rows=rows_for(n))
    g = _grads(n, dim, rng)
    want = G.bins_of(keys, g, 3)
    kd, gd = torch.from_numpy(keys).to(DEV), torch.from_numpy(g).to(DEV)
    bins = _new_bins()
    _sqnorm(kd, gd, 3, bins)
    assert _words(bins) == want
    p = torch.from_numpy(rng.permutation(n)).to(DEV)
    shuffled = _new_bins()
    _sqnorm(kd[p].contiguous(), gd[p].contiguous(), 3, shuffled)
    assert torch.equal(shuffled, bins)
    split = _new_bins()
    _sqnorm(kd[:613].contiguous(), gd[:613].contiguous(), 3, split)
    assert not torch.equal(split, bins)
    _sqnorm(kd[613:].contiguous(), gd[613:].contiguous(), 3, split)
    assert torch.equal(split, bins)
    # a buffer offset by 4 bytes: the element-by-element form, the same columns per lane
    buf = torch.zeros(n * dim + 1, dtype=torch.float32, device=DEV)
    off = buf[1:].view(n, dim)
    off.copy_(gd)
    assert off.data_ptr() % 16 == 4
    scalar = _new_bins()
    _sqnorm(kd, off, 3, scalar)
    assert torch.equal(scalar, bins)
    # the finish launch: rearm == 0 keeps the bins, rearm != 0 leaves zeros -- and the same results
    a = _finish(bins, 0.25, rearm=0)
    assert _words(bins) == want
    b = _finish(bins, 0.25, rearm=1)
    assert not bins.any() and a == b and a[1] < 1.0


# ------------------------------------------------------------------------------------------------ the scale launch
@pytest.mark.parametrize("n,dim,offset", [(5, 6, 0), (257, 16, 0), (257, 16, 1), (3, 7, 0), (270001, 16, 0)])
def test_scale_launch(n, dim, offset):
    """(257, 16, offset 1): the misaligned scalar form; (3, 7): a count that is no multiple of four; 270001 rows: past the bounded grid."""
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(n + dim)
    total, guard = n * dim, 64
    buf = torch.randn(offset + total + guard, device=DEV, generator=g)
    buf[offset + total:] = float("nan")                      # the tail is poisoned: nothing past n * dim may move (or be read into the result)
    vals = buf[offset:offset + total]
    before = buf.clone()
    coef = torch.ones(1, device=DEV)
    ops.check(lib.nrx_rows_scale(vals.data_ptr(), n, dim, coef.data_ptr(), _stream()), "nrx_rows_scale")
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))                      # coef == 1: untouched, bit for bit
    coef.fill_(0.37)
    ops.check(lib.nrx_rows_scale(vals.data_ptr(), n, dim, coef.data_ptr(), _stream()), "nrx_rows_scale")
    want = before.clone()
    want[offset:offset + total] = before[offset:offset + total] * coef
    assert torch.equal(buf.view(torch.int32), want.view(torch.int32))                        # one fp32 rounding per value; the rest as it was
    assert not torch.equal(buf[offset:offset + total], before[offset:offset + total])


def test_a_coefficient_of_one_reads_nothing():
    """coef == 1 on an all-NaN buffer with NaNs of several payloads: a pass that loaded and stored value * 1 could quieten or rewrite a payload."""
    n, dim = 64, 16
    bits = torch.full((n * dim,), 0x7FA00001, dtype=torch.int32, device=DEV)                 # signalling NaNs
    bits[::3] = -1
    before = bits.clone()
    coef = torch.ones(1, device=DEV)
    ops.check(_lib.load().nrx_rows_scale(bits.data_ptr(), n, dim, coef.data_ptr(), _stream()), "nrx_rows_scale")
    assert torch.equal(bits, before)


# ------------------------------------------------------------------------------------------------ against torch
def _two_tables(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    tabs = [torch.randn(60, 16, device=DEV, generator=g), torch.randn(45, 16, device=DEV, generator=g)]
    for t in tabs:
        t[0].zero_()
    plan = ops.EmbedPlan([ops.Slot("x", NRX_SPARSE, 0, 16, 0, 0), ops.Slot("y", NRX_SPARSE, 1, 16, 0, 16)], out_width=32)

    def batch():
        return ([torch.randint(0, 60, (96,), device=DEV, generator=g), torch.randint(0, 45, (96,), device=DEV, generator=g)],
                torch.randn(96, 1, device=DEV, generator=g))
    return plan, tabs, batch


@pytest.mark.parametrize("kind", ["exact", "adagrad"])
def test_clipped_step_matches_torch_with_clip_grad_norm(kind):
    """Three steps on two tables + one small nn.Linear: the reference is torch's optimizer on DENSE gradients after
    torch.nn.utils.clip_grad_norm_(all parameters, c).  Adam-type updates are nearly invariant to a gradient scale, so eps = 1 and a bound far
    below the norm: the clipped and the unclipped run then differ by more than 100x the tolerance -- asserted, a comparison that also passed without
    clipping would show nothing."""
    c, lr, tlr = 0.05, 0.03, 0.5
    plan, tabs, batch = _two_tables(3)
    lin0 = torch.nn.Linear(32, 1).to(DEV)
    batches = [batch() for _ in range(3)]

    def ours(max_norm):
        ps = [t.clone().requires_grad_(True) for t in tabs]
        lin = copy.deepcopy(lin0)
        sink = ops.SparseGradSink()
        kw = dict(exact=True) if kind == "exact" else dict(table_optimizer="adagrad", table_lr=tlr, adagrad_eps=1.0)
        opt = SparseDenseAdam(ps, list(lin.parameters()), lr=lr, eps=1.0, weight_decay=0.01, fused_sink=sink, max_grad_norm=max_norm, **kw)
        norms = []
        for ins, up in batches:
            opt.zero_grad()
            (lin(ops.embed_apply(plan, ps, ins, [None, None], sparse_grad=sink)[0]) * up).sum().backward()
            opt.step()
            norms.append(None if max_norm is None else opt.grad_norm.item())
        return ps, lin, norms, opt

    ref = [t.clone().requires_grad_(True) for t in tabs]
    lin_r = copy.deepcopy(lin0)
    if kind == "exact":
        opts = [torch.optim.AdamW(ref + list(lin_r.parameters()), lr=lr, eps=1.0, weight_decay=0.01)]
    else:
        opts = [torch.optim.Adagrad(ref, lr=tlr, lr_decay=0, eps=1.0, initial_accumulator_value=0),
                torch.optim.AdamW(lin_r.parameters(), lr=lr, eps=1.0, weight_decay=0.01)]
    ref_norms = []
    for ins, up in batches:
        for o in opts:
            o.zero_grad()
        (lin_r(ops.embed_apply(plan, ref, ins, [None, None])[0]) * up).sum().backward()
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_(ref + list(lin_r.parameters()), c)))
        for o in opts:
            o.step()
    ps, lin, norms, opt = ours(c)
    assert all(nr > 20 * c for nr in ref_norms)                                               # every step clips, hard
    for got, want in zip(norms, ref_norms):
        assert abs(got - want) <= 1e-5 * want                                                 # (torch sums in fp32)
    assert opt.clip_coef.item() == np.float32(c / (norms[-1] + 1e-6))
    for a, b in zip(ref + list(lin_r.parameters()), ps + list(lin.parameters())):
        torch.testing.assert_close(b.detach(), a.detach(), rtol=RTOL, atol=ATOL)
    # ... and the unclipped run is far away: the comparison above sees the clipping
    ups, ulin, _, _ = ours(None)
    for a, b in zip(ps + [lin.weight], ups + [ulin.weight]):
        gap = (a.detach() - b.detach()).abs().max().item()
        assert gap > 100 * (RTOL * a.detach().abs().max().item() + ATOL), gap


# ------------------------------------------------------------------------------------------------ the optimizer classes
def _i32(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype is torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype is b.dtype and torch.equal(_i32(a), _i32(b))


@pytest.mark.parametrize("pair_merge", [True, False])
def test_two_backward_groups_on_one_table_the_norm_is_the_merged_gradients(pair_merge):
    """Two embed calls read the SAME table in one step: the norm is taken after the merge -- the norm of the summed gradient (the coalesced COO
    gradient of the sparse_grad=True path, in float64), not of the two lists side by side.  The second call looks up the first call's ids of
    table 0 with the same upstream rows: the merged gradient of that table is TWICE either list's, its square four times one list's where the two
    lists side by side give two times -- the norm taken before the merge would be short by a factor between sqrt(2) and 1."""
    g = torch.Generator(device=DEV).manual_seed(2)
    t0 = torch.randn(40, 16, device=DEV, generator=g)
    t1 = torch.randn(30, 16, device=DEV, generator=g)
    planA = ops.EmbedPlan([ops.Slot("x", NRX_SPARSE, 0, 16, 0, 0), ops.Slot("y", NRX_SPARSE, 1, 16, 0, 16)], out_width=32)
    planB = ops.EmbedPlan([ops.Slot("z", NRX_SPARSE, 0, 16, 0, 0)], out_width=16)
    ref = [t0.clone().requires_grad_(True), t1.clone().requires_grad_(True)]
    fus = [t0.clone().requires_grad_(True), t1.clone().requires_grad_(True)]
    sink = ops.SparseGradSink()
    opt = FusedSparseAdam(sink, lr=0.05, max_grad_norm=0.5)
    opt.pair_merge = pair_merge
    ia = [torch.randint(1, 40, (64,), device=DEV, generator=g), torch.randint(1, 30, (64,), device=DEV, generator=g)]
    ib = [ia[0].clone()]
    ua = torch.randn(64, 32, device=DEV, generator=g)
    ub = ua[:, :16].clone()
    ((ops.embed_apply(planA, ref, ia, [None, None], sparse_grad=True)[0] * ua).sum() +
     (ops.embed_apply(planB, [ref[0]], ib, [None], sparse_grad=True)[0] * ub).sum()).backward()
    merged = math.sqrt(sum(float((t.grad.coalesce().values().double() ** 2).sum()) for t in ref))
    ((ops.embed_apply(planA, fus, ia, [None, None], sparse_grad=sink)[0] * ua).sum() +
     (ops.embed_apply(planB, [fus[0]], ib, [None], sparse_grad=sink)[0] * ub).sum()).backward()
    assert len(sink.pending) == 2
    apart = math.sqrt(sum(float((e["values"][:int(e["counts"][0])].double() ** 2).sum()) if not e.get("filler") else
                          float((e["values"][e["uniq"] >= 0].double() ** 2).sum()) for e in sink.pending))
    assert apart < 0.95 * merged                              # (table 0 carries about half of the squared norm: sqrt(3 / 4) = 0.87)
    opt.step()
    assert abs(opt.grad_norm.item() - merged) <= 1e-6 * merged
    assert opt.clip_coef.item() == np.float32(0.5 / (opt.grad_norm.item() + 1e-6)) and not sink.pending


def _entry(tabs, dim, keys, values):
    return dict(tables=tabs, dim=dim, uniq=keys.clone(), values=values.clone(), counts=torch.tensor([keys.numel()], device=DEV), cap=keys.numel())


def _hand_made(seed, bf16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    tabs = [torch.randn(50, 16, device=DEV, generator=g), torch.randn(33, 16, device=DEV, generator=g)]
    if bf16:
        tabs = [t.to(torch.bfloat16) for t in tabs]
    keys = torch.cat([torch.arange(0, 50, 2, device=DEV), (1 << 40) | torch.arange(1, 33, 3, device=DEV)])
    vals = torch.randn(keys.numel(), 16, device=DEV, generator=g)
    return tabs, keys, vals


@pytest.mark.parametrize("cls", [FusedSparseAdam, FusedSparseAdagrad, ExactDenseAdamW])
def test_a_norm_below_the_bound_leaves_the_unclipped_step(cls):
    tabs, keys, vals = _hand_made(4, False)
    out = []
    for bound in (None, 1e6):
        ps = [t.clone() for t in tabs]
        sink = ops.SparseGradSink()
        opt = cls(sink, ps, max_grad_norm=bound) if cls is ExactDenseAdamW else cls(sink, lr=0.05, max_grad_norm=bound)
        for _ in range(2):
            sink.pending.append(_entry(ps, 16, keys, vals))
            opt.step()
        out.append(ps)
    assert opt.clip_coef.item() == 1.0 and opt.grad_norm.item() > 1.0
    for a, b, t in zip(out[0], out[1], tabs):
        assert _same_bits(a, b) and not _same_bits(a, t)


@pytest.mark.parametrize("cls", [FusedSparseAdam, FusedSparseAdagrad])
def test_bf16_tables_step_like_the_unclipped_optimizer_fed_the_scaled_values(cls):
    tabs, keys, vals = _hand_made(6, True)
    pa, pb = [t.clone() for t in tabs], [t.clone() for t in tabs]
    sa, sb = ops.SparseGradSink(), ops.SparseGradSink()
    oa = cls(sa, lr=0.05, params=pa, sr_seed=12, max_grad_norm=0.3)
    ob = cls(sb, lr=0.05, params=pb, sr_seed=12)
    for it in range(2):
        v = vals * (1.0 + it)
        sa.pending.append(_entry(pa, 16, keys, v))
        oa.step()
        coef = oa.clip_coef.clone()
        assert 0.0 < coef.item() < 0.1
        sb.pending.append(_entry(pb, 16, keys, v * coef))                 # one fp32 rounding per value, as the scale launch
        ob.step()
    live = math.sqrt(float((v[keys != 0].double() ** 2).sum()))            # (key 0 is table 0's padding row)
    assert abs(oa.grad_norm.item() - live) <= 1e-6 * live
    for a, b, t in zip(pa, pb, tabs):
        assert a.dtype is torch.bfloat16 and _same_bits(a, b) and not _same_bits(a, t)


@pytest.mark.parametrize("kind", ["adam", "rowwise_adagrad", "exact"])
def test_checkpoint_resume_continues_bit_for_bit(kind):
    plan, tables, batch = _setup(9, shared=True)
    lin = torch.nn.Linear(56, 1).to(DEV)
    batches = [batch() for _ in range(6)]
    kw = dict(exact=True) if kind == "exact" else dict(table_optimizer=kind, table_lr=0.05)

    def build(tabs, lin_):
        sink = ops.SparseGradSink()
        ps = [t.clone().requires_grad_(True) for t in tabs]
        return ps, sink, SparseDenseAdam(ps, list(lin_.parameters()), lr=1e-2, fused_sink=sink, max_grad_norm=0.2, **kw)

    def run(ps, sink, opt, lin_, bs):
        for ins, ws, up in bs:
            opt.zero_grad()
            (lin_(ops.embed_apply(plan, ps, ins, ws, sparse_grad=sink)[0]) * up[:, :1]).sum().backward()
            opt.step()
            assert opt.clip_coef.item() < 1.0

    pa, sa, oa = build(tables, lin)
    run(pa, sa, oa, lin, batches[:3])
    sd = copy.deepcopy(oa.state_dict())
    lin_b = copy.deepcopy(lin)
    pb, sb, ob = build([p.detach() for p in pa], lin_b)
    ob.load_state_dict(sd)
    run(pa, sa, oa, lin, batches[3:])
    run(pb, sb, ob, lin_b, batches[3:])
    for a, b in zip(pa, pb):
        assert _same_bits(a, b)
    assert torch.equal(lin.weight, lin_b.weight) and oa._sparse.t == ob._sparse.t == 6
    assert torch.equal(oa.grad_norm, ob.grad_norm) and torch.equal(oa.clip_coef, ob.clip_coef)


# ------------------------------------------------------------------------------------------------ through the model classes
def _write_cfg(tmp_path, name, hp=None, **emb):
    import os
    import yaml
    from tests.conftest import CONFIGS
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, name)))
    cfg["embeddings"].update(emb)
    cfg["train_hparams"]["lr_milestones"] = [2000, 5000]
    cfg["train_hparams"].update(hp or {})
    p = tmp_path / ("clip_" + "_".join(f"{k}-{v}" for k, v in sorted(emb.items())) + "_" + name)
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


@pytest.mark.parametrize("table_optimizer", ["adam", "rowwise_adagrad"])
def test_graphed_clipped_step_replays_like_eager(tmp_path, table_optimizer):
    """GraphedStep(deterministic=True) over a small Deep model with a bound: three replays == three eager steps bit for bit (parameters, losses, norm
    and coefficient).  The bins are re-armed by the finish launch: were they not, the second replay would add to the first one's words."""
    from news_recsys_amd.graph import GraphedStep
    from news_recsys_amd.model.sort.deep.model import Deep
    from tests.test_bf16_tables_gpu import make_batch
    cfg = _write_cfg(tmp_path, "cf_deep_small.yaml", table_optimizer=table_optimizer, sparse_grad="fused")

    def build():
        torch.manual_seed(8)
        m = Deep(cfg).to(DEV)
        m._sparse_sink = ops.SparseGradSink()
        tabs = [e.weight for e in m.embedding_tables.values()]
        ids = {id(p) for p in tabs}
        opt = SparseDenseAdam(tabs, [p for p in m.parameters() if id(p) not in ids], lr=1e-2, fused_sink=m._sparse_sink, capturable=True,
                              table_optimizer=table_optimizer, table_lr=0.05, max_grad_norm=1e-3)
        return m, opt

    m_e, opt_e = build()
    m_g, opt_g = build()
    gen = torch.Generator(device=DEV).manual_seed(0)
    batches = [make_batch(m_e, 256, gen) for _ in range(4)]
    mode_before, sorted_before, wgrad_before = ops._INDEX_CHECK, ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED
    ops.set_index_check("off")
    try:
        gs = GraphedStep(_bce_step(m_g, opt_g), batches[0], warmup=2, deterministic=True)
        ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED = "det", True          # the eager loop in the modes the capture baked in
        step_e = _bce_step(m_e, opt_e)
        for _ in range(2):
            step_e(batches[0])
        seen = []
        for b in batches[1:]:
            le, lg = step_e(b).item(), gs(b).item()
            assert le == lg, (le, lg)
            assert torch.equal(opt_e.grad_norm, opt_g.grad_norm) and torch.equal(opt_e.clip_coef, opt_g.clip_coef)
            seen.append(opt_g.grad_norm.item())
        torch.cuda.synchronize()
    finally:
        ops.set_index_check(mode_before)
        ops.DENSE_BWD_SORTED, ops.WGRAD_ORDERED = sorted_before, wgrad_before
    assert len(set(seen)) == 3 and all(1e-3 < x < 100 for x in seen) and opt_g.clip_coef.item() < 1.0
    assert not opt_g._sparse._norm_bins.any()
    for (k, p), q in zip(m_e.state_dict().items(), m_g.state_dict().values()):
        assert _same_bits(p, q), k


def test_a_captured_clipped_step_over_several_ranks_is_refused(monkeypatch):
    """The all-reduce of the bins is not captured: finish_norm() with a norm_group refuses while the stream is capturing (before it calls anything)."""
    tabs, keys, vals = _hand_made(4, False)
    sink = ops.SparseGradSink()
    opt = FusedSparseAdam(sink, lr=0.05, max_grad_norm=1.0, norm_group=object(), capturable=True)
    sink.pending.append(_entry(tabs, 16, keys, vals))
    opt.prepare()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        opt.finish_norm()


@pytest.mark.parametrize("name", ["deep", "fm"])
def test_models_train_with_the_config_key(tmp_path, name):
    from tests.test_bf16_tables_gpu import _model_classes, make_batch
    cls, cfg = _model_classes()[name]
    torch.manual_seed(0)
    m = cls(_write_cfg(tmp_path, cfg, hp=dict(max_grad_norm=1e-3), sparse_grad="fused")).to(DEV)
    opt = m.configure_optimizers()["optimizer"]
    assert opt.max_grad_norm == 1e-3
    b = make_batch(m, 128, torch.Generator(device=DEV).manual_seed(1))
    before = {n: e.weight.detach().clone() for n, e in m.embedding_tables.items()}
    losses, norms = [], []
    for _ in range(5):
        opt.zero_grad()
        loss = F.binary_cross_entropy(m(b).view(-1), b["label"][:, 0])
        loss.backward()
        # the float64 norm of everything the step is about to clip: the sink's live rows and the dense .grads
        sq = sum(float((p.grad.double() ** 2).sum()) for p in m.parameters() if p.grad is not None)
        for e in m._sparse_sink.pending:
            k = e["uniq"]
            ok = (k >= 0) & ((k & ((1 << 40) - 1)) != 0)
            if not e.get("filler"):
                ok &= torch.arange(k.numel(), device=k.device) < e["counts"][0]
            sq += float((e["values"][ok].double() ** 2).sum())
        opt.step()
        assert abs(opt.grad_norm.item() - math.sqrt(sq)) <= 1e-5 * math.sqrt(sq)
        assert opt.clip_coef.item() == np.float32(min(1.0, 1e-3 / (opt.grad_norm.item() + 1e-6)))
        losses.append(loss.item())
        norms.append(opt.grad_norm.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(x > 1e-3 for x in norms), norms
    assert all(e.weight.grad is None for e in m.embedding_tables.values())
    assert all(not torch.equal(e.weight.detach(), before[n]) for n, e in m.embedding_tables.items())


def test_bound_sharded_model_at_world_1_leaves_the_unsharded_clipped_bits(tmp_path, monkeypatch):
    """shard_model_step_ at world 1 beside the unsharded fused model, both with train_hparams.max_grad_norm and row-wise Adagrad, three steps on fresh
    batches: the same norm and coefficient bits, arena rows 1.. hold the bits of the full table, the dense parameters are the same bits.  (The
    unsharded model takes the planned reduction, the one the sharded step's owner runs: tests/test_sparse_adagrad_gpu.py says why.)"""
    from news_recsys_amd.model.sort.deep.model import Deep
    from tests.test_bf16_tables_gpu import make_batch
    monkeypatch.setattr(ops, "SPARSE_SMALL_DET", False)
    cfg = _write_cfg(tmp_path, "cf_deep_small.yaml", hp=dict(max_grad_norm=1e-3), table_optimizer="rowwise_adagrad", sparse_grad="fused", table_lr=0.05)
    torch.manual_seed(0)
    ref = Deep(cfg).to(DEV)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    gen = torch.Generator(device=DEV).manual_seed(11)
    batches = [make_batch(ref, 256, gen) for _ in range(3)]
    shd = Deep(cfg).to(DEV)
    shd.load_state_dict(init)
    shard_step.shard_model_step_(shd, 0, 1)
    opt_r, opt_s = ref.configure_optimizers()["optimizer"], shd.configure_optimizers()["optimizer"]
    assert opt_s.max_grad_norm == 1e-3 and opt_s._sparse.norm_group is None and opt_s._sparse.norm_skip is None        # world 1: nothing to reduce
    seen = {}
    for m, opt in ((ref, opt_r), (shd, opt_s)):
        for b in batches:
            opt.zero_grad()
            F.binary_cross_entropy(m(b).view(-1), b["label"][:, 0]).backward()
            opt.step()
            seen.setdefault(id(opt), []).append((opt.grad_norm.clone(), opt.clip_coef.clone()))
    for (nr, cr), (ns, cs) in zip(seen[id(opt_r)], seen[id(opt_s)]):
        assert torch.equal(nr, ns) and torch.equal(cr, cs) and cr.item() < 1.0
    for n, e in ref.embedding_tables.items():
        arena = shd.embedding_tables[n].weight
        assert _same_bits(arena[1:], e.weight), n
        assert not _same_bits(e.weight, init[f"embedding_tables.{n}.weight"]), n
    for (k, p), q in zip(ref.state_dict().items(), shd.state_dict().values()):
        if not k.startswith("embedding_tables."):
            assert _same_bits(p, q), k
