"""In-batch softmax loss on the GPU (nrx_inbatch_softmax_fwd / _bwd, ops.inbatch_softmax, DSSM `negatives: in_batch`) against the float64
restatement in tests/inbatch_softmax_ref.py on the same fp32 inputs.

Tolerances are derived, not tuned (tests/inbatch_softmax_ref.py): with E_s = (d + 2) 2^-24 max|U_i| max|V_j| inv_t the error of a score,
a row loss may be off by 4 E_s + 8 2^-24 max(1, |lse_i|, |s_ii|) and a gradient element by 4 (2 E_s + 16 2^-24) (sum of the |terms| it is made of)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.recall.DSSM.model import DSSM
from tests.conftest import CONFIGS, GOLDEN
from tests.inbatch_softmax_ref import grad_tolerance, inbatch_softmax_ref, loss_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_B = (1, 2, 31, 32, 33, 64, 65)
LARGE_B = (257, 1000, 4101)
DIMS = (4, 8, 12, 16, 32, 64)
SPLITS = (1, 3, 0)


@functools.lru_cache(maxsize=None)
def _case(B, d, ids_kind, scale=None, temperature=0.1, seed=0):
    """Inputs (CPU, fp32) and the float64 reference of one case, computed once and shared by the tests (read only)."""
    gen = torch.Generator().manual_seed(1000 * B + 10 * d + seed)
    u = torch.randn(B, d, generator=gen)
    v = torch.randn(B, d, generator=gen)
    if scale is None:
        u, v = F.normalize(u, p=2, dim=1), F.normalize(v, p=2, dim=1)
    else:
        u, v = u * scale, v * scale
    ids = None
    if ids_kind is not None:
        ids = torch.randint(0, max(2, B // 4), (B,), generator=gen).to(torch.int32 if ids_kind == 32 else torch.int64)
        ids = ids + (0 if ids_kind == 32 else (1 << 33))          # int64 ids beyond 32 bits, equal in their low words only where truly equal
    g = torch.randn(B, generator=gen)
    g[::3] = 0.0
    g[1::5] = -g[1::5].abs()
    ref = inbatch_softmax_ref(u.numpy(), v.numpy(), np.float32(1.0 / temperature), ids=None if ids is None else ids.numpy(), g=g.numpy())
    return u, v, ids, g, ref


def _strided(t, pad=4):
    """The same values as rows of a wider buffer (ld = d + pad) whose other columns are NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _run(u, v, ids, g, temperature, col_splits, strided):
    ud = (_strided(u.to(DEV)) if strided else u.to(DEV)).requires_grad_(True)
    vd = (_strided(v.to(DEV)) if strided else v.to(DEV)).requires_grad_(True)
    loss = ops.inbatch_softmax(ud, vd, temperature=temperature, item_ids=None if ids is None else ids.to(DEV), col_splits=col_splits)
    gu, gv = torch.autograd.grad(loss, (ud, vd), g.to(DEV))
    return loss.detach(), gu, gv


def _check(B, d, ids_kind, col_splits, strided, **kw):
    u, v, ids, g, ref = _case(B, d, ids_kind, **kw)
    loss, gu, gv = _run(u, v, ids, g, kw.get("temperature", 0.1), col_splits, strided)
    what = f"B={B} d={d} ids={ids_kind} splits={col_splits} strided={strided}"
    loss, gu, gv = loss.cpu().numpy().astype(np.float64), gu.cpu().numpy().astype(np.float64), gv.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(gu).all() and np.isfinite(gv).all(), what
    el = np.abs(loss - ref.loss) - loss_tolerance(ref, d)
    tu, tv = grad_tolerance(ref, d)
    eu, ev = np.abs(gu - ref.dU) - tu, np.abs(gv - ref.dV) - tv
    assert el.max() <= 0, f"{what}: row loss off by {np.abs(loss - ref.loss).max():.3e} (bound {loss_tolerance(ref, d).min():.3e}..)"
    assert eu.max() <= 0, f"{what}: dU off by {np.abs(gu - ref.dU).max():.3e}, {int((eu > 0).sum())} elements beyond the bound"
    assert ev.max() <= 0, f"{what}: dV off by {np.abs(gv - ref.dV).max():.3e}, {int((ev > 0).sum())} elements beyond the bound"


@pytest.mark.parametrize("d", DIMS)
def test_small_batches_every_dim_match_float64(d):
    """Every B around the 32-row groups, with and without ids (int32, int64), each split form, contiguous and strided (ld = d + 4)."""
    for B in SMALL_B:
        for ids_kind in (None, 32, 64):
            for col_splits in SPLITS:
                _check(B, d, ids_kind, col_splits, strided=(B + (ids_kind or 0) // 32 + col_splits) % 2 == 0)


@pytest.mark.parametrize("B", LARGE_B)
def test_larger_batches_match_float64(B):
    """More than one block per side, more than one tile per split, a tail tile (257, 1000 and 4101 are no multiples of 32)."""
    for ids_kind in (None, 32, 64):
        for col_splits in SPLITS:
            _check(B, 16, ids_kind, col_splits, strided=ids_kind == 32)


@pytest.mark.parametrize("col_splits", SPLITS)
def test_scores_around_1e4_stay_finite_and_within_tolerance(col_splits):
    """Unnormalised rows scaled by 3 at temperature 0.01: |s| reaches 1e4, where exp(s) without the running maximum overflows."""
    u, v, _, _, ref = _case(257, 16, 64, scale=3.0, temperature=0.01)
    assert np.abs(ref.diag).max() > 3e3 and np.abs(ref.lse).max() > 3e3
    _check(257, 16, 64, col_splits, strided=False, scale=3.0, temperature=0.01)
    _check(257, 16, None, col_splits, strided=True, scale=3.0, temperature=0.01)


@pytest.mark.parametrize("col_splits", (1, 3))
def test_rows_whose_every_other_column_is_excluded_are_exactly_zero(col_splits):
    """Four rows with one id: only the diagonal is kept, and its score is one value used twice -- loss 0.0 and gradients 0.0, bit for bit."""
    u, v, _, _, _ = _case(4, 16, None)
    ids = torch.full((4,), 7, dtype=torch.int64)
    loss, gu, gv = _run(u, v, ids, torch.tensor([1.0, -2.0, 0.5, 3.0]), 0.1, col_splits, strided=False)
    assert torch.all(loss == 0.0) and torch.all(gu == 0.0) and torch.all(gv == 0.0)
    # ... and over several tiles, waves and splits: 130 rows with one id
    u, v, _, g, _ = _case(130, 16, 64)
    loss, gu, gv = _run(u, v, torch.full((130,), -5, dtype=torch.int64), g, 0.1, col_splits, strided=True)
    assert torch.all(loss == 0.0) and torch.all(gu == 0.0) and torch.all(gv == 0.0)


def test_a_batch_of_one_has_loss_zero():
    for d in (4, 16, 64):
        u, v, _, _, _ = _case(1, d, None)
        loss, gu, gv = _run(u, v, None, torch.ones(1), 0.1, 0, strided=False)
        assert loss.item() == 0.0 and torch.all(gu == 0.0) and torch.all(gv == 0.0)
    assert ops.inbatch_softmax(torch.zeros(0, 16, device=DEV), torch.zeros(0, 16, device=DEV)).shape == (0,)


def test_dims_outside_the_kernels_raise_the_librarys_own_codes():
    """The op forwards the entry point's status: a multiple of 4 in 65..128 is a valid shape without a kernel, anything else a bad argument."""
    with pytest.raises(_lib.NrxError, match="dim=96"):
        ops.inbatch_softmax(torch.zeros(8, 96, device=DEV), torch.zeros(8, 96, device=DEV))
    with pytest.raises(ValueError, match="dim 6"):
        ops.inbatch_softmax(torch.zeros(8, 6, device=DEV), torch.zeros(8, 6, device=DEV))


def test_either_side_may_need_no_gradient():
    u, v, ids, g, ref = _case(65, 16, 64)
    tu, tv = grad_tolerance(ref, 16)
    ud, vd = u.to(DEV).requires_grad_(True), v.to(DEV)
    (gu,) = torch.autograd.grad(ops.inbatch_softmax(ud, vd, item_ids=ids.to(DEV)), (ud,), g.to(DEV))
    assert np.all(np.abs(gu.cpu().numpy() - ref.dU) <= tu)
    ud, vd = u.to(DEV), v.to(DEV).requires_grad_(True)
    (gv,) = torch.autograd.grad(ops.inbatch_softmax(ud, vd, item_ids=ids.to(DEV)), (vd,), g.to(DEV))
    assert np.all(np.abs(gv.cpu().numpy() - ref.dV) <= tv)


@pytest.mark.parametrize("B,d,col_splits", [(33, 4, 1), (33, 16, 3), (257, 16, 0), (70, 4, 3)])
def test_nothing_is_read_or_written_past_the_ends(B, d, col_splits):
    """u, v, ids and every output are the heads of larger buffers that hold NaN / -1 beyond the end (and in the padding columns of the
    strided rows): nothing outside the outputs changes and no NaN comes in."""
    lib = _lib.load()
    u, v, ids, g, ref = _case(B, d, 64)
    ld, extra = d + 4, 97
    ub = torch.full(((B + extra), ld), float("nan"), device=DEV)
    vb = torch.full(((B + extra), ld), float("nan"), device=DEV)
    ub[:B, :d] = u.to(DEV)
    vb[:B, :d] = v.to(DEV)
    idb = torch.full((B + extra,), -1, dtype=torch.int64, device=DEV)
    idb[:B] = ids.to(DEV)
    gb = torch.full((B + extra,), float("nan"), device=DEV)
    gb[:B] = g.to(DEV)
    loss = torch.full((B + extra,), float("nan"), device=DEV)
    lse = torch.full((B + extra,), float("nan"), device=DEV)
    gu = torch.full(((B + extra), ld), float("nan"), device=DEV)
    gv = torch.full(((B + extra), ld), float("nan"), device=DEV)
    ws = torch.full((lib.nrx_inbatch_softmax_workspace(B, d, col_splits),), 0xFF, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.nrx_inbatch_softmax_fwd(ub.data_ptr(), ld, vb.data_ptr(), ld, B, d, 10.0, idb.data_ptr(), 64, col_splits, loss.data_ptr(),
                                           lse.data_ptr(), ws.data_ptr(), st), "fwd")
    ws.fill_(0xFF)
    _lib.check(lib.nrx_inbatch_softmax_bwd(ub.data_ptr(), ld, vb.data_ptr(), ld, B, d, 10.0, idb.data_ptr(), 64, col_splits, lse.data_ptr(),
                                           gb.data_ptr(), gu.data_ptr(), ld, gv.data_ptr(), ld, ws.data_ptr(), st), "bwd")
    torch.cuda.synchronize()
    for t in (loss, lse):
        assert torch.isfinite(t[:B]).all() and torch.isnan(t[B:]).all()
    for t in (gu, gv):
        assert torch.isfinite(t[:B, :d]).all() and torch.isnan(t[:B, d:]).all() and torch.isnan(t[B:]).all()
    assert torch.isnan(ub[:B, d:]).all() and torch.isnan(ub[B:]).all() and torch.equal(ub[:B, :d].cpu(), u) and torch.all(idb[B:] == -1)
    assert np.all(np.abs(loss[:B].cpu().numpy() - ref.loss) <= loss_tolerance(ref, d))
    tu, tv = grad_tolerance(ref, d)
    assert np.all(np.abs(gu[:B, :d].cpu().numpy() - ref.dU) <= tu) and np.all(np.abs(gv[:B, :d].cpu().numpy() - ref.dV) <= tv)


@pytest.mark.parametrize("B,col_splits", [(1000, 0), (1000, 3), (4101, 0)])
def test_two_calls_give_the_same_bits(B, col_splits):
    u, v, ids, g, _ = _case(B, 16, 32)
    a = _run(u, v, ids, g, 0.1, col_splits, strided=False)
    b = _run(u, v, ids, g, 0.1, col_splits, strided=False)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_forward_and_backward_need_no_b_by_b_buffer():
    """At B = 8192 the peak of forward + backward stays below an eighth of ONE [B, B] fp32 matrix (the materialised form holds several)."""
    B, d = 8192, 16
    gen = torch.Generator(device=DEV).manual_seed(5)
    u = F.normalize(torch.randn(B, d, device=DEV, generator=gen), dim=1).requires_grad_(True)
    v = F.normalize(torch.randn(B, d, device=DEV, generator=gen), dim=1).requires_grad_(True)
    ids = torch.randint(0, B // 4, (B,), device=DEV, generator=gen)
    g = torch.randn(B, device=DEV, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = ops.inbatch_softmax(u, v, item_ids=ids)
    gu, gv = torch.autograd.grad(loss, (u, v), g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < B * B * 4 // 8, rise
    assert torch.isfinite(loss).all() and torch.isfinite(gu).all() and torch.isfinite(gv).all()
    # (a row loss lies in [0, log B + 2 / temperature] for unit rows)
    assert float(loss.detach().min()) >= 0.0 and float(loss.detach().max()) < np.log(B) + 2.0 / 0.1


def test_one_capture_of_forward_and_backward_replays_to_the_eager_bits():
    u, v, ids, g, _ = _case(1000, 16, 64)
    ud, vd = u.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    idd, gd = ids.to(DEV), g.to(DEV)

    def step():
        loss = ops.inbatch_softmax(ud, vd, temperature=0.1, item_ids=idd)
        return (loss,) + torch.autograd.grad(loss, (ud, vd), gd)

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
    for x, y in zip(outs, want):
        assert torch.equal(x.detach().view(torch.int32), y.view(torch.int32))


def _torch_in_batch_loss(u, v, temperature, mask, ids):
    s = u @ v.t() / temperature
    if ids is not None:
        excl = (ids[:, None] == ids[None, :]) & ~torch.eye(u.shape[0], dtype=torch.bool, device=u.device)
        s = s.masked_fill(excl, float("-inf"))
    rows = torch.logsumexp(s, dim=1) - (u * v).sum(dim=1) / temperature
    return (rows * mask).mean()


@pytest.mark.parametrize("mask_same", [True, False])
def test_dssm_in_batch_training_step_matches_a_torch_restatement(mask_same):
    g = dict(np.load(os.path.join(GOLDEN, "model_dssm.npz"), allow_pickle=False))
    hp = {"negatives": "in_batch", "in_batch_mask_same_item": mask_same, "item_id_feature": "item_id", "temperature": 0.2,
          "lr": 1e-3, "min_lr": 1e-5, "lr_milestones": [4, 20]}
    m = DSSM(os.path.join(CONFIGS, "cf_dssm_small.yaml"), hparams=hp)
    m.load_state_dict({k[len("param/"):]: torch.from_numpy(val) for k, val in g.items() if k.startswith("param/")}, strict=True)
    m = m.to(DEV)
    batch = {k[len("batch/"):]: torch.from_numpy(val).to(DEV) for k, val in g.items() if k.startswith("batch/")}
    batch["item_id"][5] = batch["item_id"][2]                 # at least one pair of rows with the same item
    out = m(batch)
    assert len(out) == 3 and out[2] is None                  # the three-tuple stays; there is nothing to sample
    loss = m.training_step(batch, 0)
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert all(p.grad is not None for p in m.parameters())
    m.zero_grad(set_to_none=True)
    u, v, _ = m(batch)
    want_loss = _torch_in_batch_loss(u, v, 0.2, batch["label"][:, 1], batch["item_id"] if mask_same else None)
    want_loss.backward()
    np.testing.assert_allclose(loss.item(), want_loss.item(), rtol=1e-5)
    for k, p in m.named_parameters():
        want = p.grad.cpu().numpy()
        np.testing.assert_allclose(got[k].cpu().numpy(), want, rtol=2e-3, atol=2e-6 + 1e-4 * np.abs(want).max(), err_msg=k)
    if mask_same:
        del batch["item_id"]
        with pytest.raises(KeyError, match="in_batch_mask_same_item"):
            m.training_step(batch, 0)


def test_dssm_sampled_default_is_untouched_by_the_new_hparams():
    """The default draws its permutations and returns the [B, n_neg, 16] negatives as before."""
    g = dict(np.load(os.path.join(GOLDEN, "model_dssm.npz"), allow_pickle=False))
    m = DSSM(os.path.join(CONFIGS, "cf_dssm_small.yaml"), hparams={"negative_sample_rate": 3, "lr": 1e-3, "min_lr": 1e-5, "lr_milestones": [4, 20]})
    m.load_state_dict({k[len("param/"):]: torch.from_numpy(val) for k, val in g.items() if k.startswith("param/")}, strict=True)
    m = m.to(DEV)
    batch = {k[len("batch/"):]: torch.from_numpy(val).to(DEV) for k, val in g.items() if k.startswith("batch/")}
    u, i, n = m(batch, perms=torch.from_numpy(g["out/perms"]))
    np.testing.assert_allclose(n.detach().cpu().numpy(), g["out/neg_item_emb"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(m.infoNCE_loss(u, i, n, mask=batch["label"][:, 1]).item(), g["out/infonce"], rtol=1e-4)
