"""Candidate softmax loss (ops.candidate_softmax, DSSM `extra_negatives` / `logq_correction`): what can be checked without a GPU.  The float64
restatement the GPU tests compare against equals float64 autograd and, on a square set without a bias, the in-batch restatement; an fp32
torch evaluation of the materialised form stays inside the derived tolerances at the GPU tests' shapes (the bounds do not lean on the
kernel); the entry points refuse bad arguments before any launch; the hparams and the module's errors; the host half of the entry points is
clean under ASan + UBSan (a stand-alone driver)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.recall.DSSM.model import DSSM
from tests import candidate_softmax_ref as R
from tests.conftest import CONFIGS, ROOT
from tests.inbatch_softmax_ref import grad_tolerance as inbatch_grad_tolerance, inbatch_softmax_ref, loss_tolerance as inbatch_loss_tolerance

HP = {"lr": 1e-3, "min_lr": 1e-5, "lr_milestones": [4, 20]}
CFG = os.path.join(CONFIGS, "cf_dssm_small.yaml")


@pytest.mark.parametrize("ids_kind,with_bias", [(None, False), (64, False), (None, True), (32, True)])
def test_ref_is_float64_autograd_of_the_materialised_form(ids_kind, with_bias):
    u, v, ids, bias, g, ref = R.make_case(23, 14, 8, ids_kind, with_bias, scale=1.0, temperature=0.5, seed=3)
    U, V = u.double().requires_grad_(True), v.double().requires_grad_(True)
    rows = R.torch_candidate_rows(U, V, float(np.float32(2.0)), ids=ids, bias=None if bias is None else bias.double())
    rows.backward(g.double())
    if ids is not None:
        assert ((ids[:23, None] == ids[None, :]) & ~torch.eye(23, 37, dtype=torch.bool))[:, 23:].any()       # an extra collides with a positive
    np.testing.assert_allclose(ref.loss, rows.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.dU, U.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref.dV, V.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert ref.dV.shape == (37, 8) and np.abs(ref.dV[23:]).max() > 0          # the extras have gradients
    tu, tv = R.grad_tolerance(ref, 8)
    assert np.all(tu[::3] <= 2.0 ** -126) and tu.max() < 1e-3 * np.abs(ref.dU).max() and tv.max() < 1e-3 * np.abs(ref.dV).max()
    assert R.loss_tolerance(ref, 8).max() < 1e-3


@pytest.mark.parametrize("ids_kind", [None, 64])
def test_square_set_without_bias_is_the_in_batch_restatement(ids_kind):
    u, v, ids, _, g, ref = R.make_case(37, 0, 16, ids_kind)
    old = inbatch_softmax_ref(u.numpy(), v.numpy(), np.float32(10.0), ids=None if ids is None else ids.numpy(), g=g.numpy())
    for k in ("loss", "lse", "diag", "dU", "dV"):
        assert np.array_equal(getattr(ref, k), getattr(old, k)), k
    # ... and the bounds are no tighter than the in-batch op's: one more rounded addition, a weight that is never smaller
    assert np.all(R.loss_tolerance(ref, 16) >= inbatch_loss_tolerance(old, 16))
    for new, was in zip(R.grad_tolerance(ref, 16), inbatch_grad_tolerance(old, 16)):
        assert np.all(new >= was)


def _fp32_excess(case):
    """Worst error / bound of the fp32 torch evaluation of the materialised form: (loss, dU, dV)."""
    u, v, ids, bias, g, ref = R.make_case(**case)
    d = case["d"]
    U, V = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    rows = R.torch_candidate_rows(U, V, float(np.float32(1.0 / case.get("temperature", 0.1))), ids=ids, bias=bias)
    rows.backward(g)
    tu, tv = R.grad_tolerance(ref, d)
    return (float((np.abs(rows.detach().numpy().astype(np.float64) - ref.loss) / R.loss_tolerance(ref, d)).max()),
            float((np.abs(U.grad.numpy().astype(np.float64) - ref.dU) / tu).max()),
            float((np.abs(V.grad.numpy().astype(np.float64) - ref.dV) / tv).max()))


def _all_cases():
    cases = []
    for B in R.SMALL_B:
        cases += R.small_cases(B)
    for d in R.DIMS:
        cases += R.dim_cases(d)
    for B, E in R.LARGE_SHAPES:
        cases += R.large_cases(B, E)
    return cases + R.hot_cases()


def test_an_fp32_torch_evaluation_stays_inside_the_tolerances_at_the_gpu_tests_shapes():
    """The bounds are derived (tests/candidate_softmax_ref.py); this holds them against an fp32 evaluation that is not the kernel, at every
    case the GPU tests run.  Nothing comes close to the bound: a bound that fp32 rounding alone exceeded would be a wrong derivation."""
    worst = np.zeros(3)
    for case in _all_cases():
        ex = np.array(_fp32_excess(case))
        assert np.all(np.isfinite(ex)) and ex.max() <= 1.0, (case, ex)
        worst = np.maximum(worst, ex)
    print("worst fp32 error / bound (loss, dU, dV):", worst)
    assert worst.max() > 1e-4          # ... and are not vacuous


def test_hot_cases_reach_scores_near_1e4():
    for case in R.hot_cases():
        ref = R.make_case(**case)[5]
        assert ref.zmax > 3e3 and np.abs(ref.lse).max() > 3e3


# ---- the C-ABI refuses bad arguments before any launch (host "device" buffers: never dereferenced) -----------------------------------------
class _Bufs:
    def __init__(self):
        self.keep = [ctypes.create_string_buffer(8192 + 64) for _ in range(10)]
        base = [(ctypes.addressof(b) + 63) & ~63 for b in self.keep]
        self.u, self.v, self.gu, self.gv, self.loss, self.lse, self.g, self.ids, self.ws, self.bias = base


def _fwd(lib, b, **kw):
    a = dict(u=b.u, u_ld=16, v=b.v, v_ld=16, batch=8, n=12, dim=16, inv_t=10.0, ids=b.ids, bits=64, bias=b.bias, splits=0, loss=b.loss,
             lse=b.lse, ws=b.ws)
    a.update(kw)
    return lib.nrx_cand_softmax_fwd(a["u"], a["u_ld"], a["v"], a["v_ld"], a["batch"], a["n"], a["dim"], a["inv_t"], a["ids"], a["bits"],
                                    a["bias"], a["splits"], a["loss"], a["lse"], a["ws"], None)


def _bwd(lib, b, **kw):
    a = dict(u=b.u, u_ld=16, v=b.v, v_ld=16, batch=8, n=12, dim=16, inv_t=10.0, ids=b.ids, bits=64, bias=b.bias, splits=0, lse=b.lse, g=b.g,
             gu=b.gu, gu_ld=16, gv=b.gv, gv_ld=16, ws=b.ws)
    a.update(kw)
    return lib.nrx_cand_softmax_bwd(a["u"], a["u_ld"], a["v"], a["v_ld"], a["batch"], a["n"], a["dim"], a["inv_t"], a["ids"], a["bits"],
                                    a["bias"], a["splits"], a["lse"], a["g"], a["gu"], a["gu_ld"], a["gv"], a["gv_ld"], a["ws"], None)


BAD_BOTH = [(dict(u=None), "null"), (dict(v=None), "null"), (dict(lse=None), "null"), (dict(ws=None), "null"),
            (dict(dim=0), "dim"), (dict(dim=5), "dim"), (dict(dim=132, u_ld=132, v_ld=132, gu_ld=132, gv_ld=132), "dim"),
            (dict(u_ld=12), "row stride"), (dict(v_ld=8), "row stride"),
            (dict(u_ld=18), "misaligned"), (dict(v_ld=17), "misaligned"),
            (dict(bits=16), "index_bits"), (dict(batch=-1), "batch"),
            (dict(n=7), "n_cand"), (dict(n=-1), "n_cand"), (dict(n=2 ** 31 - 1), "n_cand"), (dict(n=2 ** 40), "n_cand"),
            (dict(inv_t=0.0), "inv_temperature"), (dict(inv_t=-2.0), "inv_temperature"), (dict(inv_t=float("inf")), "inv_temperature"),
            (dict(inv_t=float("nan")), "inv_temperature"), (dict(splits=-1), "col_splits"), (dict(splits=65), "col_splits")]


@pytest.mark.parametrize("kw,word", BAD_BOTH + [(dict(loss=None), "null")])
def test_forward_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    b = _Bufs()
    kw = {k: v for k, v in kw.items() if not k.startswith("g")}
    assert _fwd(lib, b, **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_cand_softmax_fwd" in lib.nrx_last_error()


@pytest.mark.parametrize("kw,word", BAD_BOTH + [(dict(g=None), "null"), (dict(gu_ld=12), "row stride"), (dict(gv_ld=18), "misaligned")])
def test_backward_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    b = _Bufs()
    assert _bwd(lib, b, **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_cand_softmax_bwd" in lib.nrx_last_error()


def test_misaligned_bases_unsupported_dims_empty_calls_and_the_size_call():
    lib = _lib.load()
    b = _Bufs()
    assert _fwd(lib, b, u=b.u + 4) == -1 and b"misaligned rows" in lib.nrx_last_error()
    assert _bwd(lib, b, gv=b.gv + 8) == -1 and b"misaligned rows" in lib.nrx_last_error()
    assert _fwd(lib, b, ids=b.ids + 4) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    assert _fwd(lib, b, bias=b.bias + 2) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    assert _bwd(lib, b, bias=b.bias + 1) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    wide = dict(dim=96, u_ld=96, v_ld=96)
    assert _fwd(lib, b, **wide) == _lib.NRX_ERR_UNSUPPORTED and b"dim=96" in lib.nrx_last_error()
    assert _bwd(lib, b, gu_ld=96, gv_ld=96, **wide) == _lib.NRX_ERR_UNSUPPORTED
    # nothing to do: NRX_OK without a launch (no device here: a launch would fail) -- an empty batch, with or without candidates
    none = dict(u=None, v=None, lse=None, ws=None, ids=None, bias=None)
    assert _fwd(lib, b, batch=0, n=0, loss=None, **none) == 0 and _fwd(lib, b, batch=0, n=12) == 0
    assert _bwd(lib, b, batch=0, n=0, g=None, gu=None, gv=None, **none) == 0 and _bwd(lib, b, batch=0, n=12) == 0
    assert _bwd(lib, b, gu=None, gv=None) == 0
    # the size call: forward B (2 splits + 1); a split backward role splits * owned * dim; never B * N
    assert lib.nrx_cand_softmax_workspace(8, 12, 16, 1) >= 4 * 3 * 8
    assert lib.nrx_cand_softmax_workspace(4096, 8192, 16, 3) >= 4 * 3 * 8192 * 16
    assert lib.nrx_cand_softmax_workspace(4096, 8192, 16, 0) < 4096 * 8192 * 4 // 8
    for bad in ((-1, 12, 16, 0), (8, 7, 16, 0), (8, 2 ** 31 - 1, 16, 0), (8, 12, 0, 0), (8, 12, 5, 0), (8, 12, 132, 0), (8, 12, 96, 0),
                (8, 12, 16, 65), (2 ** 40, 2 ** 40, 16, 0)):
        assert lib.nrx_cand_softmax_workspace(*bad) == -1, bad
    # a square set is the in-batch op's own sizes: the same split choice
    for B in (1, 33, 511, 512, 1000, 4096, 8191, 65536, 10 ** 6):
        for s in (0, 1, 3, 64):
            assert lib.nrx_cand_softmax_workspace(B, B, 16, s) == lib.nrx_inbatch_softmax_workspace(B, 16, s), (B, s)
    assert lib.nrx_abi_version() == 3 == _lib.NRX_ABI_VERSION           # the additions are additive


def test_op_has_no_cpu_fallback():
    """(The refusals that need device tensors to be reached are in tests/test_candidate_softmax_gpu.py.)"""
    u, v = torch.randn(8, 16), torch.randn(12, 16)
    with pytest.raises(_lib.NrxError, match="candidate_softmax: u"):
        ops.candidate_softmax(u, v)
    with pytest.raises(_lib.NrxError):
        ops.candidate_softmax(u.requires_grad_(True), v, temperature=0.05, ids=torch.arange(12), col_bias=torch.zeros(12))


# ---- hparams and the module's errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [-1, 1.5, "8", None, True])
def test_extra_negatives_hparam_is_validated_at_construction(value):
    with pytest.raises(ValueError, match="extra_negatives"):
        DSSM(CFG, hparams=dict(HP, negatives="in_batch", extra_negatives=value))


@pytest.mark.parametrize("value", [1, "yes", None])
def test_logq_correction_hparam_is_validated_at_construction(value):
    with pytest.raises(ValueError, match="logq_correction"):
        DSSM(CFG, hparams=dict(HP, negatives="in_batch", logq_correction=value))


def test_new_hparams_default_off_and_belong_to_in_batch():
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch"))
    assert m.extra_negatives == 0 and m.logq_correction is False and m.negative_corpus is None and m.item_probs is None
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch", extra_negatives=24, logq_correction=True))
    assert m.extra_negatives == 24 and m.logq_correction is True
    assert DSSM(CFG, hparams=HP).extra_negatives == 0
    for extra in (dict(extra_negatives=4), dict(logq_correction=True)):
        with pytest.raises(ValueError, match="in_batch"):
            DSSM(CFG, hparams=dict(HP, **extra))


def _corpus(M=45):
    return {"item_id": torch.arange(M), "category": torch.arange(M) % 18}


def test_item_counts_are_a_non_persistent_buffer_of_smoothed_frequencies():
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch", logq_correction=True))
    keys = list(m.state_dict().keys())
    counts = torch.tensor([0.0, 3.0, 1.0, 0.0, 6.0])
    p = m.set_item_counts(counts, smoothing=0.5)
    np.testing.assert_allclose(p.numpy(), ((counts + 0.5) / (10.0 + 2.5)).numpy(), rtol=1e-6)
    np.testing.assert_allclose(m.set_item_counts([1, 1, 2]).numpy(), np.array([2, 2, 3]) / 7.0, rtol=1e-6)       # smoothing defaults to 1
    assert list(m.state_dict().keys()) == keys and "item_probs" in dict(m.named_buffers())
    assert list(DSSM(CFG, hparams=HP).state_dict().keys()) == keys
    for bad in ([], [1.0, -1.0], [float("nan")], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="set_item_counts"):
            m.set_item_counts(bad)
    with pytest.raises(ValueError, match="set_item_counts"):
        m.set_item_counts([0.0, 0.0], smoothing=0.0)


def test_logq_bias_is_minus_log_of_the_expected_appearances():
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch", item_id_feature="item_id", logq_correction=True, extra_negatives=6))
    with pytest.raises(ValueError, match="set_item_counts"):
        m.logq_bias(torch.tensor([1, 2]), 4)
    p = m.set_item_counts(torch.arange(45, dtype=torch.float32))
    with pytest.raises(ValueError, match="set_negative_corpus"):
        m.logq_bias(torch.tensor([1, 2]), 4)
    m.set_negative_corpus(_corpus())
    ids = torch.tensor([3, 44, 0, 3])
    np.testing.assert_allclose(m.logq_bias(ids, 16).numpy(), -np.log(16 * p[ids].numpy().astype(np.float64) + 6 / 45), rtol=1e-6)
    m0 = DSSM(CFG, hparams=dict(HP, negatives="in_batch", logq_correction=True))         # E == 0: no uniform term
    p = m0.set_item_counts(torch.arange(45, dtype=torch.float32))
    np.testing.assert_allclose(m0.logq_bias(ids, 16).numpy(), -np.log(16 * p[ids].numpy().astype(np.float64)), rtol=1e-6)


def test_negative_corpus_columns_are_checked_and_read_from_the_item_loader():
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch", item_id_feature="item_id", extra_negatives=4))
    with pytest.raises(ValueError, match="movies_dataloader"):
        m.set_negative_corpus()
    with pytest.raises(KeyError, match="item_id"):
        m.set_negative_corpus({"category": torch.arange(5)})
    with pytest.raises(ValueError, match="one row per item"):
        m.set_negative_corpus({"item_id": torch.arange(5), "category": torch.arange(4)})
    with pytest.raises(ValueError, match="one row per item"):
        m.set_negative_corpus({"item_id": torch.arange(0), "category": torch.arange(0)})
    with pytest.raises(ValueError, match="CSR"):
        m.set_negative_corpus({"item_id": torch.arange(5), "tags_offsets": torch.arange(5)})
    got = m.set_negative_corpus(_corpus())
    assert set(got) == {"item_id", "category"} and got["item_id"].shape == (45,)
    # from the loader: the item tower's columns and the id column of every batch, in order; other columns are left behind
    loader = [{"item_id": torch.arange(0, 30), "category": torch.arange(0, 30) % 18, "title": torch.zeros(30)},
              {"item_id": torch.arange(30, 45), "category": torch.arange(30, 45) % 18, "title": torch.zeros(15)}]
    m = DSSM(CFG, dataloaders={"movies_dataloader": loader}, hparams=dict(HP, negatives="in_batch", item_id_feature="item_id", extra_negatives=4))
    got = m.set_negative_corpus()
    assert set(got) == {"item_id", "category"} and torch.equal(got["item_id"], torch.arange(45)) and torch.equal(got["category"], torch.arange(45) % 18)
    idx = m._draw_extra_idx("cpu")
    assert idx.shape == (4,) and int(idx.min()) >= 0 and int(idx.max()) < 45
    cols = m._extra_columns(torch.tensor([44, 0, 7, 7]))
    assert cols["item_id"].tolist() == [44, 0, 7, 7] and cols["category"].tolist() == [44 % 18, 0, 7, 7]


def test_training_without_the_corpus_or_the_counts_is_refused():
    batch = {"label": torch.ones(4, 2), "item_id": torch.arange(4)}
    m = DSSM(CFG, hparams=dict(HP, negatives="in_batch", item_id_feature="item_id", extra_negatives=4))
    with pytest.raises(ValueError, match="set_negative_corpus"):
        m.training_step(batch, 0)
    with pytest.raises(ValueError, match="set_negative_corpus"):
        m._extra_columns(torch.arange(4))


# ---- the host half of the entry points under ASan + UBSan: a stand-alone driver with its own main, run directly
def test_cand_softmax_host_validation_is_clean_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    if not os.path.exists(os.path.join(ROOT, "tests", "sanitize", "cand_softmax.mk")):
        pytest.skip("tests/sanitize/ is not part of this tree (it does not travel to the GPU machines)")
    p = subprocess.run(["make", "-C", "tests/sanitize", "-f", "cand_softmax.mk", "run"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert "nrx_cand_softmax validation sanitize driver: OK" in out
