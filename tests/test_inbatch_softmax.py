"""In-batch softmax loss (ops.inbatch_softmax, DSSM `negatives: in_batch`): what can be checked without a GPU.  The float64 restatement the GPU
tests compare against is tied to the reference-pinned infoNCE loss; the entry points refuse bad arguments before any launch; the hparams are
validated; the host half of the entry points is clean under ASan + UBSan (a stand-alone driver)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.recall.DSSM.model import DSSM
from tests.conftest import CONFIGS, ROOT
from tests.inbatch_softmax_ref import grad_tolerance, inbatch_softmax_ref, loss_tolerance

HP = {"lr": 1e-3, "min_lr": 1e-5, "lr_milestones": [4, 20]}


def _uv(B, d, seed=0, normalise=True):
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(B, d, generator=gen)
    v = torch.randn(B, d, generator=gen)
    if normalise:
        u, v = F.normalize(u, p=2, dim=1), F.normalize(v, p=2, dim=1)
    return u, v


def test_ref_equals_the_reference_pinned_infonce_loss_fed_every_other_item():
    """Without ids the row losses are the reference's infoNCE loss (DSSM.infoNCE_loss, pinned by tests/golden/model_dssm.npz through
    tests/test_models_gpu.py) whose negatives are the B - 1 cyclic shifts of the batch."""
    B, d = 37, 16
    u, v = _uv(B, d)
    mask = (torch.arange(B) % 3 != 0).float()
    neg = torch.stack([v[(torch.arange(B) + k + 1) % B] for k in range(B - 1)], dim=1)           # [B, B-1, d]
    want = DSSM.infoNCE_loss(None, u, v, neg, temperature=0.1, mask=mask).item()
    ref = inbatch_softmax_ref(u.numpy(), v.numpy(), 1.0 / 0.1)
    got = float((ref.loss * mask.numpy().astype(np.float64)).mean())
    np.testing.assert_allclose(got, want, rtol=1e-6)


def test_ref_gradients_are_autograds_and_the_mask_drops_same_item_columns():
    """The restated dU / dV are what float64 autograd gives for the materialised masked form, and the bounds are not vacuous."""
    B, d = 23, 8
    u, v = _uv(B, d, seed=1, normalise=False)
    ids = torch.randint(0, 5, (B,), generator=torch.Generator().manual_seed(2))
    g = torch.randn(B, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    g[::4] = 0.0
    ref = inbatch_softmax_ref(u.numpy(), v.numpy(), 2.0, ids=ids.numpy(), g=g.numpy())
    U = u.double().requires_grad_(True)
    V = v.double().requires_grad_(True)
    s = U @ V.T * 2.0
    excl = (ids[:, None] == ids[None, :]) & ~torch.eye(B, dtype=torch.bool)
    assert excl.any()
    rows = torch.logsumexp(s.masked_fill(excl, float("-inf")), dim=1) - s.diagonal()
    rows.backward(g)
    np.testing.assert_allclose(ref.loss, rows.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.dU, U.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref.dV, V.grad.numpy(), rtol=1e-10, atol=1e-12)
    tu, tv = grad_tolerance(ref, d)
    assert np.all(tu[::4] <= 2.0 ** -126) and tu.max() < 1e-3 * np.abs(ref.dU).max() and tv.max() < 1e-3 * np.abs(ref.dV).max()
    assert loss_tolerance(ref, d).max() < 1e-3


# ---- the C-ABI refuses bad arguments before any launch (host "device" buffers: never dereferenced) -----------------------------------------
class _Bufs:
    def __init__(self):
        self.keep = [ctypes.create_string_buffer(8192 + 64) for _ in range(9)]
        base = [(ctypes.addressof(b) + 63) & ~63 for b in self.keep]
        self.u, self.v, self.gu, self.gv, self.loss, self.lse, self.g, self.ids, self.ws = base


def _fwd(lib, b, **kw):
    a = dict(u=b.u, u_ld=16, v=b.v, v_ld=16, batch=8, dim=16, inv_t=10.0, ids=b.ids, bits=64, splits=0, loss=b.loss, lse=b.lse, ws=b.ws)
    a.update(kw)
    return lib.nrx_inbatch_softmax_fwd(a["u"], a["u_ld"], a["v"], a["v_ld"], a["batch"], a["dim"], a["inv_t"], a["ids"], a["bits"], a["splits"],
                                       a["loss"], a["lse"], a["ws"], None)


def _bwd(lib, b, **kw):
    a = dict(u=b.u, u_ld=16, v=b.v, v_ld=16, batch=8, dim=16, inv_t=10.0, ids=b.ids, bits=64, splits=0, lse=b.lse, g=b.g, gu=b.gu, gu_ld=16,
             gv=b.gv, gv_ld=16, ws=b.ws)
    a.update(kw)
    return lib.nrx_inbatch_softmax_bwd(a["u"], a["u_ld"], a["v"], a["v_ld"], a["batch"], a["dim"], a["inv_t"], a["ids"], a["bits"], a["splits"],
                                       a["lse"], a["g"], a["gu"], a["gu_ld"], a["gv"], a["gv_ld"], a["ws"], None)


BAD_BOTH = [(dict(u=None), "null"), (dict(v=None), "null"), (dict(lse=None), "null"), (dict(ws=None), "null"),
            (dict(dim=0), "dim"), (dict(dim=5), "dim"), (dict(dim=132, u_ld=132, v_ld=132, gu_ld=132, gv_ld=132), "dim"),
            (dict(u_ld=12), "row stride"), (dict(v_ld=8), "row stride"),
            (dict(u_ld=18), "misaligned"), (dict(v_ld=17), "misaligned"),
            (dict(bits=16), "index_bits"), (dict(batch=-1), "batch"),
            (dict(inv_t=0.0), "inv_temperature"), (dict(inv_t=-2.0), "inv_temperature"), (dict(inv_t=float("inf")), "inv_temperature"),
            (dict(inv_t=float("nan")), "inv_temperature"), (dict(splits=-1), "col_splits"), (dict(splits=65), "col_splits")]


@pytest.mark.parametrize("kw,word", BAD_BOTH + [(dict(loss=None), "null")])
def test_forward_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    b = _Bufs()
    kw = {k: v for k, v in kw.items() if not k.startswith("g")}
    assert _fwd(lib, b, **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_inbatch_softmax_fwd" in lib.nrx_last_error()


@pytest.mark.parametrize("kw,word", BAD_BOTH + [(dict(g=None), "null"), (dict(gu_ld=12), "row stride"), (dict(gv_ld=18), "misaligned")])
def test_backward_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    b = _Bufs()
    assert _bwd(lib, b, **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_inbatch_softmax_bwd" in lib.nrx_last_error()


def test_misaligned_bases_unsupported_dims_and_empty_calls():
    lib = _lib.load()
    b = _Bufs()
    assert _fwd(lib, b, u=b.u + 4) == -1 and b"misaligned rows" in lib.nrx_last_error()
    assert _bwd(lib, b, gv=b.gv + 8) == -1 and b"misaligned rows" in lib.nrx_last_error()
    assert _fwd(lib, b, ids=b.ids + 4) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    # a multiple of 4 in 65..128 is a valid shape this build has no kernel for: its own code, nothing launched
    wide = dict(dim=96, u_ld=96, v_ld=96)
    assert _fwd(lib, b, **wide) == _lib.NRX_ERR_UNSUPPORTED and b"dim=96" in lib.nrx_last_error()
    assert _bwd(lib, b, gu_ld=96, gv_ld=96, **wide) == _lib.NRX_ERR_UNSUPPORTED
    # nothing to do: NRX_OK without a launch (no device here: a launch would fail)
    assert _fwd(lib, b, batch=0, u=None, v=None, loss=None, lse=None, ws=None, ids=None) == 0
    assert _bwd(lib, b, batch=0, u=None, v=None, lse=None, g=None, gu=None, gv=None, ws=None, ids=None) == 0
    assert _bwd(lib, b, gu=None, gv=None) == 0
    # the size call
    assert lib.nrx_inbatch_softmax_workspace(8, 16, 1) >= 4 * 3 * 8
    assert lib.nrx_inbatch_softmax_workspace(4096, 16, 3) >= 4 * 3 * 4096 * 16
    for bad in ((-1, 16, 0), (8, 0, 0), (8, 5, 0), (8, 132, 0), (8, 96, 0), (8, 16, 65), (2 ** 40, 16, 0)):
        assert lib.nrx_inbatch_softmax_workspace(*bad) == -1, bad
    # the workspace never holds a [B, B] matrix: at the flagship batch it is B * dim floats per split, and one split is chosen
    assert lib.nrx_inbatch_softmax_workspace(65536, 16, 0) <= 4 * 3 * 65536 + 256


def test_op_has_no_cpu_fallback_and_checks_its_inputs():
    u, v = _uv(8, 16)
    with pytest.raises(_lib.NrxError):
        ops.inbatch_softmax(u, v)
    with pytest.raises(_lib.NrxError):
        ops.inbatch_softmax(u.requires_grad_(True), v, temperature=0.05, item_ids=torch.arange(8))


@pytest.mark.parametrize("value", ["in-batch", "", None, 1])
def test_negatives_hparam_is_validated_at_construction(value):
    with pytest.raises(ValueError, match="negatives"):
        DSSM(os.path.join(CONFIGS, "cf_dssm_small.yaml"), hparams=dict(HP, negatives=value))


def test_negatives_hparam_defaults_to_the_references_sampled_loss():
    m = DSSM(os.path.join(CONFIGS, "cf_dssm_small.yaml"), hparams=HP)
    assert m.negatives == "sampled" and m.in_batch_mask_same_item is True
    m = DSSM(os.path.join(CONFIGS, "cf_dssm_small.yaml"), hparams=dict(HP, negatives="in_batch", in_batch_mask_same_item=False))
    assert m.negatives == "in_batch" and m.in_batch_mask_same_item is False
    assert callable(m.in_batch_softmax_loss)


# ---- the host half of the entry points under ASan + UBSan: a stand-alone driver with its own main, run directly
def test_inbatch_host_validation_is_clean_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    if not os.path.exists(os.path.join(ROOT, "tests", "sanitize", "inbatch.mk")):
        pytest.skip("tests/sanitize/ is not part of this tree (it does not travel to the GPU machines)")
    p = subprocess.run(["make", "-C", "tests/sanitize", "-f", "inbatch.mk", "run"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert "nrx_inbatch_softmax validation sanitize driver: OK" in out
