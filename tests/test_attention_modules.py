"""MultiHeadSelfAttention and TransformerBlock (news_recsys_amd/model/model_utils/utils.py) on the CPU against the fixture recorded from the
reference's own classes (tests/golden/data/attention.npz, written by tests/golden/gen_attention_golden.py), the key mask's semantics on
the torch path, and the host side of nrx_attn_fwd / _bwd (argument checks answer before any launch, so no GPU is needed).

Tolerances against the fixture are the project's own for fp32 through nn.Linear (tests/test_inbatch_softmax_gpu.py, the DSSM test):
outputs rtol 1e-4, atol 1e-5 max|want|; gradients rtol 2e-3, atol 2e-6 + 1e-4 max|want|."""
import ctypes
import os

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.model_utils.utils import MultiHeadSelfAttention, TransformerBlock
from tests.conftest import GOLDEN

# name, class, embed_dim, heads, ff_dim, B, N
CASES = (("mhsa_16x2", MultiHeadSelfAttention, 16, 2, None, 3, 7),
         ("mhsa_32x4", MultiHeadSelfAttention, 32, 4, None, 2, 50),
         ("block_16x2", TransformerBlock, 16, 2, 32, 3, 7),
         ("block_32x4", TransformerBlock, 32, 4, 64, 2, 50))
MHSA_KEYS = ["qkv_proj.weight", "qkv_proj.bias", "out_proj.weight", "out_proj.bias"]
BLOCK_KEYS = (["attention." + k for k in MHSA_KEYS] + ["norm1.weight", "norm1.bias", "ffn.0.weight", "ffn.0.bias", "ffn.2.weight", "ffn.2.bias",
                                                       "norm2.weight", "norm2.bias"])


def fixture():
    return np.load(os.path.join(GOLDEN, "data", "attention.npz"))


def build(case, device="cpu"):
    """The module of a case with the fixture's weights (strict), and the fixture's arrays of that case."""
    name, cls, dim, heads, ff, B, N = case
    data = fixture()
    module = cls(dim, heads) if ff is None else cls(dim, heads, ff)
    prefix = name + "/sd/"
    state = {k[len(prefix):]: torch.from_numpy(data[k]) for k in data.files if k.startswith(prefix)}
    module.load_state_dict(state, strict=True)
    return module.to(device), {k[len(name) + 1:]: data[k] for k in data.files if k.startswith(name + "/")}


def check_against_fixture(module, arrays, device="cpu"):
    x = torch.from_numpy(arrays["x"]).to(device).requires_grad_(True)
    out = module(x)
    (out * torch.from_numpy(arrays["g"]).to(device)).sum().backward()
    want = arrays["out"]
    np.testing.assert_allclose(out.detach().cpu().numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
    grads = {"grad_x": x.grad}
    grads.update({"grad/" + k: p.grad for k, p in module.named_parameters()})
    assert sorted(grads) == sorted(k for k in arrays if k.startswith("grad"))
    for key, got in grads.items():
        want = arrays[key]
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-3, atol=2e-6 + 1e-4 * np.abs(want).max(), err_msg=key)


def test_state_dict_keys_shapes_and_attributes():
    m = MultiHeadSelfAttention(32, 4)
    assert (m.embed_dim, m.num_heads, m.head_dim) == (32, 4, 8)
    assert list(m.state_dict()) == MHSA_KEYS
    assert m.qkv_proj.weight.shape == (96, 32) and m.qkv_proj.bias.shape == (96,) and m.out_proj.weight.shape == (32, 32)
    b = TransformerBlock(16, 2, 40, dropout=0.25)
    assert list(b.state_dict()) == BLOCK_KEYS
    assert isinstance(b.attention, MultiHeadSelfAttention) and isinstance(b.norm1, torch.nn.LayerNorm) and isinstance(b.norm2, torch.nn.LayerNorm)
    assert b.ffn[0].weight.shape == (40, 16) and isinstance(b.ffn[1], torch.nn.ReLU) and b.ffn[2].weight.shape == (16, 40)
    assert isinstance(b.dropout, torch.nn.Dropout) and b.dropout.p == 0.25 and TransformerBlock(16, 2, 40).dropout.p == 0.0
    with pytest.raises((ValueError, AssertionError)):
        MultiHeadSelfAttention(30, 4)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixture_weights_load_strict_and_results_match(case):
    module, arrays = build(case)
    want_keys = MHSA_KEYS if case[4] is None else BLOCK_KEYS
    assert sorted(k[3:] for k in arrays if k.startswith("sd/")) == sorted(want_keys)
    check_against_fixture(module, arrays)


@pytest.mark.parametrize("case", (CASES[0], CASES[3]), ids=(CASES[0][0], CASES[3][0]))
def test_no_mask_and_a_mask_of_ones_agree(case):
    module, arrays = build(case)
    x = torch.from_numpy(arrays["x"])
    a = module(x)
    b = module(x, torch.ones(x.shape[:2]))
    assert torch.equal(a, b)


def test_prefix_mask_equals_the_truncated_sequence():
    module, arrays = build(CASES[1])
    x = torch.from_numpy(arrays["x"])
    B, N, _ = x.shape
    lens = [13, 50]
    mask = (torch.arange(N)[None, :] < torch.tensor(lens)[:, None]).float()
    xg = x.clone().requires_grad_(True)
    full = module(xg, mask)
    g = torch.from_numpy(arrays["g"]) * mask[..., None]           # the padded queries' rows are computed, but nobody reads them
    (full * g).sum().backward()
    for b, n in enumerate(lens):
        xt = x[b:b + 1, :n].clone().requires_grad_(True)
        cut = module(xt)
        torch.testing.assert_close(full[b:b + 1, :n], cut, rtol=1e-5, atol=1e-6)
        (cut * g[b:b + 1, :n]).sum().backward()
        torch.testing.assert_close(xg.grad[b:b + 1, :n], xt.grad, rtol=1e-4, atol=1e-6)
        assert not xg.grad[b, n:].any()                           # a masked key with an unread query row receives nothing


def test_all_zero_mask_gives_zero_attention_and_finite_gradients():
    module, arrays = build(CASES[0])
    x = torch.from_numpy(arrays["x"]).requires_grad_(True)
    mask = torch.ones(x.shape[:2])
    mask[1] = 0.0
    out = module(x, mask)
    # zero attention output: what is left of the sample is out_proj's bias
    assert torch.equal(out[1], module.out_proj.bias.expand_as(out[1]))
    out.square().sum().backward()
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in module.parameters())
    assert not x.grad[1].any() and x.grad[0].any()
    block, arrays = build(CASES[2])
    xb = torch.from_numpy(arrays["x"]).requires_grad_(True)
    yb = block(xb, mask)
    yb.square().sum().backward()
    assert torch.isfinite(yb).all() and torch.isfinite(xb.grad).all()


def test_longer_sequences_and_other_dtypes_take_the_torch_path():
    module = MultiHeadSelfAttention(16, 2)
    x = torch.randn(2, 129, 16, generator=torch.Generator().manual_seed(0), requires_grad=True)
    mask = torch.ones(2, 129)
    mask[0, 100:] = 0
    out = module(x, mask)
    out.sum().backward()
    assert out.shape == (2, 129, 16) and torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    half = MultiHeadSelfAttention(16, 2).double()
    assert half(torch.randn(1, 5, 16, dtype=torch.float64)).dtype == torch.float64
    assert MultiHeadSelfAttention(18, 3)(torch.randn(2, 4, 18)).shape == (2, 4, 18)          # head_dim 6: no fused form, torch path


def test_binding_declares_the_entry_points():
    assert "nrx_attn_fwd" in _lib.SIGNATURES and "nrx_attn_bwd" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nrx_attn_fwd"][1]) == 12 and len(_lib.SIGNATURES["nrx_attn_bwd"][1]) == 16
    lib = _lib.load()
    assert hasattr(lib, "nrx_attn_fwd") and hasattr(lib, "nrx_attn_bwd")


def test_op_has_no_cpu_fallback_and_names_unsupported_shapes():
    with pytest.raises(_lib.NrxError):
        ops.seq_attention(torch.zeros(2, 5, 48), 2)
    assert ops.seq_attention_supported(50, 2, 8) and ops.seq_attention_supported(128, 4, 64) and ops.seq_attention_supported(1, 1, 4)
    assert not ops.seq_attention_supported(129, 2, 8) and not ops.seq_attention_supported(50, 3, 6)
    assert not ops.seq_attention_supported(50, 8, 64) and not ops.seq_attention_supported(50, 1, 68)


def test_bad_arguments_are_refused_before_any_launch():
    """Host memory stands in for the buffers: every call below must be answered by the argument checks alone."""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, BAD, UNS = _lib.NRX_OK, _lib.NRX_ERR_BAD_ARG, _lib.NRX_ERR_UNSUPPORTED

    def fwd(qkv=p, qkv_ld=48, batch=2, seq=5, heads=2, hd=8, scale=0.35, mask=None, out=p, out_ld=16, lse=p):
        return lib.nrx_attn_fwd(qkv, qkv_ld, batch, seq, heads, hd, scale, mask, out, out_ld, lse, None)

    def bwd(qkv=p, qkv_ld=48, batch=2, seq=5, heads=2, hd=8, scale=0.35, mask=None, out=p, out_ld=16, lse=p, g=p, g_ld=16, gq=p, gq_ld=48):
        return lib.nrx_attn_bwd(qkv, qkv_ld, batch, seq, heads, hd, scale, mask, out, out_ld, lse, g, g_ld, gq, gq_ld, None)

    assert fwd(batch=0) == OK and bwd(batch=0) == OK
    assert fwd(batch=0, qkv=None, out=None, lse=None) == OK
    for call in (fwd, bwd):
        assert call(qkv=None) == BAD and b"null" in lib.nrx_last_error()
        assert call(out=None) == BAD and call(lse=None) == BAD
        assert call(qkv=p + 4) == BAD and call(out=p + 8) == BAD and call(lse=p + 2) == BAD and call(mask=p + 1) == BAD
        assert call(qkv_ld=47) == BAD and call(qkv_ld=50) == BAD and call(out_ld=12) == BAD and call(out_ld=18) == BAD
        assert call(heads=0) == BAD and call(seq=0) == BAD and call(hd=0) == BAD and call(batch=-1) == BAD
        assert call(scale=float("nan")) == BAD
        assert call(seq=129) == UNS and b"seq" in lib.nrx_last_error()
        assert call(hd=6, qkv_ld=36, out_ld=12) == UNS
        wide = {} if call is fwd else {"g_ld": 512, "gq_ld": 1536}
        assert call(hd=68, heads=1, qkv_ld=204, out_ld=68, **wide) == UNS
        assert call(heads=8, hd=64, qkv_ld=1536, out_ld=512, **wide) == UNS
    assert bwd(g=None) == BAD and bwd(gq=None) == BAD and bwd(g=p + 4) == BAD and bwd(gq=p + 4) == BAD
    assert bwd(g_ld=12) == BAD and bwd(gq_ld=44) == BAD and bwd(g_ld=18) == BAD
    with pytest.raises(ValueError):
        _lib.check(fwd(heads=0), "nrx_attn_fwd")
    with pytest.raises(_lib.NrxError):
        _lib.check(fwd(seq=129), "nrx_attn_fwd")
