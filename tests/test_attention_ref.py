"""tests/attention_ref.py, the float64 restatement the GPU attention tests are judged by, checked on the CPU: it agrees with a
straightforward torch float64 softmax(Q K^T) V and its autograd, and the project's fp32 torch path (attention_math) sits under a quarter of
the derived bounds on every case the GPU tests use -- the bounds are not what makes those tests pass."""
import numpy as np
import pytest
import torch

from news_recsys_amd.model.model_utils.utils import attention_math
from tests.attention_ref import BIG_CASE, GPU_CASES, attention_ref, case_id, make_case, worst_ratio

CHECKED = [(3, 7, 2, 8, "none", 1.0), (3, 7, 2, 8, "prefix", 1.0), (2, 50, 4, 16, "holes", 1.0), (4, 33, 3, 12, "weights", 3.0),
           (1, 1, 1, 4, "none", 1.0), (2, 128, 1, 64, "none", 1.0)]


def _torch_plain(qkv, g_out, mask, heads, dtype):
    """softmax(q k^T scale) v per head with -inf on masked keys, samples without a kept key zeroed; values and autograd gradient."""
    x = torch.from_numpy(qkv).to(dtype).requires_grad_(True)
    B, N, W = x.shape
    C = W // 3
    hd = C // heads
    q, k, v = x.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * (hd ** -0.5)
    some = torch.ones(B, dtype=torch.bool)
    if mask is not None:
        keep = torch.from_numpy(mask) != 0
        some = keep.any(dim=1)
        s = s.masked_fill(~keep[:, None, None, :] & some[:, None, None, None], float("-inf"))
    lse = torch.where(some[:, None, None], torch.logsumexp(s, dim=-1), torch.tensor(float("-inf"), dtype=dtype))
    out = (torch.softmax(s, dim=-1) @ v * some[:, None, None, None].to(dtype)).transpose(1, 2).reshape(B, N, C)
    (grad,) = torch.autograd.grad(out, x, torch.from_numpy(g_out).to(dtype))
    return out.detach().numpy(), lse.detach().numpy(), grad.numpy()


@pytest.mark.parametrize("case", CHECKED, ids=case_id)
def test_restatement_matches_torch_float64(case):
    B, N, H, hd, mk, sc = case
    qkv, g_out, mask = make_case(7, B, N, H, hd, mk, sc)
    ref = attention_ref(qkv, H, mask=mask, g_out=g_out)
    out, lse, grad = _torch_plain(qkv, g_out, mask, H, torch.float64)
    np.testing.assert_allclose(ref.out, out, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref.lse, lse, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref.g_qkv, grad, rtol=1e-11, atol=1e-12 * max(1.0, np.abs(grad).max()))


def test_a_sample_without_a_kept_key_is_zero_with_bound_zero():
    qkv, g_out, mask = make_case(3, 3, 9, 2, 8, "prefix")
    assert not mask[1].any() and mask[0].all()
    ref = attention_ref(qkv, 2, mask=mask, g_out=g_out)
    assert not ref.out[1].any() and not ref.g_qkv[1].any() and np.all(np.isneginf(ref.lse[1]))
    assert not ref.tol_out[1].any() and not ref.tol_g_qkv[1].any() and not ref.tol_lse[1].any()
    assert worst_ratio(ref.out, ref.out, ref.tol_out) == 0.0 and worst_ratio(ref.lse, ref.lse, ref.tol_lse) == 0.0
    assert worst_ratio(ref.out + 1e-30, ref.out, ref.tol_out) == np.inf          # bound 0 means exact


def test_custom_scale_and_mask_weights_count_as_kept():
    qkv, g_out, mask = make_case(5, 4, 11, 2, 4, "weights")
    a = attention_ref(qkv, 2, mask=mask, g_out=g_out, scale=0.3)
    b = attention_ref(qkv, 2, mask=(mask != 0).astype(np.float32), g_out=g_out, scale=0.3)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.g_qkv, b.g_qkv)
    assert not np.array_equal(a.out, attention_ref(qkv, 2, mask=mask).out)


@pytest.mark.parametrize("case", GPU_CASES + [BIG_CASE], ids=case_id)
def test_fp32_torch_sits_under_a_quarter_of_the_bound(case):
    B, N, H, hd, mk, sc = case
    qkv, g_out, mask = make_case(0, B, N, H, hd, mk, sc)
    ref = attention_ref(qkv, H, mask=mask, g_out=g_out)
    x = torch.from_numpy(qkv).requires_grad_(True)
    out = attention_math(x, H, None if mask is None else torch.from_numpy(mask))
    (grad,) = torch.autograd.grad(out, x, torch.from_numpy(g_out))
    _, lse, _ = _torch_plain(qkv, g_out, mask, H, torch.float32)
    r_out = worst_ratio(out.detach().numpy(), ref.out, ref.tol_out)
    r_grad = worst_ratio(grad.numpy(), ref.g_qkv, ref.tol_g_qkv)
    r_lse = worst_ratio(lse, ref.lse, ref.tol_lse)
    print(f"{case_id(case)}: out {r_out:.4f} grad {r_grad:.4f} lse {r_lse:.4f} of the bound")
    assert r_out <= 0.25 and r_grad <= 0.25 and r_lse <= 0.25
