"""CPU checks of the target-attention pooling's yardsticks: the float64 restatement tests/din_pool_ref.py against torch's float64
autograd of the plain formula, and ops.din_pool_math in fp32 against that restatement within a quarter of the bounds the HIP kernels are held
to -- at every case of tests/din_pool_cases.py, the list the GPU test runs."""
import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from tests import din_pool_cases as cases
from tests import din_pool_ref as R


def _plain_torch64(c):
    """out, lse, g_query, dense table gradient by torch.float64 autograd of softmax(q . e * scale) e, sample by sample (an empty sample: zeros)."""
    table = torch.from_numpy(c["table"]).double().requires_grad_(True)
    query = torch.from_numpy(c["query"]).double().requires_grad_(True)
    ids = torch.from_numpy(c["ids"]).long()
    g = torch.from_numpy(c["g_out"]).double()
    B, L = ids.shape
    outs, lses = [], []
    for b in range(B):
        keep = torch.ones(L, dtype=torch.bool) if c["mask_arr"] is None else torch.from_numpy(c["mask_arr"][b] != 0)
        if not keep.any():
            outs.append(torch.zeros(table.shape[1], dtype=torch.float64))
            lses.append(torch.tensor(float("-inf"), dtype=torch.float64))
            continue
        e = table[ids[b][keep]]
        s = (e @ query[b]) * c["scale"]
        outs.append(torch.softmax(s, 0) @ e)
        lses.append(torch.logsumexp(s.detach(), 0))
    out = torch.stack(outs)
    (out * g).sum().backward()
    return out.detach().numpy(), torch.stack(lses).numpy(), query.grad.numpy(), table.grad.numpy()


@pytest.mark.parametrize("i", range(cases.N_CASES), ids=cases.case_id)
def test_float64_reference_equals_torch_autograd(i):
    c = cases.make_case(i)
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    out, lse, gq, gt = _plain_torch64(c)
    np.testing.assert_allclose(ref["out"], out, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["lse"], lse, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["g_query"], gq, rtol=1e-11, atol=1e-12)
    # torch's table gradient includes row 0 (the reference's scatter leaves the padding row out, as the library does)
    want = R.table_grad_ref(ref, c["ids"], cases.ROWS)
    np.testing.assert_allclose(want[1:], gt[1:], rtol=1e-11, atol=1e-12)
    assert not want[0].any()


def test_reference_conventions():
    """Empty sample: zeros, lse -inf, zero gradients; an out-of-range id reads row 0 and gets a zero g_rows row; any non-zero weight keeps."""
    rng = np.random.default_rng(0)
    table = rng.standard_normal((9, 8))
    ids = np.array([[1, 2, 3], [4, -1, 9], [5, 6, 7]])
    mask = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0, -2.0]], dtype=np.float32)
    q, g = rng.standard_normal((3, 8)), rng.standard_normal((3, 8))
    ref = R.din_pool_ref(table, ids, mask, q, 0.3, g)
    assert not ref["out"][0].any() and ref["lse"][0] == -np.inf and not ref["g_query"][0].any() and not ref["g_rows"][0].any()
    same = R.din_pool_ref(table, np.array([[1, 2, 3], [4, 0, 0], [5, 6, 7]]), mask, q, 0.3, g)
    np.testing.assert_array_equal(ref["out"], same["out"])
    assert not ref["g_rows"][1, 1:].any() and same["g_rows"][1, 1:].any()
    assert ref["p"][2, 1] == 0 and ref["p"][2, 0] > 0 and ref["p"][2, 2] > 0


@pytest.mark.parametrize("i", range(cases.N_CASES), ids=cases.case_id)
def test_din_pool_math_fp32_within_a_quarter_of_the_bounds(i):
    c = cases.make_case(i)
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"], c["g_out"])
    bnd = R.bounds(ref, c["table"], c["query"], c["scale"])
    table = torch.from_numpy(c["table"])
    if c["bf16"]:
        table = table.to(torch.bfloat16)
    ids = torch.from_numpy(c["ids"])
    rows = table[ids.long()].float().requires_grad_(True)          # the per-lookup rows as a leaf: their gradient is g_rows
    query = torch.from_numpy(c["query"]).requires_grad_(True)
    mask = None if c["mask_arr"] is None else torch.from_numpy(c["mask_arr"])
    out, lse = ops.din_pool_math(None, None, query, mask, c["scale"], rows=rows, return_lse=True)
    assert out.dtype == torch.float32
    out.backward(torch.from_numpy(c["g_out"]))
    ratios = dict(out=R.worst_ratio(out.detach().numpy(), ref["out"], bnd["out"]), lse=R.worst_ratio(lse.numpy(), ref["lse"], bnd["lse"]),
                  g_query=R.worst_ratio(query.grad.numpy(), ref["g_query"], bnd["g_query"]),
                  g_rows=R.worst_ratio(rows.grad.numpy(), ref["g_rows"], bnd["g_rows"]))
    print(cases.case_id(i), {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 0.25, ratios
    # the table form gives the same output
    out2 = ops.din_pool_math(table, ids, torch.from_numpy(c["query"]), mask, c["scale"])
    assert torch.equal(out2, out.detach())


def test_din_pool_math_large_scores_and_default_scale():
    c = cases.make_case(6, amp=100.0)             # L 50, D 32: scores of the order 1e4 * D ** -0.5
    ref = R.din_pool_ref(c["table"], c["ids"], c["mask_arr"], c["query"], c["scale"])
    bnd = R.bounds(ref, c["table"], c["query"], c["scale"])
    out, lse = ops.din_pool_math(torch.from_numpy(c["table"]), torch.from_numpy(c["ids"]), torch.from_numpy(c["query"]),
                                 torch.from_numpy(c["mask_arr"]), None, return_lse=True)
    assert torch.isfinite(out).all()
    assert R.worst_ratio(out.numpy(), ref["out"], bnd["out"]) <= 0.25 and R.worst_ratio(lse.numpy(), ref["lse"], bnd["lse"]) <= 0.25


def test_supported_shapes():
    assert ops.din_pool_supported(1, 4) and ops.din_pool_supported(256, 64) and ops.din_pool_supported(50, 20)
    assert not ops.din_pool_supported(0, 16) and not ops.din_pool_supported(257, 16)
    assert not ops.din_pool_supported(50, 6) and not ops.din_pool_supported(50, 68) and not ops.din_pool_supported(50, 0)


def test_din_pool_refuses_cpu_tensors():
    from news_recsys_amd import _lib
    with pytest.raises(_lib.NrxError):
        ops.din_pool(torch.zeros(9, 8), torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 8))
