"""tests/row_optim_ref.py against torch's own optimizers, in float64 on the CPU -- the restatements the GPU tests hold the kernels to are
themselves held to torch here.  Betas, lr, eps and the decay are exactly representable in float32 (0.875, 0.984375, 2^-5, 2^-20, ...), so the
float32 rounding the restatements apply to their hyperparameters is a no-op and the comparison holds to rtol 1e-12."""
import numpy as np
import pytest
import torch

from tests import row_optim_ref as R

RTOL = 1e-12
B1, B2, LR, EPS = 0.875, 0.984375, 2.0 ** -5, 2.0 ** -20


def test_the_hyperparameters_of_this_file_are_float32_values():
    for x in (B1, B2, LR, EPS, 2.0 ** -3, LR * 2.0 ** -3):
        assert R.f32(x) == x
    assert R.f32(0.999) != 0.999 and abs((1 - R.f32(0.999)) / (1 - 0.999) - 1) > 1e-5        # (why the restatements round: see their docstring)


def test_key_list_has_every_kind_of_entry_and_hides_a_live_one():
    rng = np.random.default_rng(0)
    for n in (1, 3, 4, 5, 37, 2053):
        rows = R.rows_for(n)
        keys, n_dev = R.key_list(n, rng, rows)
        assert keys.shape == (n,) and n_dev == (n - 1 if n >= 3 else None)
        live = [int(k) for k in keys if R.is_live(k, 3)]
        assert len(set(live)) == len(live) and all(R.split_key(k)[1] < rows for k in live)
        if n >= 37:
            kinds = {"neg": (keys == -1).any(), "big": (keys == R.BIG).any(), "row0": (keys == (1 << 40)).any(), "table3": (keys == ((3 << 40) | 5)).any()}
            assert all(kinds.values()), kinds
            assert R.is_live(keys[-1], 3) and int(keys[-1]) not in [int(k) for k in keys[:-1]]
            # the list is not padded out with fillers: the tables supply enough distinct rows
            assert len(live) >= n - (n + 4) // 5 - (n + 6) // 7 - 2
            assert {R.split_key(k)[0] for k in live[:-1]} == {0, 1, 2} and rows <= n // 2


def _coo(rows_named, dim, n_rows, rng):
    idx = torch.tensor(sorted(rows_named), dtype=torch.int64)
    val = torch.from_numpy(rng.standard_normal((idx.numel(), dim)))
    return idx, val, torch.sparse_coo_tensor(idx[None], val, (n_rows, dim)).coalesce()


@pytest.mark.parametrize("dim", [1, 6])
def test_adam_rows_is_torch_sparse_adam_in_float64(dim):
    rng = np.random.default_rng([1, dim])
    n_rows, n_tables = 23, 3
    params = [torch.from_numpy(rng.standard_normal((n_rows, dim))).requires_grad_(True) for _ in range(n_tables)]
    opt = torch.optim.SparseAdam(params, lr=LR, betas=(B1, B2), eps=EPS)
    w = [p.detach().numpy().copy() for p in params]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    w0 = [x.copy() for x in w]
    ever = [set() for _ in range(n_tables)]
    for step in range(1, 5):
        # SparseAdam's step size is lr * sqrt(1 - beta2^t) / (1 - beta1^t); the kernel takes it as a float: this step's lr is chosen so that it is one
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
        ss = R.f32(LR * np.sqrt(bc2) / bc1)
        opt.param_groups[0]["lr"] = ss * bc1 / np.sqrt(bc2)
        keys, grads = [], []
        for t, p in enumerate(params):
            named = set(int(r) for r in rng.choice(np.arange(1, n_rows), size=7, replace=False))
            idx, val, p.grad = _coo(named, dim, n_rows, rng)
            keys += [(t << 40) | int(r) for r in idx]
            grads += [val.numpy()]
            ever[t] |= named
        # what torch never sees and the rule must skip: fillers, the padding row, a table out of range (their gradient rows are garbage)
        extra = np.array([-1, R.BIG, (1 << 40) | 0, (n_tables << 40) | 3], dtype=np.int64)
        keys = np.concatenate([np.array(keys, dtype=np.int64), extra])
        g = np.concatenate(grads + [rng.standard_normal((extra.size, dim)) * 100])
        perm = rng.permutation(keys.size)
        opt.step()
        w, m, v, named = R.adam_rows(w, m, v, keys[perm], g[perm], n_tables, ss, B1, B2, EPS, 0.0)
        assert sum(len(x) for x in named) == 21
        for t, p in enumerate(params):
            st = opt.state[p]
            np.testing.assert_allclose(w[t], p.detach().numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(m[t], st["exp_avg"].numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(v[t], st["exp_avg_sq"].numpy(), rtol=RTOL, atol=0)
    for t in range(n_tables):                    # rows no step named: untouched, bit for bit
        rest = np.array(sorted(set(range(n_rows)) - ever[t]))
        assert rest.size and 0 in rest
        assert np.array_equal(w[t][rest], w0[t][rest]) and not m[t][rest].any() and not v[t][rest].any()
        assert not np.array_equal(w[t][sorted(ever[t])], w0[t][sorted(ever[t])])


def test_adam_rows_decay_is_decoupled_and_applies_to_named_rows_only():
    """SparseAdam has no weight decay: the decayed rule differs from the plain one by exactly w * decay on the named rows."""
    rng = np.random.default_rng(2)
    w = [rng.standard_normal((9, 4))]
    m, v = [0.3 * rng.standard_normal((9, 4))], [0.1 + rng.random((9, 4))]
    keys = np.array([3, 5, 0, -1], dtype=np.int64)
    g = rng.standard_normal((4, 4))
    decay = 2.0 ** -7
    wa, ma, va, na = R.adam_rows(w, m, v, keys, g, 1, 2.0 ** -4, B1, B2, EPS, 0.0)
    wb, mb, vb, nb = R.adam_rows(w, m, v, keys, g, 1, 2.0 ** -4, B1, B2, EPS, decay)
    assert na == nb == [{3, 5}]
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(va[0], vb[0])
    np.testing.assert_allclose(wa[0][[3, 5]] - wb[0][[3, 5]], w[0][[3, 5]] * decay, rtol=1e-9, atol=0)
    rest = [0, 1, 2, 4, 6, 7, 8]
    assert np.array_equal(wb[0][rest], w[0][rest]) and np.array_equal(mb[0][rest], m[0][rest]) and np.array_equal(vb[0][rest], v[0][rest])


@pytest.mark.parametrize("dim", [1, 6])
def test_adamw_all_rows_is_torch_adamw_in_float64_on_mostly_zero_gradients(dim):
    rng = np.random.default_rng([3, dim])
    rows, wd = [19, 1, 8], 2.0 ** -3
    params = [torch.from_numpy(rng.standard_normal((r, dim))).requires_grad_(True) for r in rows]
    opt = torch.optim.AdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    w = [p.detach().numpy().copy() for p in params]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    for step in range(1, 5):
        keys = np.array([(0 << 40) | 3, (0 << 40) | int(rng.integers(4, 19)), (2 << 40) | int(rng.integers(1, 8)), -1, R.BIG, (0 << 40) | 0,
                         (2 << 40) | 8, (3 << 40) | 1], dtype=np.int64)          # the last five: fillers, the padding row, a row past the table, table 3
        g = rng.standard_normal((keys.size, dim))
        slots = R.mark_slots(keys, rows, 3)
        assert [sorted(s.values()) for s in slots] == [[0, 1], [], [2]]
        for t, p in enumerate(params):
            p.grad = torch.zeros_like(p)
            for r, i in slots[t].items():
                p.grad[r] = torch.from_numpy(g[i])
        opt.step()
        before = [x.copy() for x in w]
        w, m, v = R.adamw_all_rows(w, m, v, [{r: g[i] for r, i in s.items()} for s in slots], step, LR, B1, B2, EPS, wd)
        for t, p in enumerate(params):
            st = opt.state[p]
            np.testing.assert_allclose(w[t], p.detach().numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(m[t], st["exp_avg"].numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(v[t], st["exp_avg_sq"].numpy(), rtol=RTOL, atol=0)
            assert (w[t] != before[t]).all()                     # every row moves every step, row 0 included


def test_merge_lists_folds_shared_rows_once_in_fp32():
    rows = [10, 4]
    ka = np.array([(0 << 40) | 3, -1, (1 << 40) | 2, (0 << 40) | 7, (0 << 40) | 0, R.BIG], dtype=np.int64)
    kb = np.array([(1 << 40) | 2, (0 << 40) | 5, (0 << 40) | 3, -1, (0 << 40) | 0, (1 << 40) | 9, (2 << 40) | 3, R.BIG], dtype=np.int64)
    rng = np.random.default_rng(4)
    va, vb = rng.standard_normal((6, 3)).astype(np.float32), rng.standard_normal((8, 3)).astype(np.float32)
    assert R.mark_slots(ka, rows, 2) == [{3: 0, 7: 3}, {2: 2}]
    kb2, va2 = R.merge_lists(ka, va, kb, vb, rows, 2)
    assert kb2.tolist() == [-1, kb[1], -1] + kb[3:].tolist()
    assert va2.dtype == np.float32
    assert np.array_equal(va2[0], va[0] + vb[2]) and np.array_equal(va2[2], va[2] + vb[0])
    assert np.array_equal(va2[[1, 3, 4, 5]], va[[1, 3, 4, 5]])
    assert kb[0] == (1 << 40) | 2 and np.array_equal(ka, ka.copy())          # the inputs are left alone
