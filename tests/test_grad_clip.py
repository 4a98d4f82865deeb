"""Global-norm clipping of the row-sparse table gradients, CPU side: the numpy restatement of the norm (tests/grad_norm_ref.py) against math.fsum, the
binding of the three entry points, their argument validation, the config key and the Lightning hook, the sequence of library calls an optimizer step
makes with and without a bound, and the host half of the entry points under ASan + UBSan (a stand-alone driver,
tests/sanitize/gradnorm_validation_driver.cpp)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.model_utils.optim import ExactDenseAdamW, FusedSparseAdagrad, FusedSparseAdam, SparseDenseAdam
from news_recsys_amd.model.sort.deep.model import Deep
from news_recsys_amd.model.sort.fm.model import FM
from tests import grad_norm_ref as G
from tests.conftest import CONFIGS, ROOT

ENTRY_POINTS = ("nrx_rows_sqnorm", "nrx_rows_sqnorm_finish", "nrx_rows_scale")


# ---- the restatement
@pytest.mark.parametrize("dim", [1, 6, 16, 112, 320])
def test_restatement_against_fsum(dim):
    """Every row sum is rounded once to fp32 -- 2^-24 = 6e-8 relative on the square -- and the double adds are negligible beside that: the norm is
    within 1e-6 relative of the exactly rounded one with more than 10x margin."""
    rng = np.random.default_rng(dim)
    n = 300
    g = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-12, 6, (n, 1)))).astype(np.float32)
    keys = np.array([(i % 3) << 40 | (i + 1) for i in range(n)], dtype=np.int64)
    norm, coef = G.finish(G.bins_of(keys, g, 3), 1.0)
    exact = math.sqrt(math.fsum(float(x) * float(x) for x in g.reshape(-1)))
    assert abs(norm - exact) <= 1e-6 * exact
    assert coef == np.float32(min(1.0, 1.0 / (norm + 1e-6)))


def test_restatement_bins_do_not_depend_on_order_or_split():
    rng = np.random.default_rng(5)
    g = rng.standard_normal((64, 8)).astype(np.float32)
    keys = np.arange(1, 65, dtype=np.int64)
    whole = G.bins_of(keys, g, 1)
    p = rng.permutation(64)
    assert G.bins_of(keys[p], g[p], 1) == whole
    assert G.bins_of(keys[40:], g[40:], 1, bins=G.bins_of(keys[:40], g[:40], 1)) == whole
    assert sum(whole) == sum(G.row_word(r)[1] for r in g)


def test_restatement_edges():
    z = np.zeros(8, np.float32)
    assert G.row_word(z) == (1, 0)
    tiny = np.full(8, 1e-23, np.float32)                   # the sum is a float denormal
    b, m = G.row_word(tiny)
    assert b == 1 and 0 < m < 0x800000
    assert G.row_word(np.full(8, 3e19, np.float32)) == (256, 1)          # 8 * 9e38 > FLT_MAX
    assert G.row_word(np.array([1, np.nan], np.float32)) == (257, 1)
    assert G.row_word(np.array([np.inf], np.float32)) == (256, 1)
    keys = np.array([1, 2], dtype=np.int64)
    norm, coef = G.finish(G.bins_of(keys, np.stack([np.full(8, 3e19, np.float32), z]), 1), 2.0)
    assert norm == math.inf and coef == 0
    norm, coef = G.finish(G.bins_of(keys[:1], np.array([[np.nan]], np.float32), 1), 2.0)
    assert math.isnan(norm) and math.isnan(float(coef))
    # keys that are not live: fillers, a table the call does not have, the padding row, a skipped table, an entry past the device-side count
    keys = np.array([-1, G.BIG, 3 << 40 | 5, 1 << 40, 2 << 40 | 7, 1 << 40 | 3, 9], dtype=np.int64)
    g = np.ones((7, 4), np.float32)
    bins = G.bins_of(keys, g, 3, n_dev=6, skip_tables=1 << 2)
    assert bins == G.bins_of(keys[5:6], g[5:6], 3) and sum(bins) == 0x800000
    assert [G.lanes_for(d) for d in (1, 4, 5, 16, 112, 256, 257, 320)] == [1, 1, 2, 4, 32, 64, 64, 64]


# ---- the binding
def test_binding_exposes_the_symbols_with_the_declared_argument_types():
    p, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    want = {"nrx_rows_sqnorm": [p, p, i64, p, i32, i32, u64, p, p],
            "nrx_rows_sqnorm_finish": [p, p, f64, p, p, i32, p],
            "nrx_rows_scale": [p, i64, i32, p, p]}
    names = {"nrx_rows_sqnorm": ["uniq_keys", "grads", "n", "n_dev", "n_tables", "dim", "skip_tables", "bins", "stream"],
             "nrx_rows_sqnorm_finish": ["bins", "extra_sq_dev", "max_norm", "norm_out", "coef_out", "rearm", "stream"],
             "nrx_rows_scale": ["values", "n", "dim", "coef_dev", "stream"]}
    ctype = {"int32_t": i32, "int64_t": i64, "uint64_t": u64, "double": f64}
    txt = open(os.path.join(ROOT, "include", "nrx_embed.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want[name]
        decl = re.search(r"NRX_API int %s\((.*?)\);" % name, txt, flags=re.S).group(1)
        declared = [a.strip().rsplit(" ", 1) for a in decl.split(",")]
        assert [n for _, n in declared] == names[name]
        for (ty, _), got in zip(declared, args):
            assert got is (p if ty.endswith("*") else ctype[ty]), (name, ty, got)
        assert getattr(lib, name).argtypes == args
    assert _lib.NRX_ABI_VERSION == 3                       # additive: the ABI version stays


def test_bad_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    for n, n_tables, dim in ((4, 0, 16), (4, 65, 16), (4, 1, 0), (-1, 1, 16)):
        rc = lib.nrx_rows_sqnorm(64, 64, n, None, n_tables, dim, 0, 64, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"bad argument" in lib.nrx_last_error()
    for keys, grads, bins in ((None, 64, 64), (64, None, 64), (64, 64, None)):
        rc = lib.nrx_rows_sqnorm(keys, grads, 4, None, 1, 16, 0, bins, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"null buffer" in lib.nrx_last_error()
    assert lib.nrx_rows_sqnorm(64, 66, 4, None, 1, 16, 0, 64, None) == _lib.NRX_ERR_BAD_ARG and b"misaligned" in lib.nrx_last_error()
    assert lib.nrx_rows_sqnorm(64, 64, 0, None, 1, 16, 0, 64, None) == 0               # an empty list
    for max_norm in (0.0, -2.0, math.nan):
        rc = lib.nrx_rows_sqnorm_finish(64, None, max_norm, 64, 64, 1, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"max_norm" in lib.nrx_last_error()
    for bins, norm, coef in ((None, 64, 64), (64, None, 64), (64, 64, None)):
        rc = lib.nrx_rows_sqnorm_finish(bins, None, 1.0, norm, coef, 0, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"null buffer" in lib.nrx_last_error()
    for n, dim in ((4, 0), (-1, 16)):
        rc = lib.nrx_rows_scale(64, n, dim, 64, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"bad argument" in lib.nrx_last_error()
    for values, coef in ((None, 64), (64, None)):
        rc = lib.nrx_rows_scale(values, 4, 16, coef, None)
        assert rc == _lib.NRX_ERR_BAD_ARG and b"null buffer" in lib.nrx_last_error()
    assert lib.nrx_rows_scale(64, 0, 16, 64, None) == 0
    with pytest.raises(ValueError, match="max_norm"):
        _lib.check(lib.nrx_rows_sqnorm_finish(64, None, 0.0, 64, 64, 1, None), "nrx_rows_sqnorm_finish")


# ---- the optimizers
def _tables():
    return [torch.zeros(8, 4), torch.zeros(5, 4)]


def test_optimizers_take_and_check_the_bound():
    for cls in (FusedSparseAdam, FusedSparseAdagrad):
        o = cls(ops.SparseGradSink(), lr=0.1)
        assert o.max_grad_norm is None and o.norm_group is None and o.norm_skip is None and o.grad_norm is None and o.clip_coef is None
        o = cls(ops.SparseGradSink(), lr=0.1, max_grad_norm=2)
        assert o.max_grad_norm == 2.0
        o.set_max_grad_norm(0.5)
        assert o.max_grad_norm == 0.5
        o.set_max_grad_norm(None)
        assert o.max_grad_norm is None
        for bad in (0, -1.0, math.nan):
            with pytest.raises(ValueError, match="max_grad_norm"):
                o.set_max_grad_norm(bad)
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(ops.SparseGradSink(), lr=0.1, max_grad_norm=bad)
    tabs = _tables()
    o = ExactDenseAdamW(ops.SparseGradSink(), tabs, max_grad_norm=3.0, norm_skip=[tabs[1]])
    assert o.max_grad_norm == 3.0 and o.norm_skip[0] is tabs[1]


def test_sparse_dense_adam_passes_the_bound_on_and_refuses_it_without_the_sink():
    tabs = [t.requires_grad_(True) for t in _tables()]
    with pytest.raises(ValueError, match="max_grad_norm"):
        SparseDenseAdam(tabs, [torch.zeros(3, requires_grad=True)], max_grad_norm=1.0)
    for kw, cls in ((dict(), FusedSparseAdam), (dict(exact=True), ExactDenseAdamW), (dict(table_optimizer="rowwise_adagrad"), FusedSparseAdagrad)):
        opt = SparseDenseAdam(tabs, [torch.zeros(3, requires_grad=True)], fused_sink=ops.SparseGradSink(), max_grad_norm=1.5, norm_skip=[tabs[0]], **kw)
        assert type(opt._sparse) is cls and opt.max_grad_norm == 1.5 and opt._sparse.max_grad_norm == 1.5 and opt._sparse.norm_skip[0] is tabs[0]
        opt.set_max_grad_norm(None)
        assert opt.max_grad_norm is None
    opt = SparseDenseAdam(tabs, [], fused_sink=ops.SparseGradSink())
    assert opt.max_grad_norm is None and opt.grad_norm is None and opt.clip_coef is None
    with pytest.raises(ValueError, match="max_grad_norm"):
        SparseDenseAdam(tabs, []).set_max_grad_norm(1.0)


class _FakeLib:
    """Records the names of the library calls an optimizer step makes; every call succeeds.  refuse: names that raise."""

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], set(refuse)

    def __getattr__(self, name):
        if not name.startswith("nrx_"):
            raise AttributeError(name)

        def call(*args):
            if name in self.refuse:
                raise AssertionError(f"{name} called")
            self.calls.append(name)
            return 0
        return call


class _Stream:
    cuda_stream = 0


def _entry(tabs, dim, keys):
    k = torch.tensor(keys, dtype=torch.int64)
    return dict(tables=tabs, dim=dim, uniq=k, values=torch.ones(len(keys), dim), counts=torch.tensor([len(keys)]), cap=len(keys))


def _make(kind, tabs, **kw):
    sink = ops.SparseGradSink()
    if kind == "adam":
        return FusedSparseAdam(sink, lr=0.1, **kw)
    if kind == "adagrad":
        return FusedSparseAdagrad(sink, lr=0.1, rowwise=False, **kw)
    if kind == "rowwise":
        return FusedSparseAdagrad(sink, lr=0.1, **kw)
    return ExactDenseAdamW(sink, tabs, **kw)


UPDATE = {"adam": ["nrx_sparse_adam_step"], "adagrad": ["nrx_sparse_adagrad_step"], "rowwise": ["nrx_sparse_adagrad_step"],
          "exact": ["nrx_rows_mark", "nrx_dense_adamw_rows"]}


@pytest.mark.parametrize("kind", ["adam", "adagrad", "rowwise", "exact"])
def test_without_a_bound_no_new_entry_point_is_called_and_with_one_the_phases_run_in_order(kind, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: _Stream())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    tabs = _tables()
    fake = _FakeLib(refuse=ENTRY_POINTS)
    monkeypatch.setattr(_lib, "_lib", fake)
    opt = _make(kind, tabs)
    opt.sink.pending.append(_entry(tabs, 4, [1, 2, (1 << 40) | 3]))
    opt.step()
    assert fake.calls == UPDATE[kind] and not opt.sink.pending and opt.grad_norm is None
    # ... two backward groups on one width: the pair merge of the fused optimizers, then one update per list
    fake.calls.clear()
    opt.sink.pending.extend([_entry(tabs, 4, [1, 2]), _entry(tabs, 4, [2, 3])])
    opt.step()
    pair = ["nrx_rows_mark", "nrx_rows_merge", "nrx_rows_mark"]
    assert fake.calls == (UPDATE[kind] if kind == "exact" else pair + UPDATE[kind] * 2)
    # ---- with a bound: merge, norm over every list, finish, scale, updates
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "_lib", fake)
    opt = _make(kind, tabs, max_grad_norm=1.0)
    opt.sink.pending.append(_entry(tabs, 4, [1, 2, (1 << 40) | 3]))
    opt.step()
    assert fake.calls == ["nrx_rows_sqnorm", "nrx_rows_sqnorm_finish", "nrx_rows_scale"] + UPDATE[kind]
    assert opt.grad_norm.dtype is torch.float64 and tuple(opt.grad_norm.shape) == (1,)
    assert opt.clip_coef.dtype is torch.float32 and tuple(opt.clip_coef.shape) == (1,) and not opt.sink.pending
    fake.calls.clear()
    opt.sink.pending.extend([_entry(tabs, 4, [1, 2]), _entry(tabs, 4, [2, 3])])
    opt.step()
    if kind == "exact":         # (its own merge: one list per width)
        assert fake.calls == ["nrx_rows_sqnorm", "nrx_rows_sqnorm_finish", "nrx_rows_scale"] + UPDATE[kind]
    else:                       # the norm is taken AFTER the merge
        assert fake.calls == pair + ["nrx_rows_sqnorm"] * 2 + ["nrx_rows_sqnorm_finish"] + ["nrx_rows_scale"] * 2 + UPDATE[kind] * 2
    # the bound taken away again: today's sequence
    opt.set_max_grad_norm(None)
    fake.refuse = set(ENTRY_POINTS)
    fake.calls.clear()
    opt.sink.pending.append(_entry(tabs, 4, [1]))
    opt.step()
    assert fake.calls == UPDATE[kind]


def test_sparse_dense_adam_clips_the_dense_part_between_the_phases(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: _Stream())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "_lib", fake)
    tabs = _tables()
    w = torch.ones(3, requires_grad=True)
    opt = SparseDenseAdam(tabs, [w], lr=0.5, fused_sink=ops.SparseGradSink(), max_grad_norm=1.0)
    opt._sparse.sink.pending.append(_entry(tabs, 4, [1, 2]))
    w.grad = torch.full((3,), 2.0)
    seen = {}
    real = opt._sparse.finish_norm

    def finish(extra=None):
        seen["extra"] = extra.clone()
        real(extra)
        opt._sparse.clip_coef.fill_(0.25)          # (the fake library computes nothing)
    monkeypatch.setattr(opt._sparse, "finish_norm", finish)
    opt.step()
    assert fake.calls == ["nrx_rows_sqnorm", "nrx_rows_sqnorm_finish", "nrx_rows_scale", "nrx_sparse_adam_step"]
    assert seen["extra"].dtype is torch.float64 and tuple(seen["extra"].shape) == (1,) and seen["extra"].item() == pytest.approx(12.0)
    assert torch.equal(w.grad, torch.full((3,), 0.5))                      # the dense gradients scaled by the coefficient, on the device
    assert not torch.equal(w.detach(), torch.ones(3))                      # ... and the dense AdamW stepped


# ---- the config key and the hook
def write_cfg(tmp_path, name, hp=None, **emb):
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, name)))
    cfg["embeddings"].update(emb)
    cfg["train_hparams"].update(hp or {})
    p = tmp_path / ("clip_" + name)
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


@pytest.mark.parametrize("sg", [False, True])
def test_config_refuses_the_key_outside_the_sink_modes(tmp_path, sg):
    with pytest.raises(ValueError, match=r"max_grad_norm.*sparse_grad"):
        FM(write_cfg(tmp_path, "cf_fm_small.yaml", hp=dict(max_grad_norm=1.0), sparse_grad=sg))


@pytest.mark.parametrize("bad", [0, -1.0])
def test_config_refuses_a_bound_that_is_not_positive(tmp_path, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        FM(write_cfg(tmp_path, "cf_fm_small.yaml", hp=dict(max_grad_norm=bad), sparse_grad="fused"))


@pytest.mark.parametrize("sg,cls", [("fused", FusedSparseAdam), ("exact", ExactDenseAdamW)])
def test_config_key_reaches_the_optimizer(tmp_path, sg, cls):
    m = Deep(write_cfg(tmp_path, "cf_array_small.yaml", hp=dict(max_grad_norm=0.75), sparse_grad=sg))
    assert m.max_grad_norm == 0.75
    opt = m.configure_optimizers()["optimizer"]
    assert type(opt._sparse) is cls and opt.max_grad_norm == 0.75 and opt._sparse.norm_group is None and opt._sparse.norm_skip is None
    d = Deep(write_cfg(tmp_path, "cf_array_small.yaml", sparse_grad=sg))
    assert d.max_grad_norm is None and d.configure_optimizers()["optimizer"].max_grad_norm is None          # the default is untouched


def test_dssm_refuses_the_key(tmp_path):
    from news_recsys_amd.model.recall.DSSM.model import DSSM
    m = DSSM(write_cfg(tmp_path, "cf_dssm_small.yaml", hp=dict(max_grad_norm=1.0), sparse_grad="fused"))
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        m.configure_optimizers()


def test_hook_sets_the_optimizer_and_refuses_clipping_by_value(tmp_path):
    m = Deep(write_cfg(tmp_path, "cf_array_small.yaml", sparse_grad="fused"))
    opt = m.configure_optimizers()["optimizer"]
    m.configure_gradient_clipping(opt, gradient_clip_val=None)
    assert opt.max_grad_norm is None
    m.configure_gradient_clipping(opt, gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    assert opt.max_grad_norm == 0.5
    with pytest.raises(NotImplementedError, match="value"):
        m.configure_gradient_clipping(opt, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    with pytest.raises(NotImplementedError, match="configure_optimizers"):
        m.configure_gradient_clipping(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1), gradient_clip_val=0.5)


def test_hook_in_the_dense_gradient_mode_clips_the_grad_tensors_without_lightning(tmp_path, monkeypatch):
    from news_recsys_amd import lightning_shim
    monkeypatch.setattr(lightning_shim, "HAVE_LIGHTNING", False)
    m = Deep(write_cfg(tmp_path, "cf_array_small.yaml"))
    opt = m.configure_optimizers()["optimizer"]
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    total = math.sqrt(sum(p.numel() for p in m.parameters()))
    m.configure_gradient_clipping(opt, gradient_clip_val=1.0)
    got = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in m.parameters()))
    assert total > 10 and got == pytest.approx(1.0, rel=1e-4)


def test_hook_in_the_dense_gradient_mode_defers_to_lightning_when_it_is_there(tmp_path, monkeypatch):
    """The Lightning branch: the parent's hook gets the arguments unchanged and nothing is clipped here (a stub stands in for
    LightningModule.configure_gradient_clipping, which needs a Trainer)."""
    from news_recsys_amd import lightning_shim
    seen = []
    monkeypatch.setattr(lightning_shim, "HAVE_LIGHTNING", True)
    monkeypatch.setattr(lightning_shim.LightningModule, "configure_gradient_clipping",
                        lambda self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None:
                        seen.append((self, optimizer, gradient_clip_val, gradient_clip_algorithm)), raising=False)
    m = Deep(write_cfg(tmp_path, "cf_array_small.yaml"))
    opt = m.configure_optimizers()["optimizer"]
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    m.configure_gradient_clipping(opt, gradient_clip_val=1.0, gradient_clip_algorithm="value")
    assert seen == [(m, opt, 1.0, "value")]
    assert all(torch.equal(p.grad, torch.ones_like(p)) for p in m.parameters())


def test_a_norm_skip_tensor_is_found_by_its_storage_and_an_unknown_one_is_an_error():
    tabs = _tables()
    o = FusedSparseAdam(ops.SparseGradSink(), lr=0.1, params=tabs, norm_skip=[tabs[1].data])       # another object over the same memory
    assert o._skip_mask() == 0                              # known to `params`, not registered yet: absent from this step, no error
    o._register(tabs[0])
    o._register(tabs[1])
    assert o._skip_mask() == 1 << 1
    o.norm_skip = [tabs[0]]
    assert o._skip_mask() == 1 << 0
    o.norm_skip = [torch.zeros(5, 4)]
    with pytest.raises(ValueError, match="norm_skip"):
        o._skip_mask()
    with pytest.raises(ValueError, match="norm_skip"):
        FusedSparseAdam(ops.SparseGradSink(), lr=0.1, norm_skip=[tabs[0]])._skip_mask()               # no params, nothing registered


# ---- the host half of the entry points under ASan + UBSan: a stand-alone driver with its own main, run directly
def test_gradnorm_host_validation_is_clean_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    if not os.path.exists(os.path.join(ROOT, "tests", "sanitize", "gradnorm.mk")):
        pytest.skip("tests/sanitize/ is not part of this tree (it does not travel to the GPU machines)")
    p = subprocess.run(["make", "-C", "tests/sanitize", "-f", "gradnorm.mk", "run"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert "nrx_rows_sqnorm validation sanitize driver: OK" in out
