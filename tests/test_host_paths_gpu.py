"""Both host bindings of the embedding call, and table sets that change between two calls.

ops.embed_apply reaches nrx_embed_fwd_train through the compiled binding (csrc/nrx_bind.cpp: BoundPlan.forward) or through ctypes
(ops._FastForward, ops._EmbedFn._forward_ctypes).  Each validates the batch, refreshes the descriptors, allocates the outputs and reads the
status on its own; which one runs depends on what loaded and on what the batch looks like.  Here every launch runs through BOTH inside one
process (the module global ops._BIND chooses: False = ctypes, None = look again), a spy says which one really ran, and the results are

  * word for word equal between the two: one entry point, descriptors that must be identical, deterministic kernels -- no tolerance;
  * checked against float64: single-valued columns are copies (bit for bit), pooled columns rtol 1e-6 / atol 1e-6, the FM logit rtol 1e-5 /
    atol 1e-5, and everything -- gradients included -- within embed_cases' bound C * n * 2^-24 * A;
  * equal to ops.PreparedEmbed's, which takes neither path.

The plans: the generated seeds the binding can serve (chosen by predicate: tests/test_host_paths.py) and hand-made ones for what those lack,
first of all the 26-feature all-ids plan, the only shape that takes _FastForward's all-ids branch.  The hand-made tables hold N(0, 1/16)
values: the FM logit's own float32 rounding grows with the square of the values (26 fields of N(0, 1) leave ~1e-5 absolute on a logit that
may cancel to zero); at a quarter of the scale it is ~1e-6, a tenth of the absolute bar, so that the bar tests the kernel and not the
draw.  Batches the binding declines must end the same way -- the same tensors or the same exception -- whether or not it is loaded.

Then the table set changes under a plan that stays: one table of the list swapped (first, middle, last), the middle one grown, shrunk,
or converted to bf16 -- at ops level in every backward mode, and through the model (a Parameter's .data swapped, a Parameter replaced).
Every replaced tensor stays referenced until its test ends: a stale descriptor reads old values from live memory, never freed memory."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from news_recsys_amd._lib import (NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM, NRX_DENSE, NRX_FEAT_BAG_CSR, NRX_FEAT_TABLE_BF16,
                                  NRX_SPARSE, NrxError)
from tests import embed_cases as E
from tests.conftest import CONFIGS
from tests.test_host_paths import servable_seeds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASK = (1 << 40) - 1
PATHS = ("ctypes", "binding")
SCALE = 0.25                       # the hand-made tables' values (see the module's docstring)


# ------------------------------------------------------------------------------------------------- A. choosing the host path
def _binding_files():
    from news_recsys_amd import ops
    return glob.glob(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "lib", "nrx_bind*.so"))


class _Seen:
    """What the ctypes layer did since the leg began (its two entry points are wrapped), and every answer of BoundPlan.forward."""

    def __init__(self):
        self.bind_tables = 0           # _FastForward._bind_tables: only the ctypes branch of the no-grad form binds
        self.forward_ctypes = 0        # _EmbedFn._forward_ctypes: the training form's ctypes launch
        self.bound = []                # results of BoundPlan.forward (watch())

    def ctypes_work(self):
        return self.bind_tables + self.forward_ctypes


class _BoundSpy:
    def __init__(self, bp, seen):
        self.bp, self.seen = bp, seen

    def forward(self, *a):
        try:
            r = self.bp.forward(*a)
        except Exception as e:           # noqa: BLE001 -- recorded, and the caller's to see
            self.seen.bound.append(e)
            raise
        self.seen.bound.append(r)
        return r


def _host_path(monkeypatch, path):
    """Make `path` the host path of every plan built from here on (fresh plans only: a plan keeps _bound / _fast / _arr_cache / _sg)."""
    from news_recsys_amd import ops
    monkeypatch.delenv("NRX_NO_BIND", raising=False)
    if path == "ctypes":
        monkeypatch.setattr(ops, "_BIND", False)
        assert ops._binding() is None
    else:
        if not _binding_files():
            pytest.skip("no compiled host binding under news_recsys_amd/lib: the binding leg is not run (the ctypes leg is)")
        monkeypatch.setattr(ops, "_BIND", None)
        assert ops._binding() is not None, f"{_binding_files()[0]} is there but does not load: the suite would silently test ctypes only"
    seen = _Seen()
    orig_bt, orig_fc = ops._FastForward._bind_tables, ops._EmbedFn._forward_ctypes

    def bind_tables(self, tables):
        seen.bind_tables += 1
        return orig_bt(self, tables)

    def forward_ctypes(*a):
        seen.forward_ctypes += 1
        return orig_fc(*a)

    monkeypatch.setattr(ops._FastForward, "_bind_tables", bind_tables)
    monkeypatch.setattr(ops._EmbedFn, "_forward_ctypes", staticmethod(forward_ctypes))
    return seen


def _watch(plan, seen):
    """Record what the plan's BoundPlan answers (binding leg; a no-op on the ctypes leg, whose plans have none)."""
    from news_recsys_amd import ops
    bp = ops._bound_plan(plan)
    if bp is not None and not isinstance(bp, _BoundSpy):
        plan.__dict__["_bound"] = _BoundSpy(bp, seen)
    return plan


def _ran_on(path, seen, plan, served=True):
    """The leg really took `path` (served=False: a batch the binding hands back -- asked, answered None, and ctypes did the work)."""
    if path == "ctypes":
        assert plan.__dict__.get("_bound", None) is None and not seen.bound
        assert seen.ctypes_work() > 0, "the ctypes leg did no ctypes work"
    elif not served:
        assert seen.bound and all(r is None for r in seen.bound), f"the binding was expected to decline: {seen.bound}"
        assert seen.ctypes_work() > 0
    else:
        assert seen.bound and all(type(r) is tuple for r in seen.bound), f"the binding declined or failed: {seen.bound}"
        assert seen.ctypes_work() == 0, "the binding leg fell back to ctypes"


def test_a_built_binding_loads(monkeypatch):
    """Where build() left the binding, it must load: ops._binding() swallows every load error and the package goes on through ctypes."""
    from news_recsys_amd import ops
    files = _binding_files()
    if not files:
        pytest.skip("no compiled host binding under news_recsys_amd/lib")
    monkeypatch.delenv("NRX_NO_BIND", raising=False)
    monkeypatch.setattr(ops, "_BIND", None)
    mod = ops._binding()
    assert mod is not None and hasattr(mod, "BoundPlan"), f"{files[0]} does not load"
    monkeypatch.setattr(ops, "_BIND", False)
    assert ops._binding() is None


# ------------------------------------------------------------------------------------------------- helpers
def _words(t):
    return t.detach().contiguous().view(torch.int32)


def _same_words(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} != {tuple(b.shape)} {b.dtype}"
        assert torch.equal(_words(a), _words(b)), f"{what}: the two differ in {int((_words(a) != _words(b)).sum())} words"


def _set_knobs(monkeypatch, case):
    from news_recsys_amd import ops
    for k, v in case.knobs.items():
        monkeypatch.setattr(ops, k, v)


def _dev_inputs(case):
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in case.inputs]
    ws = [None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(DEV) for w in case.weights]
    return ins, ws


def _dev_tables(case, requires_grad=False):
    ts = []
    for t in case.tables:
        x = torch.from_numpy(t).to(DEV)
        if case.bf16:
            x = x.to(torch.bfloat16)                  # exact: the values are bf16 values
        ts.append(x.requires_grad_(requires_grad))
    return ts


def _sink_dense(pending, shapes):
    """A sink's entries scattered into dense float32 gradients (keys: launch-local table << 40 | row)."""
    grads = [torch.zeros(tuple(s), dtype=torch.float32, device=DEV) for s in shapes]
    for e in pending:
        keys = e["uniq"]
        valid = (keys >= 0) if e.get("filler") else (torch.arange(keys.numel(), device=DEV) < e["counts"][0])
        k = keys[valid]
        v = e["values"][:keys.numel()][valid]
        assert torch.unique(k).numel() == k.numel(), "a key appears twice in one sink entry"
        t, r = k >> 40, k & MASK
        for ti in torch.unique(t).tolist():
            sel = t == ti
            grads[ti].index_put_((r[sel],), v[sel], accumulate=True)
    return grads


def _make_case(name, B, slots, rows, rng, use_fm=False, bf16=False, id_dtype=np.int64, out_ld=None, narrow=False):
    """A hand-made launch as an embed_cases.Case (columns laid out in slot order), so that its float64 restatement and bound serve."""
    col = wide_w = 0
    for s in slots:
        s.out_col = col
        col += s.dim - (1 if s.wide_col >= 0 else 0)
        wide_w = max(wide_w, s.wide_col + 1)
        if bf16 and s.kind != NRX_DENSE:
            s.flags |= NRX_FEAT_TABLE_BF16
    dims = {}
    for s in slots:
        if s.kind != NRX_DENSE:
            dims[s.table] = s.dim
    tables = []
    for t, r in enumerate(rows):
        x = (rng.standard_normal((r, dims[t])) * SCALE).astype(np.float32)
        tables.append(E._bf16_exact(x) if bf16 else x)
    inputs, weights = [], []
    for s in slots:
        if s.kind == NRX_DENSE:
            inputs.append(rng.standard_normal(B).astype(np.float32))
            weights.append(None)
        elif s.bag_len == 0:
            inputs.append(E._ids(rng, rows[s.table], (B,), False).astype(id_dtype))
            weights.append(None)
        else:
            x = E._ids(rng, rows[s.table], (B, s.bag_len), False)
            valid = np.arange(s.bag_len)[None, :] < rng.integers(0, s.bag_len + 1, (B, 1))          # empty bags included
            if s.kind == NRX_BAG_MASKED_MEAN:
                inputs.append((x * valid).astype(id_dtype))
                weights.append(valid.astype(np.float32))
            else:
                inputs.append(x.astype(id_dtype))
                weights.append(None)
    ld = out_ld or col
    case = E.Case(-1, name, B, slots, col, ld, narrow, wide_w, use_fm, bf16, tables, inputs, weights,
                  rng.standard_normal((B, ld)).astype(np.float32),
                  rng.standard_normal((B, wide_w)).astype(np.float32) if wide_w else None,
                  rng.standard_normal(B).astype(np.float32) if use_fm else None)
    case.knobs = dict(E.KNOB_DEFAULTS)
    return case


def _c2_mini(B, id_dtype, fm, seed=0):
    """C2 in miniature: 26 single-valued features of D = 16 over 26 tables of 40-300 rows (the all-ids shape of the flagship workload)."""
    rng = np.random.default_rng([26, B, int(fm), seed])
    rows = [int(r) for r in rng.integers(40, 301, 26)]
    slots = [E.SlotSpec(f"C{i:02d}", NRX_SPARSE, i, 16, fm_field=int(fm)) for i in range(26)]
    return _make_case(f"c2_mini{'_fm' if fm else ''}", B, slots, rows, rng, use_fm=fm, id_dtype=id_dtype)


def _tower(B=257):
    rng = np.random.default_rng([3, B])
    slots = [E.SlotSpec("user_id", NRX_SPARSE, 0, 16), E.SlotSpec("item_id", NRX_SPARSE, 1, 16),
             E.SlotSpec("history", NRX_BAG_MASKED_MEAN, 1, 16, 5)]
    return _make_case("tower", B, slots, [120, 211], rng)


def _wide_deep(B=257):
    """Wide&Deep: three of five features give their first column to the wide part; the row stride padded to 4 floats, narrow=True."""
    rng = np.random.default_rng([5, B])
    slots = [E.SlotSpec(f"w{i}", NRX_SPARSE, i, 8, wide_col=(i // 2 if i % 2 == 0 else -1)) for i in range(5)]
    return _make_case("wide_deep", B, slots, [40, 77, 130, 64, 300], rng, out_ld=40, narrow=True, id_dtype=np.int32)


def _bf16_set(B=65):
    rng = np.random.default_rng([16, B])
    slots = [E.SlotSpec("a", NRX_SPARSE, 0, 16), E.SlotSpec("b", NRX_SPARSE, 1, 32), E.SlotSpec("c", NRX_SPARSE, 0, 16),
             E.SlotSpec("m", NRX_BAG_MEAN, 1, 32, 3)]
    return _make_case("bf16_set", B, slots, [90, 150], rng, bf16=True)


HAND_MADE = {}
for _B in (1, 65, 257):
    for _dt in (np.int32, np.int64):
        for _fm in (False, True):
            HAND_MADE[f"c2_mini{'_fm' if _fm else ''}-B{_B}-{np.dtype(_dt).name}"] = (lambda B=_B, dt=_dt, fm=_fm: _c2_mini(B, dt, fm))
HAND_MADE["tower"] = _tower
HAND_MADE["wide_deep"] = _wide_deep
HAND_MADE["bf16_set"] = _bf16_set


# ------------------------------------------------------------------------------------------------- B. the two layers, every form
def _forms_of(case):
    return ("nograd", "sink") if case.bf16 else ("nograd", "coo", "sink")      # (bf16 tables train only through the sink)


def _run_form(case, form, seen):
    """One launch of the case in `form` with a fresh plan; (plan, {name: tensor})."""
    from news_recsys_amd import ops
    plan = _watch(case.plan(), seen)
    ins, ws = _dev_inputs(case)
    W = case.out_width
    res = {}
    if form == "nograd":
        tabs = _dev_tables(case)
        with torch.no_grad():
            out, wide, fm = ops.embed_apply(plan, tabs, ins, ws, out_ld=case.out_ld, narrow=case.narrow)
    else:
        tabs = _dev_tables(case, requires_grad=True)
        sink = ops.SparseGradSink() if form == "sink" else None
        out, wide, fm = ops.embed_apply(plan, tabs, ins, ws, out_ld=case.out_ld, narrow=case.narrow, sparse_grad=sink if sink is not None else True)
        g_out = torch.from_numpy(case.g_out).to(DEV)
        if case.narrow:
            g_out = g_out[:, :W].contiguous()
        outs, ups = [out], [g_out]
        if wide is not None:
            outs.append(wide)
            ups.append(torch.from_numpy(case.g_wide).to(DEV))
        if fm is not None:
            outs.append(fm)
            ups.append(torch.from_numpy(case.g_fm).to(DEV))
        res["has_fm_sums"] = out.grad_fn.fm_sums is not None
        torch.autograd.backward(outs, ups)
        if sink is not None:
            assert all(t.grad is None for t in tabs)
            grads = _sink_dense(sink.pending, [t.shape for t in tabs])
        else:
            grads = [t.grad.to_dense() for t in tabs]
        for t, g in enumerate(grads):
            res[f"grad{t}"] = g
    assert out.shape == (case.B, W if case.narrow else case.out_ld)
    res["out"] = out.detach()[:, :W]
    if wide is not None:
        res["wide"] = wide.detach()
    if fm is not None:
        res["fm"] = fm.detach()
    torch.cuda.synchronize()
    return plan, res


def _against_float64(case, res, ref, form, hand_made):
    out = res["out"]
    cc = ref.copy_cols
    if cc:
        assert torch.equal(out[:, cc], ref.out[:, cc].float()), f"{form}: a single-valued column is not table[ids]\n{case.spec()}"
    for name, r64, A, n in (("out", ref.out, ref.A_out, ref.n_out), ("wide", ref.wide, ref.A_wide, ref.n_out), ("fm", ref.fm, ref.A_fm, ref.n_fm)):
        if r64 is None:
            continue
        ex, i = E.excess(res[name], r64, A, n)
        print(f"{case.style} {form} {name}: max |err| {float((res[name].double() - r64).abs().max()):.3g}  excess {ex:.3g}")
        assert ex <= 0, f"{form} {name}: element {i} beyond the bound by {ex:.3g}\n{case.spec()}"
    if case.wide_width and ref.wide_copy_cols:
        wc = ref.wide_copy_cols
        assert torch.equal(res["wide"][:, wc], ref.wide[:, wc].float()), f"{form}: a wide column of a single-valued feature is not a copy"
    if hand_made:                                    # the project's bars for pooled columns and the FM logit
        torch.testing.assert_close(out.double(), ref.out, rtol=1e-6, atol=1e-6)
        if case.use_fm:
            torch.testing.assert_close(res["fm"].double(), ref.fm, rtol=1e-5, atol=1e-5)
    if form != "nograd":
        for t in range(len(case.tables)):
            g = res[f"grad{t}"]
            ex, i = E.excess(g, ref.grads[t], ref.A_grads[t], ref.n_grads[t])
            assert ex <= 0, f"{form}: gradient of table {t}: element {i} beyond the bound by {ex:.3g}\n{case.spec()}"
            assert float(g[0].abs().max()) == 0.0, f"{form}: the padding row of table {t} has a gradient"
            assert bool((g[ref.A_grads[t] == 0] == 0).all()), f"{form}: a row that was not looked up has a gradient (table {t})"


def _binding_serves(case):
    """Beyond the predicate of the seed selection the binding hands back one more kind of launch: a sum bag without weights."""
    return not any(s.kind == NRX_BAG_SUM and w is None for s, w in zip(case.slots, case.weights))


def _one_leg(case, path, monkeypatch):
    """Every form of the case on one host path: {form: results}; the spy has confirmed the path."""
    out = {}
    for form in _forms_of(case):
        with monkeypatch.context() as mp:
            seen = _host_path(mp, path)
            plan, out[form] = _run_form(case, form, seen)
            _ran_on(path, seen, plan, served=_binding_serves(case))
    return out


def _both_layers(case, path, monkeypatch, hand_made):
    from news_recsys_amd import ops
    _set_knobs(monkeypatch, case)
    ref = E.restate(case, DEV)
    legs = {path: _one_leg(case, path, monkeypatch)}
    for form, res in legs[path].items():
        _against_float64(case, res, ref, form, hand_made)
    # the third opinion: a bound launch, which takes neither path
    ins, ws = _dev_inputs(case)
    pre = ops.PreparedEmbed(case.plan(), _dev_tables(case), ins, ws, out_ld=case.out_ld).run()
    torch.cuda.synchronize()
    names = ("out", "wide", "fm")
    prepared = {"out": pre[0][:, :case.out_width], "wide": pre[1], "fm": pre[2]}
    for form, res in legs[path].items():
        for nm in names:
            _same_words(res.get(nm), prepared[nm], f"{path} {form} vs PreparedEmbed ({nm})\n{case.spec()}")
    if path == "binding":                               # the binding leg also runs the other layer and compares word for word
        legs["ctypes"] = _one_leg(case, "ctypes", monkeypatch)
        for form in _forms_of(case):
            a, b = legs["binding"][form], legs["ctypes"][form]
            assert a.keys() == b.keys(), (form, sorted(a), sorted(b))
            for nm in a:
                if nm == "has_fm_sums":
                    assert a[nm] == b[nm], f"{form}: the field sums are kept on one path only"
                else:
                    _same_words(a[nm], b[nm], f"binding vs ctypes, {form} ({nm})\n{case.spec()}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("seed", servable_seeds())
def test_generated_seed_on_both_host_paths(seed, path, monkeypatch):
    _both_layers(E.make_case(seed), path, monkeypatch, hand_made=False)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_plan_on_both_host_paths(name, path, monkeypatch):
    _both_layers(HAND_MADE[name](), path, monkeypatch, hand_made=True)


def test_all_ids_plan_takes_the_all_ids_branch(monkeypatch):
    """The premise of the 26-feature plans: without the binding the no-grad form runs _FastForward's all-ids branch (no _prep_inputs)."""
    from news_recsys_amd import ops
    case = _c2_mini(65, np.int64, True)
    seen = _host_path(monkeypatch, "ctypes")
    calls = []
    orig = ops._prep_inputs
    monkeypatch.setattr(ops, "_prep_inputs", lambda *a: calls.append(1) or orig(*a))
    plan = case.plan()
    ins, ws = _dev_inputs(case)
    with torch.no_grad():
        ops.embed_apply(plan, _dev_tables(case), ins, ws)
    assert plan.__dict__["_fast"].simple and seen.bind_tables == 1 and not calls


def _legs(path):
    return ("ctypes",) if path == "ctypes" else ("binding", "ctypes")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "train"])
def test_fm_without_the_concat(grad, path, monkeypatch):
    """need_out=False with the FM epilogue: only the logit comes back, the same words as with the concat, on both paths."""
    from news_recsys_amd import ops
    case = _c2_mini(65, np.int64, True, seed=1)
    ref = E.restate(case, DEV, grads=False)
    got = {}
    for leg in _legs(path):
        with monkeypatch.context() as mp:
            seen = _host_path(mp, leg)
            plan = _watch(case.plan(), seen)
            ins, ws = _dev_inputs(case)
            tabs = _dev_tables(case, requires_grad=grad)
            with torch.set_grad_enabled(grad):
                out, wide, fm = ops.embed_apply(plan, tabs, ins, ws, need_out=False)
                full = ops.embed_apply(case.plan(), tabs, ins, ws)[2]
            _ran_on(leg, seen, plan)
        assert out is None and wide is None and fm.shape == (case.B,)
        _same_words(fm, full, f"{leg}: fm without the concat vs with it")
        torch.testing.assert_close(fm.detach().double(), ref.fm, rtol=1e-5, atol=1e-5)
        got[leg] = fm.detach()
    if len(got) == 2:
        _same_words(got["binding"], got["ctypes"], "binding vs ctypes (fm, need_out=False)")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fm", [False, True], ids=["plain", "fm"])
def test_empty_batch(fm, path, monkeypatch):
    """B = 0: empty outputs of the right shapes, nothing launched, zero gradients -- on both paths."""
    from news_recsys_amd import ops
    case = _c2_mini(65, np.int64, fm)
    ins = [x[:0] for x in _dev_inputs(case)[0]]
    ws = [None] * len(ins)
    for leg in _legs(path):
        with monkeypatch.context() as mp:
            seen = _host_path(mp, leg)
            for grad in (False, True):
                plan = _watch(case.plan(), seen)
                tabs = _dev_tables(case, requires_grad=grad)
                with torch.set_grad_enabled(grad):
                    out, wide, fmv = ops.embed_apply(plan, tabs, ins, ws)
                assert out.shape == (0, case.out_width) and wide is None and ((fmv is None) if not fm else fmv.shape == (0,))
                if grad:
                    out.sum().backward()
                    torch.cuda.synchronize()
                    assert all(t.grad is None or float(t.grad.abs().max()) == 0.0 for t in tabs)
                _ran_on(leg, seen, plan)


@pytest.mark.parametrize("path", PATHS)
def test_index_check_modes_agree(path, monkeypatch):
    """sync, deferred and off: the same words for in-range ids, nothing pending afterwards -- on both paths."""
    from news_recsys_amd import ops
    case = _c2_mini(65, np.int32, True, seed=2)
    ops.flush_index_checks()
    got = {}
    for leg in _legs(path):
        for mode in ("sync", "deferred", "off"):
            for grad in (False, True):
                with monkeypatch.context() as mp:
                    seen = _host_path(mp, leg)
                    plan = _watch(case.plan(), seen)
                    ins, ws = _dev_inputs(case)
                    with torch.set_grad_enabled(grad):
                        res = ops.embed_apply(plan, _dev_tables(case, requires_grad=grad), ins, ws, index_check=mode)
                    _ran_on(leg, seen, plan)
                got[(leg, mode, grad)] = res
    ops.flush_index_checks()
    assert not ops.deferred_index_error_pending()
    first = next(iter(got.values()))
    for key, res in got.items():
        _same_words(res[0], first[0], f"{key} (concat)")
        _same_words(res[2], first[2], f"{key} (fm)")


# ------------------------------------------------------------------------------------------------- B. batches the binding declines
def _decl_plan(slots, **kw):
    from news_recsys_amd import ops
    col = 0
    out = []
    for name, kind, table, dim, L, flags in slots:
        out.append(ops.Slot(name, kind, table, dim, L, col, flags=flags))
        col += dim
    return ops.EmbedPlan(out, out_width=col, **kw)


class _Decl:
    """One batch the binding hands back (or answers as ctypes does): how to build it, what must come of it."""

    def __init__(self, build, raises=None, match=None, declined=True, mode=None, flush=False, derived_in_train=False):
        """declined: BoundPlan.forward is asked and answers None in both forms (else: it answers itself, or Python never asks it).
        derived_in_train: the training form launches a plan derived from this one (CSR bags expanded for the planner), with a BoundPlan of its own."""
        self.build, self.raises, self.match, self.declined, self.mode, self.flush = build, raises, match, declined, mode, flush
        self.derived_in_train = derived_in_train


def _base(B=33, seed=0, rows=(50, 70)):
    """Plan pieces shared by the declined batches: ids a -> T0, ids b -> T1, a masked-mean bag h (L = 4) -> T1, a dense value v."""
    g = torch.Generator().manual_seed(seed)
    T = [(torch.randn(r, 16, generator=g) * SCALE).to(DEV) for r in rows]
    a = torch.randint(0, rows[0], (B,), generator=g).to(DEV)
    b = torch.randint(0, rows[1], (B,), generator=g).to(DEV)
    h = torch.randint(1, rows[1], (B, 4), generator=g)
    m = (torch.arange(4)[None, :] < torch.randint(0, 5, (B, 1), generator=g)).float()
    v = torch.randn(B, generator=g).to(DEV)
    return T, a, b, (h * m.long()).to(DEV), m.to(DEV), v


_AB = [("a", NRX_SPARSE, 0, 16, 0, 0), ("b", NRX_SPARSE, 1, 16, 0, 0)]
_ABH = _AB + [("h", NRX_BAG_MASKED_MEAN, 1, 16, 4, 0)]
_ABV = _AB + [("v", NRX_DENSE, -1, 1, 0, 0)]


def _d_strided_ids():
    T, a, b, h, m, v = _base()
    two = torch.stack([a, b], 1).contiguous()                  # [B, 2]: each feature a strided column
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[two[:, 0], two[:, 1]], weights=[None, None]), dict(inputs=[a, b])


def _d_small_int_ids(dt):
    def build():
        T, a, b, h, m, v = _base()
        return dict(plan=_decl_plan(_AB), tables=T, inputs=[a.to(dt), b.to(dt)], weights=[None, None]), dict(inputs=[a, b])
    return build


def _d_dense_dtype(dt):
    def build():
        T, a, b, h, m, v = _base()
        x = v.to(dt)
        return dict(plan=_decl_plan(_ABV), tables=T, inputs=[a, b, x], weights=[None] * 3), dict(inputs=[a, b, x.float()])
    return build


def _d_mask_noncontig():
    T, a, b, h, m, v = _base()
    wide = torch.zeros(m.shape[0], 8, device=DEV)
    wide[:, ::2] = m
    return dict(plan=_decl_plan(_ABH), tables=T, inputs=[a, b, h], weights=[None, None, wide[:, ::2]]), dict(weights=[None, None, m])


def _d_mask_dtype():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_ABH), tables=T, inputs=[a, b, h], weights=[None, None, m.double()]), None


def _d_mask_shape():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_ABH), tables=T, inputs=[a, b, h], weights=[None, None, m[:, :3].contiguous()]), None


def _d_ids_rank():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[a, b[:, None].contiguous()], weights=[None, None]), None


def _d_different_B():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[a, b[:-1].contiguous()], weights=[None, None]), None


def _d_cpu_ids():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[a, b.cpu()], weights=[None, None]), None


def _d_masked_mean_without_mask():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_ABH), tables=T, inputs=[a, b, h], weights=[None, None, None]), None


def _d_sum_without_weights():
    T, a, b, h, m, v = _base()
    plan = _decl_plan(_AB + [("h", NRX_BAG_SUM, 1, 16, 4, 0)])
    ones = torch.ones_like(m)                                  # an unweighted sum is the sum with unit weights
    return dict(plan=plan, tables=T, inputs=[a, b, h], weights=[None, None, None]), dict(weights=[None, None, ones], close=True)


def _d_csr():
    T, a, b, h, m, v = _base()
    lens = m.sum(1).long()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), lens.cumsum(0)])
    vals = h[m.bool()]                                         # row-major: bag after bag, the valid entries of each
    plan = _decl_plan(_AB + [("h", NRX_BAG_MASKED_MEAN, 1, 16, 4, NRX_FEAT_BAG_CSR)])
    return (dict(plan=plan, tables=T, inputs=[a, b, vals], weights=[None, None, off]),
            dict(plan=_decl_plan(_ABH), inputs=[a, b, h], weights=[None, None, m], close=True))


def _d_tables_tuple():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=tuple(T), inputs=[a, b], weights=[None, None]), dict(tables=T)


def _d_out_ld_small():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[a, b], weights=[None, None], out_ld=31), None


def _d_bf16_without_flag():
    T, a, b, h, m, v = _base()
    return dict(plan=_decl_plan(_AB), tables=[T[0], T[1].to(torch.bfloat16)], inputs=[a, b], weights=[None, None]), None


def _d_out_of_range():
    T, a, b, h, m, v = _base()
    b = b.clone()
    b[7] = 70 + 5                                              # ONE offender: the library's bounds check clamps it to row 0 and reports
    return dict(plan=_decl_plan(_AB), tables=T, inputs=[a, b], weights=[None, None]), None


DECLINED = {
    "strided_ids": _Decl(_d_strided_ids),
    "int16_ids": _Decl(_d_small_int_ids(torch.int16)),
    "uint8_ids": _Decl(_d_small_int_ids(torch.uint8)),
    "float64_dense": _Decl(_d_dense_dtype(torch.float64), declined=False),       # (the binding reads a double dense value itself)
    "float16_dense": _Decl(_d_dense_dtype(torch.float16)),
    "noncontiguous_mask": _Decl(_d_mask_noncontig),
    "mask_dtype": _Decl(_d_mask_dtype, raises=TypeError, match="mask of 'h': expected float32"),
    "mask_shape": _Decl(_d_mask_shape, raises=ValueError, match="mask of 'h': shape"),
    "ids_rank": _Decl(_d_ids_rank, raises=ValueError, match="feature 'b': expected a 1-D"),
    "different_B": _Decl(_d_different_B, raises=ValueError, match="feature 'b': batch 32 != 33"),
    "cpu_ids": _Decl(_d_cpu_ids, raises=NrxError, match="feature 'b': expected a ROCm device tensor"),
    "masked_mean_without_mask": _Decl(_d_masked_mean_without_mask, raises=ValueError, match="masked mean needs a mask"),
    "sum_without_weights": _Decl(_d_sum_without_weights),
    "csr_bags": _Decl(_d_csr, derived_in_train=True),
    "tables_tuple": _Decl(_d_tables_tuple, declined=False),        # (no-grad: Python never asks; training: handed over as a list and served)
    "out_ld_small": _Decl(_d_out_ld_small, raises=ValueError, match="out_ld smaller than the plan's out_width", declined=False),
    "bf16_without_flag": _Decl(_d_bf16_without_flag, raises=TypeError, match="feature 'b': its table is torch.bfloat16 but the slot lacks"),
    "out_of_range_sync": _Decl(_d_out_of_range, raises=IndexError, match="1 lookup\\(s\\); first: feature 'b', sample 7, id 75",
                               declined=False, mode="sync"),
    "out_of_range_deferred": _Decl(_d_out_of_range, raises=IndexError, match="1 lookup\\(s\\); first: feature 'b', sample 7, id 75",
                                   declined=False, mode="deferred", flush=True),
}


def _outcome(d, kw, grad, seen):
    """Run one call; ('ok', tensors) or ('raised', type, message).  A deferred check is flushed inside."""
    from news_recsys_amd import ops
    plan = _watch(kw["plan"], seen)
    tables = kw["tables"]
    if grad:          # training form: leaves that train (through the sink, which takes every table type)
        tables = type(tables)(t.detach().clone().requires_grad_(True) for t in tables)
    try:
        with torch.set_grad_enabled(grad):
            res = ops.embed_apply(plan, tables, kw["inputs"], kw["weights"], out_ld=kw.get("out_ld"), index_check=d.mode,
                                  sparse_grad=ops.SparseGradSink() if grad else False)
            if d.flush:
                ops.flush_index_checks()
        torch.cuda.synchronize()
        return ("ok", [None if r is None else r.detach() for r in res])
    except Exception as e:           # noqa: BLE001 -- the outcome under test
        return ("raised", type(e), str(e))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "train"])
@pytest.mark.parametrize("name", list(DECLINED))
def test_declined_batch_ends_the_same_way(name, grad, path, monkeypatch):
    from news_recsys_amd import ops
    d = DECLINED[name]
    ops.flush_index_checks()
    ends = {}
    for leg in _legs(path):
        with monkeypatch.context() as mp:
            seen = _host_path(mp, leg)
            kw, canon = d.build()
            end = _outcome(d, kw, grad, seen)
            if leg == "binding" and d.declined and not (grad and d.derived_in_train):
                assert seen.bound and all(r is None for r in seen.bound), f"the binding was not asked or did not decline: {seen.bound}"
            if d.raises is not None:
                assert end[0] == "raised" and end[1] is d.raises, end
                assert re.search(d.match, end[2]), end[2]
            else:
                assert end[0] == "ok", end
                # the same batch with the conversion made by hand (a fresh plan, the same path)
                ckw = dict(kw, plan=ops.EmbedPlan(list(kw["plan"].slots), kw["plan"].out_width, kw["plan"].wide_width, kw["plan"].use_fm))
                ckw.update({k: v for k, v in canon.items() if k != "close"})
                want = _outcome(d, ckw, grad, _Seen())
                assert want[0] == "ok", want
                for got_t, want_t, nm in zip(end[1], want[1], ("out", "wide", "fm")):
                    if canon.get("close") and got_t is not None:          # another kernel form of the same sum: the pooled bar
                        torch.testing.assert_close(got_t, want_t, rtol=1e-6, atol=1e-6)
                    else:
                        _same_words(got_t, want_t, f"{leg} {name} vs the converted batch ({nm})")
            ends[leg] = end
        try:                                          # leave no deferred report behind for the next leg / test
            ops.flush_index_checks()
        except IndexError:
            pass
    if len(ends) == 2:
        a, b = ends["binding"], ends["ctypes"]
        assert a[0] == b[0]
        if a[0] == "raised":
            assert a[1] is b[1] and a[2] == b[2], f"the two paths raise differently:\n  binding: {a[1].__name__}: {a[2]}\n  ctypes:  {b[1].__name__}: {b[2]}"
        else:
            for x, y, nm in zip(a[1], b[1], ("out", "wide", "fm")):
                _same_words(x, y, f"binding vs ctypes, {name} ({nm})")


# ------------------------------------------------------------------------------------------------- C. tables that change (ops level)
ROWS3 = (50, 70, 90)
B3, D3, L3 = 139, 16, 4
MODES = ("nograd", "dense", "dense_sorted", "coo", "sink")


def _plan3():
    from news_recsys_amd import ops
    return ops.EmbedPlan([ops.Slot("a", NRX_SPARSE, 0, D3, 0, 0), ops.Slot("b", NRX_SPARSE, 1, D3, 0, D3), ops.Slot("c", NRX_SPARSE, 2, D3, 0, 2 * D3),
                          ops.Slot("h", NRX_BAG_MASKED_MEAN, 2, D3, L3, 3 * D3)], out_width=4 * D3)


def _table(gen, rows, mode, dtype=torch.float32):
    t = torch.randn(rows, D3, generator=gen).to(DEV).to(dtype)
    return t.requires_grad_(mode != "nograd" and (dtype is torch.float32 or mode == "sink"))


def _batch3(gen, rows, b_perm=False):
    """ids of the four features for tables of `rows` rows (b_perm: feature b looks every row of [1, rows[1]) up exactly once, B3 = 139)."""
    a = torch.randint(0, rows[0], (B3,), generator=gen)
    if b_perm:
        assert rows[1] - 1 == B3
        b = torch.randperm(rows[1] - 1, generator=gen) + 1
    else:
        b = torch.randint(0, rows[1], (B3,), generator=gen)
    c = torch.randint(0, rows[2], (B3,), generator=gen)
    m = (torch.arange(L3)[None, :] < torch.randint(0, L3 + 1, (B3, 1), generator=gen)).float()
    h = torch.randint(1, rows[2], (B3, L3), generator=gen) * m.long()
    g_out = torch.randn(B3, 4 * D3, generator=gen)
    return [a.to(DEV), b.to(DEV), c.to(DEV), h.to(DEV)], m.to(DEV), g_out.to(DEV)


def _ref3(tables, ids, m, g_out):
    """float64: the concat, every table's gradient (padding row zeroed) and, per gradient element, the sum of |contribution|."""
    a, b, c, h = ids
    T = [t.detach().double() for t in tables]
    md = m.double()
    den = md.sum(1, keepdim=True) + 1e-8
    out = torch.cat([T[0][a], T[1][b], T[2][c], (T[2][h] * md[:, :, None]).sum(1) / den], 1)
    g = g_out.double()
    grads, A = [], []
    for t, feats in enumerate((((a, 0),), ((b, 1),), ((c, 2),))):
        gt, At = torch.zeros_like(T[t]), torch.zeros_like(T[t])
        for idx, f in feats:
            gt.index_add_(0, idx, g[:, f * D3:(f + 1) * D3])
            At.index_add_(0, idx, g[:, f * D3:(f + 1) * D3].abs())
        if t == 2:
            w = (md / den)[:, :, None] * g[:, None, 3 * D3:]
            gt.index_add_(0, h.reshape(-1), w.reshape(-1, D3))
            At.index_add_(0, h.reshape(-1), w.abs().reshape(-1, D3))
        gt[0] = 0
        At[0] = 0
        grads.append(gt)
        A.append(At)
    return out, grads, A


def _step3(plan, tables, ids, m, g_out, mode, monkeypatch):
    """One forward (+ backward) of the three-table plan; (concat, per-table dense float32 gradients | None, the sink | None)."""
    from news_recsys_amd import ops
    ws = [None, None, None, m]
    if mode == "nograd":
        with torch.no_grad():
            out = ops.embed_apply(plan, tables, ids, ws)[0]
        torch.cuda.synchronize()
        return out, None, None
    for t in tables:
        t.grad = None
    sink = ops.SparseGradSink() if mode == "sink" else None
    with monkeypatch.context() as mp:
        if mode == "dense_sorted":
            mp.setattr(ops, "DENSE_BWD_SORTED", True)          # the planned reduction at any size: the dense mode that reads the cached row counts
        out = ops.embed_apply(plan, tables, ids, ws, sparse_grad=sink if sink is not None else (mode == "coo"))[0]
        out.backward(g_out)
    if sink is not None:
        assert all(t.grad is None for t in tables)
        grads = _sink_dense(sink.pending, [t.shape for t in tables])
    else:
        grads = [torch.zeros_like(t) if t.grad is None else (t.grad.to_dense() if t.grad.is_sparse else t.grad) for t in tables]
    torch.cuda.synchronize()
    return out.detach(), grads, sink


def _check3(tables, ids, m, g_out, out, grads, what):
    ref_out, ref_g, ref_A = _ref3(tables, ids, m, g_out)
    for f in range(3):
        assert torch.equal(out[:, f * D3:(f + 1) * D3], tables[f].detach()[ids[f]].float()), f"{what}: feature {'abc'[f]} is not its CURRENT table's rows"
    torch.testing.assert_close(out[:, 3 * D3:].double(), ref_out[:, 3 * D3:], rtol=1e-6, atol=1e-6)
    if grads is None:
        return
    for t in range(3):
        assert grads[t].shape == tables[t].shape, f"{what}: the gradient of table {t} has the shape of another table"
        err = (grads[t].double() - ref_g[t]).abs()
        over = err - 2e-6 * ref_A[t]
        assert float(over.max()) <= 0, f"{what}: gradient of table {t} beyond 2e-6 * sum|contribution| by {float(over.max()):.3g} " \
                                       f"(row {int(over.max(1).values.argmax())}: got {grads[t][int(over.max(1).values.argmax())][:4].tolist()})"


CHANGES = ("swap_first", "swap_middle", "swap_last", "grow_middle", "shrink_middle")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("change", CHANGES)
def test_table_set_changes_under_a_plan(change, mode, path, monkeypatch):
    """Two calls of ONE plan with ONE list object; between them one table of the list is replaced.  The second call reads the new table,
    its gradient belongs to the new table and covers every row of it, and no IndexError is raised for ids the new table has."""
    seen = _host_path(monkeypatch, path)
    gen = torch.Generator().manual_seed(CHANGES.index(change) * 10 + MODES.index(mode))
    rows = list(ROWS3)
    if change == "shrink_middle":
        rows[1] = 140
    plan = _watch(_plan3(), seen)
    tables = [_table(gen, r, mode) for r in rows]
    keep = list(tables)                                         # every tensor of this test stays alive until it ends
    ids, m, g_out = _batch3(gen, rows, b_perm=rows[1] == 140)
    out, grads, sink = _step3(plan, tables, ids, m, g_out, mode, monkeypatch)
    _check3(tables, ids, m, g_out, out, grads, f"{change} {mode} first call")
    for t in keep:
        t.grad = None
    # ---- the change
    k = {"swap_first": 0, "swap_last": 2}.get(change, 1)
    if change == "grow_middle":
        rows[1] = 140
    elif change == "shrink_middle":
        rows[1] = 70
    old = tables[k]
    new = _table(gen, rows[k], mode)
    keep.append(new)
    tables[k] = new
    ids, m, g_out = _batch3(gen, rows, b_perm=rows[1] == 140)
    if change == "grow_middle":
        assert int(ids[1].max()) == 139 and int((ids[1] >= 70).sum()) == 70
    out, grads, sink = _step3(plan, tables, ids, m, g_out, mode, monkeypatch)        # (index check 'sync': a stale row count would raise here)
    _check3(tables, ids, m, g_out, out, grads, f"{change} {mode} second call")
    _ran_on(path, seen, plan)
    if grads is None:
        return
    if sink is not None:
        assert all(e["tables"][k] is new for e in sink.pending), "the sink's entries name the replaced table"
    else:
        assert new.grad is not None and new.grad.shape == new.shape, "no gradient on the new table"
        assert old.grad is None                                  # (cleared before the second call: nothing was added to the old one)
    looked = torch.zeros(rows[k], dtype=torch.bool, device=DEV)
    for f, t in ((0, 0), (1, 1), (2, 2), (3, 2)):
        if t == k:
            looked[ids[f].reshape(-1)] = True
    looked[0] = False
    assert bool((grads[k][looked].abs().sum(1) > 0).all()), "a looked-up row of the new table has no gradient"
    if rows[1] == 140:
        # feature b looked every row of [1, 140) up exactly once: its gradient row IS the upstream row
        want = torch.zeros(140, D3, device=DEV)
        want[ids[1]] = g_out[:, D3:2 * D3]
        assert torch.equal(_words(grads[1]), _words(want)), f"rows without their gradient: {torch.nonzero((grads[1] != want).any(1))[:, 0].tolist()[:12]}"
    if change == "shrink_middle" or change.startswith("swap"):
        # as a fresh plan and a fresh list give it (the deterministic modes word for word)
        out2, grads2, _ = _step3(_plan3(), list(tables), ids, m, g_out, mode, monkeypatch)
        _same_words(out, out2, "changed plan vs fresh plan (concat)")
        for t in range(3):
            if mode == "dense":
                torch.testing.assert_close(grads[t], grads2[t], rtol=1e-5, atol=1e-6)
            else:
                _same_words(grads[t], grads2[t], f"changed plan vs fresh plan (gradient of table {t})")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", MODES)
def test_middle_table_converted_to_bf16_under_an_fp32_slot(mode, path, monkeypatch):
    from news_recsys_amd import ops
    seen = _host_path(monkeypatch, path)
    gen = torch.Generator().manual_seed(7)
    plan = _watch(_plan3(), seen)
    tables = [_table(gen, r, mode) for r in ROWS3]
    keep = list(tables)
    ids, m, g_out = _batch3(gen, ROWS3)
    out, grads, _ = _step3(plan, tables, ids, m, g_out, mode, monkeypatch)
    _check3(tables, ids, m, g_out, out, grads, f"bf16 {mode} first call")
    tables[1] = _table(gen, ROWS3[1], mode, dtype=torch.bfloat16)
    keep.append(tables[1])
    with pytest.raises(TypeError, match="feature 'b': its table is torch.bfloat16 but the slot lacks NRX_FEAT_TABLE_BF16"):
        _step3(plan, tables, ids, m, g_out, mode, monkeypatch)
    if path == "binding":
        assert seen.bound[-1] is None                           # the binding's convention: decline, Python raises
    assert len(keep) == 4
    ops.flush_index_checks()


@pytest.mark.parametrize("path", PATHS)
def test_all_ids_plan_sees_a_converted_middle_table(path, monkeypatch):
    """The same for a plan of single-valued features only, whose no-grad ctypes form validates the tables only when it binds them."""
    from news_recsys_amd import ops
    seen = _host_path(monkeypatch, path)
    gen = torch.Generator().manual_seed(8)
    plan = _watch(ops.EmbedPlan(_plan3().slots[:3], out_width=3 * D3), seen)
    tables = [_table(gen, r, "nograd") for r in ROWS3]
    keep = list(tables)
    ids = _batch3(gen, ROWS3)[0][:3]
    with torch.no_grad():
        out = ops.embed_apply(plan, tables, ids, [None] * 3)[0]
        for f in range(3):
            assert torch.equal(out[:, f * D3:(f + 1) * D3], tables[f][ids[f]])
        _ran_on(path, seen, plan)
        tables[1] = tables[1].to(torch.bfloat16)
        keep.append(tables[1])
        with pytest.raises(TypeError, match="feature 'b': its table is torch.bfloat16 but the slot lacks NRX_FEAT_TABLE_BF16"):
            ops.embed_apply(plan, tables, ids, [None] * 3)
    assert len(keep) == 4


# ------------------------------------------------------------------------------------------------- D. the same through the model
MODEL_CASES = [("cf_deep_small.yaml", "subcategory"), ("cf_array_small.yaml", "item_id"), ("cf_array_small.yaml", "user_click_cats")]


def _model_batch(m, names, B, gen):
    batch = {}
    for n in sorted(names):
        rows = m.embedding_tables[m._get_emb_feature_name(n)].num_embeddings
        if n in m.array_feature_names:
            L = m.array_max_length[n]
            mask = (torch.arange(L)[None, :] < torch.randint(1, L + 1, (B, 1), generator=gen)).float()
            batch[n] = (torch.randint(1, rows, (B, L), generator=gen) * mask.long()).to(DEV)
            batch[f"{n}_mask"] = mask.to(DEV)
        else:
            batch[n] = torch.randint(1, rows, (B,), generator=gen).to(DEV)
    return batch


def _model_ref(m, batch, names, G):
    """float64 restatement of get_embeddings_from_batch over sorted(names) and of d (features * G).sum() / d table."""
    cols, col = {}, 0
    tabs = {tn: emb.weight.detach().double().requires_grad_(True) for tn, emb in m.embedding_tables.items()}
    parts = []
    for n in sorted(names):
        t = tabs[m._get_emb_feature_name(n)]
        if n in m.array_feature_names:
            md = batch[f"{n}_mask"].double()
            e = (t[batch[n]] * md[:, :, None]).sum(1) / (md.sum(1, keepdim=True) + 1e-8)
        else:
            e = t[batch[n]]
        cols[n] = (col, col + e.shape[1])
        col += e.shape[1]
        parts.append(e)
    out = torch.cat(parts, 1)
    (out * G.double()).sum().backward()
    grads = {}
    for tn, t in tabs.items():
        g = torch.zeros_like(t) if t.grad is None else t.grad.clone()
        g[0] = 0                                              # padding_idx = 0
        grads[tn] = g
    return out.detach(), cols, grads


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("how", ["data", "parameter"])
@pytest.mark.parametrize("cfg,tname", MODEL_CASES)
def test_model_follows_a_changed_table(cfg, tname, how, path, monkeypatch):
    """After a step, a table that is neither first nor last in the plan's table list gets new values -- its Parameter's .data swapped, or
    the Parameter replaced.  The next call reads the new rows, and the default (dense) backward leaves the gradient on the new Parameter."""
    from news_recsys_amd.model.sort.deep.model import Deep
    seen = _host_path(monkeypatch, path)
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(3)
    m = Deep(os.path.join(CONFIGS, cfg)).to(DEV)
    names = m.user_feature_names | m.item_feature_names
    B = 32
    batch = _model_batch(m, names, B, gen)
    keep = []

    def step(tag):
        """no-grad and training call; both against float64.  Returns the parameter gradients."""
        with torch.no_grad():
            inf = m.get_embeddings_from_batch(batch, names)[0]
        for p in m.parameters():
            p.grad = None
        feats = m.get_embeddings_from_batch(batch, names)[0]
        G = torch.randn(feats.shape, generator=gen).to(DEV)
        loss = (feats * G).sum()
        loss.backward()
        torch.cuda.synchronize()
        ref, cols, ref_g = _model_ref(m, batch, names, G)
        _same_words(inf, feats, f"{tag}: no-grad vs training call")
        for n in sorted(names):
            lo, hi = cols[n]
            if n in m.array_feature_names:
                torch.testing.assert_close(feats[:, lo:hi].detach().double(), ref[:, lo:hi], rtol=1e-6, atol=1e-6, msg=lambda s: f"{tag} {n}: {s}")
            else:
                w = m.embedding_tables[m._get_emb_feature_name(n)].weight.detach()
                assert torch.equal(feats[:, lo:hi].detach(), w[batch[n]]), f"{tag}: feature {n} is not its CURRENT table's rows"
        for tn, emb in m.embedding_tables.items():
            if not any(m._get_emb_feature_name(n) == tn for n in names):
                continue
            assert emb.weight.grad is not None, f"{tag}: no gradient on the current Parameter of {tn}"
            torch.testing.assert_close(emb.weight.grad.double(), ref_g[tn], rtol=1e-4, atol=1e-5, msg=lambda s: f"{tag} {tn}: {s}")
        return ref, cols

    step("first step")
    plan = next(iter(m._embed_cache.values()))[0]
    table_names = []
    for s in plan.slots:
        tn = m._get_emb_feature_name(s.name)
        if tn not in table_names:
            table_names.append(tn)
    assert 0 < table_names.index(tname) < len(table_names) - 1, table_names
    emb = m.embedding_tables[tname]
    old = emb.weight
    keep.append(old)
    keep.append(old.data)
    old.grad = None                                            # (the first step's; what the second step adds to it would show)
    new_values = torch.randn(old.shape, generator=gen).to(DEV)
    new_values[0] = 0
    if how == "data":
        emb.weight.data = new_values
    else:
        emb.weight = torch.nn.Parameter(new_values)
    _watch(plan, seen)
    ref, cols = step(f"after the {how} change")
    cur = m.embedding_tables[tname].weight
    assert torch.equal(cur.detach(), new_values)
    if how == "parameter":
        assert cur is not old and old.grad is None, "the gradient went to the replaced Parameter"
    looked = torch.zeros(cur.shape[0], dtype=torch.bool, device=DEV)
    for n in sorted(names):
        if m._get_emb_feature_name(n) == tname:
            looked[batch[n].reshape(-1)] = True
    looked[0] = False
    assert bool(looked.any()) and bool((cur.grad[looked].abs().sum(1) > 0).all()), "a looked-up row of the new table has no gradient"
    if path == "ctypes":
        assert not seen.bound and seen.ctypes_work() > 0
    else:
        assert seen.ctypes_work() == 0, "the binding leg fell back to ctypes"
