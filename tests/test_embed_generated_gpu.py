"""Generated embedding launches (tests/embed_cases.py) end to end on the GPU against their float64 restatement.

Per seed: the forward in its three forms (inference, training, PreparedEmbed) under both forward kernel families; the table gradients in
every backward mode (dense auto / planned / deterministic / atomic, COO, the sink, PreparedSparseBackward) with the seed's planner, padding
split, placement and size-threshold knobs; the sink's (keys, values) and one FusedSparseAdam step against a float64 Adam, bf16 tables
included.  Copies are bit-exact; every other element lies within the bound C * n * 2^-24 * A of embed_cases; the deterministic modes agree
word for word with each other and with a second run.  A last test checks that the seed list still reaches every dispatch path."""
import math

import numpy as np
import pytest
import torch

from news_recsys_amd._lib import NRX_DENSE, NRX_FEAT_BAG_CSR
from tests import embed_cases as E
from tests import sr_bf16_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASK = (1 << 40) - 1
SENTINEL = -12345.678


def _lib():
    from news_recsys_amd import _lib
    return _lib.load()


@pytest.fixture(params=["small_kernel", "big_kernels"])
def kernel_family(request):
    """Both forward families (nrx_set_small_batch_max: every batch through the one-block-per-sample kernel, or none)."""
    lib = _lib()
    prev = lib.nrx_set_small_batch_max((1 << 20) if request.param == "small_kernel" else 0)
    yield request.param
    lib.nrx_set_small_batch_max(prev)


def _set_knobs(monkeypatch, case):
    from news_recsys_amd import ops
    for k, v in case.knobs.items():
        monkeypatch.setattr(ops, k, v)


def _dev(case):
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in case.inputs]
    ws = [None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(DEV) for w in case.weights]
    return ins, ws


def _tables(case, requires_grad=False):
    ts = []
    for t in case.tables:
        x = torch.from_numpy(t).to(DEV)
        if case.bf16:
            x = x.to(torch.bfloat16)                  # exact: the generator drew bf16 values
        ts.append(x.requires_grad_(requires_grad))
    return ts


def _up(case, narrow):
    g_out = torch.from_numpy(case.g_out).to(DEV)
    if narrow:
        g_out = g_out[:, :case.out_width].contiguous()
    g_wide = None if case.g_wide is None else torch.from_numpy(case.g_wide).to(DEV)
    g_fm = None if case.g_fm is None else torch.from_numpy(case.g_fm).to(DEV)
    return g_out, g_wide, g_fm


def _within(got, ref, A, n, what, case):
    ex, i = E.excess(got, ref, A, n)
    assert ex <= 0, f"{what}: element {i} (of shape {tuple(ref.shape)}) beyond the bound by {ex:.3g}: got " \
                    f"{float(got.reshape(-1)[i])} want {float(ref.reshape(-1)[i])}\n{case.spec()}"


def _words(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("seed", E.SEEDS)
def test_forward_three_forms_against_float64(seed, kernel_family, monkeypatch):
    from news_recsys_amd import ops
    case = E.make_case(seed)
    _set_knobs(monkeypatch, case)
    ins, ws = _dev(case)
    B, W, ld = case.B, case.out_width, case.out_ld
    ref = E.restate(case, DEV, grads=False)
    # inference form (no grad: _FastForward for <= 64 features)
    tabs = _tables(case)
    with torch.no_grad():
        inf = ops.embed_apply(case.plan(), tabs, ins, ws, out_ld=ld, narrow=case.narrow)
    # training form (_EmbedFn; bf16 tables train only through the sink)
    tabs_g = _tables(case, requires_grad=True)
    trn = ops.embed_apply(case.plan(), tabs_g, ins, ws, out_ld=ld, narrow=case.narrow,
                          sparse_grad=ops.SparseGradSink() if case.bf16 else False)
    # PreparedEmbed into a sentinel-filled buffer with rows past B and a padded stride
    big = torch.full((B + 3, ld), SENTINEL, dtype=torch.float32, device=DEV)
    bigfm = torch.full((B + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    prep = ops.PreparedEmbed(case.plan(), tabs, ins, ws, out_ld=ld, out=big[:B], fm=bigfm[:B] if case.use_fm else None)
    if case.n_feats > 64:
        assert len(prep.calls) > 1                      # the launch is split at 64 features
    pre = prep.run()
    torch.cuda.synchronize()
    want_cols = W if case.narrow else ld
    for name, res in (("inference", inf), ("training", trn)):
        assert res[0].shape == (B, want_cols), (name, tuple(res[0].shape))
    forms = {"inference": inf, "training": trn, "prepared": pre}
    o0, w0, f0 = (x.detach() if x is not None else None for x in inf)
    for name, (o, w, f) in forms.items():
        o = o.detach()
        assert torch.equal(_words(o[:, :W]), _words(o0[:, :W])), f"{name} != inference (concat)\n{case.spec()}"
        if case.wide_width:
            assert torch.equal(_words(w.detach()), _words(w0)), f"{name} != inference (wide)"
        if case.use_fm:
            assert torch.equal(_words(f.detach()), _words(f0)), f"{name} != inference (fm)"
    # the stride padding and the rows past B are never written
    assert bool((big[:B, W:] == SENTINEL).all()) and bool((big[B:] == SENTINEL).all()), "a write outside the concat's columns / rows"
    assert bool((bigfm[B:] == SENTINEL).all()) and (case.use_fm or bool((bigfm == SENTINEL).all()))
    # against float64
    out = o0[:, :W]
    cc = ref.copy_cols
    if cc:
        assert torch.equal(out[:, cc], ref.out[:, cc].float()), f"copied columns differ\n{case.spec()}"
    _within(out, ref.out, ref.A_out, ref.n_out, "concat", case)
    if case.wide_width:
        wc = ref.wide_copy_cols
        if wc:
            assert torch.equal(w0[:, wc], ref.wide[:, wc].float()), "wide columns of single ids are copies"
        _within(w0, ref.wide, ref.A_wide, ref.n_out, "wide", case)
    if case.use_fm:
        _within(f0, ref.fm, ref.A_fm, ref.n_fm, "fm", case)


# ------------------------------------------------------------------------------------------------- backward
def _sink_dense(pending, shapes, check_unique=True):
    """A sink's entries scattered into dense float32 gradients (keys: launch-local table << 40 | row)."""
    grads = [torch.zeros(s, dtype=torch.float32, device=DEV) for s in shapes]
    for e in pending:
        keys = e["uniq"]
        if e.get("filler"):
            valid = keys >= 0
        else:
            valid = torch.arange(keys.numel(), device=DEV) < e["counts"][0]
        k = keys[valid]
        v = e["values"][:keys.numel()][valid]
        if check_unique:
            assert torch.unique(k).numel() == k.numel(), "a key appears twice in one sink entry"
        t, r = k >> 40, k & MASK
        for ti in torch.unique(t).tolist():
            sel = t == ti
            grads[ti].index_put_((r[sel],), v[sel], accumulate=True)
    return grads


def _backward(case, plan, mode, monkeypatch):
    """One forward + backward of the case in `mode`; returns (per-table float32 gradients, info)."""
    from news_recsys_amd import ops
    ins, ws = _dev(case)
    tabs = _tables(case, requires_grad=True)
    shapes = [t.shape for t in tabs]
    info = {}
    before = dict(ops.dense_bwd_paths)
    if mode == "prepared":
        g_out, g_wide, g_fm = _up(case, False)
        sums = None
        if case.use_fm:
            sums = torch.empty((case.B, max(s.dim for s in case.slots if s.fm_field)), dtype=torch.float32, device=DEV)
        fwd = ops.PreparedEmbed(plan, tabs, ins, ws, out_ld=case.out_ld, fm_sums=sums)
        fwd.run()
        bwd = ops.PreparedSparseBackward(fwd, g_out, g_fm=g_fm, g_wide=g_wide)
        groups = bwd.run()
        pend = [dict(uniq=g["uniq"], values=g["values"], counts=g["counts"]) for g in groups]
        grads = _sink_dense(pend, shapes)
        torch.cuda.synchronize()
        return grads, info
    sink = None
    if mode == "sink":
        sink = ops.SparseGradSink()
        sg = sink
    else:
        sg = mode == "coo"
        monkeypatch.setattr(ops, "DENSE_BWD_SORTED", {"auto": None, "sorted": True, "det": "det", "atomic": False, "coo": None}[mode])
    out, wide, fm = ops.embed_apply(plan, tabs, ins, ws, out_ld=case.out_ld, narrow=case.narrow, sparse_grad=sg)
    g_out, g_wide, g_fm = _up(case, case.narrow)
    if case.use_fm and case.n_feats > 64:
        info["fm_concat"] = out.grad_fn.fm_sums is None
    outs, ups = [out], [g_out]
    if wide is not None:
        outs.append(wide)
        ups.append(g_wide)
    if fm is not None:
        outs.append(fm)
        ups.append(g_fm)
    torch.autograd.backward(outs, ups)
    if sink is not None:
        assert all(t.grad is None for t in tabs)
        info["filler"] = any(e.get("filler") for e in sink.pending)
        info["pending"] = list(sink.pending)
        grads = _sink_dense(sink.pending, shapes)
    else:
        grads = [torch.zeros(s, dtype=torch.float32, device=DEV) if t.grad is None else
                 (t.grad.to_dense() if t.grad.is_sparse else t.grad) for s, t in zip(shapes, tabs)]
    torch.cuda.synchronize()
    info["paths"] = {k: ops.dense_bwd_paths[k] - before.get(k, 0) for k in ("small", "sorted", "atomic")}
    return grads, info


def _prepared_applies(case):
    if case.n_feats > 64 or case.bf16 or any(s.flags & NRX_FEAT_BAG_CSR for s in case.slots):
        return False
    by_dim = {}
    for s, x in zip(case.slots, case.inputs):
        if s.kind != NRX_DENSE:
            by_dim.setdefault(s.dim, set()).add(x.dtype)
    return all(len(v) == 1 for v in by_dim.values())


@pytest.mark.parametrize("seed", [s for s in E.SEEDS if not E.make_case(s).bf16])
def test_backward_every_mode_against_float64(seed, monkeypatch):
    case = E.make_case(seed)
    _set_knobs(monkeypatch, case)
    ref = E.restate(case, DEV)
    modes = ["auto", "sorted", "det", "atomic", "coo", "sink"] + (["prepared"] if _prepared_applies(case) else [])
    deterministic = {"sorted", "det", "coo", "sink", "prepared"}
    res = {}
    for mode in modes:
        plan = case.plan()
        runs = [_backward(case, plan, mode, monkeypatch)]
        if mode in deterministic:
            runs.append(_backward(case, plan, mode, monkeypatch))      # the same plan object again: planner statistics now recorded
        grads, info = runs[0]
        for t, g in enumerate(grads):
            _within(g, ref.grads[t], ref.A_grads[t], ref.n_grads[t], f"{mode}: gradient of table {t}", case)
            assert float(g[0].abs().max()) == 0.0, f"{mode}: the padding row of table {t} has a gradient"
            assert bool((g[ref.A_grads[t] == 0] == 0).all()), f"{mode}: a row that was not looked up has a gradient (table {t})"
        if len(runs) == 2:
            for t, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
                assert torch.equal(_words(a), _words(b)), f"{mode}: two runs differ (table {t})\n{case.spec()}"
        if mode == "det":
            info["took_small"] = info["paths"]["small"] > 0
        if mode == "sink" and info.get("fm_concat") is not None:
            assert info["fm_concat"]
        res[mode] = (grads, info)
    # the planned reductions agree word for word (the one-launch small kernels sum in their own order: compared among themselves)
    planned = [m for m in ("sorted", "coo", "prepared") if m in res]
    if "sink" in res and not res["sink"][1]["filler"]:
        planned.append("sink")
    if not res["det"][1]["took_small"]:
        planned.append("det")
    for m in planned[1:]:
        for t, (a, b) in enumerate(zip(res[planned[0]][0], res[m][0])):
            assert torch.equal(_words(a), _words(b)), f"{planned[0]} != {m} (table {t})\n{case.spec()}"
    auto_paths = res["auto"][1]["paths"]
    assert sum(auto_paths.values()) >= 1
    for p in ("small", "sorted", "atomic"):
        if f"dense_{p}" in case.paths:
            assert auto_paths[p] >= 1, f"auto mode did not take the {p} path: {auto_paths}\n{case.spec()}"


# ------------------------------------------------------------------------------------------------- sink + FusedSparseAdam
LR, BETAS, ADAM_EPS = 0.01, (0.9, 0.999), 1e-8


def _ulp32(x):
    return torch.clamp(x.abs(), min=2.0 ** -126) * 2.0 ** -23


@pytest.mark.parametrize("seed", E.SEEDS)
def test_sink_and_fused_sparse_adam_step(seed, monkeypatch):
    """The sink's (keys, values) against the float64 gradient, then one FusedSparseAdam step against a float64 Adam applied to those same
    values: moments and weights to a few ulp (fp32 tables) or one of the two bf16 neighbours chosen by the stochastic rounding's bits (bf16
    tables); rows that were not looked up keep their bits."""
    from news_recsys_amd import ops
    from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
    case = E.make_case(seed)
    _set_knobs(monkeypatch, case)
    ref = E.restate(case, DEV)
    ins, ws = _dev(case)
    tabs = _tables(case, requires_grad=True)
    before = [t.detach().clone() for t in tabs]
    sink = ops.SparseGradSink()
    opt = FusedSparseAdam(sink, lr=LR, betas=BETAS, eps=ADAM_EPS, params=tabs if case.bf16 else None, sr_seed=seed * 7919 + 1)
    out, wide, fm = ops.embed_apply(case.plan(), tabs, ins, ws, out_ld=case.out_ld, narrow=case.narrow, sparse_grad=sink)
    g_out, g_wide, g_fm = _up(case, case.narrow)
    outs, ups = [out], [g_out]
    for o, g in ((wide, g_wide), (fm, g_fm)):
        if o is not None:
            outs.append(o)
            ups.append(g)
    torch.autograd.backward(outs, ups)
    assert sink.pending
    shapes = [t.shape for t in tabs]
    g_sink = _sink_dense(sink.pending, shapes)
    # what Adam is checked against: the float64 sum of the entries' pieces (two entries of one width meet in one fp32 addition: nrx_rows_merge)
    g64 = [torch.zeros(s, dtype=torch.float64, device=DEV) for s in shapes]
    for e in sink.pending:
        part = _sink_dense([e], shapes)
        for t in range(len(shapes)):
            g64[t] += part[t].double()
    for t, g in enumerate(g_sink):
        _within(g, ref.grads[t], ref.A_grads[t], ref.n_grads[t], f"sink gradient of table {t}", case)
    dims = {}
    for e in sink.pending:
        dims[e["dim"]] = dims.get(e["dim"], 0) + 1
    two_groups = any(v >= 2 for v in dims.values())
    looked = [torch.zeros(s[0], dtype=torch.bool, device=DEV) for s in shapes]
    for e in sink.pending:
        keys = e["uniq"]
        valid = (keys >= 0) if e.get("filler") else (torch.arange(keys.numel(), device=DEV) < e["counts"][0])
        k = keys[valid]
        for ti in torch.unique(k >> 40).tolist():
            looked[ti][(k & MASK)[(k >> 40) == ti]] = True
    for lk in looked:
        lk[0] = False                                    # the padding row never moves
    opt.step()
    torch.cuda.synchronize()
    assert not sink.pending
    if two_groups:
        assert len(opt._maps) > 0, "two backward groups of one width did not take the pair merge"
    # the float64 Adam takes the hyperparameters as the C-ABI carries them: float32 betas (the kernel's 1 - beta2 is 1 - float(0.999),
    # 1.3e-5 relative off torch's 1 - 0.999) and the float32 step size optim.FusedSparseAdam passes
    b1, b2 = (float(np.float32(b)) for b in BETAS)
    step_size = float(np.float32(LR * math.sqrt(1.0 - BETAS[1]) / (1.0 - BETAS[0])))
    for t, tab in enumerate(tabs):
        new = tab.detach()
        lk = looked[t]
        assert torch.equal(new[~lk].float().view(torch.int32), before[t][~lk].float().view(torch.int32)), f"table {t}: an untouched row moved"
        if not bool(lk.any()):
            continue
        i = opt._index[id(tab)]
        m_got, v_got = opt.moments[i]
        g = g64[t][lk]
        m64 = (1 - b1) * g
        v64 = (1 - b2) * g * g
        upd = m64 / (v64.sqrt() + ADAM_EPS)
        w_old = before[t][lk].double()
        w64 = w_old - step_size * upd
        gerr = 4 * _ulp32(g)                             # the fp32 merge of two groups' pieces rounds once
        assert bool(((m_got[lk].double() - m64).abs() <= 4 * _ulp32(m64) + (1 - b1) * gerr).all()), f"table {t}: exp_avg"
        assert bool(((v_got[lk].double() - v64).abs() <= 8 * _ulp32(v64) + (1 - b2) * 2 * g.abs() * gerr).all()), f"table {t}: exp_avg_sq"
        if not case.bf16:
            tol = 4 * _ulp32(w64) + 8 * _ulp32(step_size * upd) + step_size * 1e-6 * (gerr / (g.abs() + ADAM_EPS)).clamp(max=1)
            err = (new[lk].double() - w64).abs()
            assert bool((err <= tol).all()), f"table {t}: weights beyond a few ulp of float64 Adam: max {float(err.max())}\n{case.spec()}"
        else:
            # one of the two bf16 neighbours of the float64 result, and the one the rounding's bits choose
            got16 = new[lk].view(torch.int16).cpu().numpy().view(np.uint16)
            w32 = w64.float().cpu().numpy()
            rows = torch.nonzero(lk)[:, 0].cpu().numpy()
            bits = SR.sr_bits(opt.sr_seed, 1, opt._index[id(tab)], rows, np.arange(tab.shape[1]))
            want = SR.sr_round(w32, bits)
            f_got = SR.bf16_to_f32(got16).astype(np.float64)
            w_np = w64.cpu().numpy()
            down = (np.asarray(w32, np.float32).view(np.uint32) >> 16 << 16).view(np.float32).astype(np.float64)
            up = (((np.asarray(w32, np.float32).view(np.uint32) >> 16) + 1) << 16).astype(np.uint32).view(np.float32).astype(np.float64)
            lo_n, hi_n = np.minimum(down, up), np.maximum(down, up)
            slack = 4 * np.abs(w_np) * 2.0 ** -23
            assert np.all((f_got >= lo_n - slack) & (f_got <= hi_n + slack)), f"table {t}: a bf16 weight is not a neighbour of float64 Adam"
            # the choice: equal to the restated rounding except where the kernel's fp32 result may sit on the other side of the rounding
            # threshold -- within its own error (a few ulp of the old weight and of the update; many ulp of a result that cancels) of it
            u = np.asarray(w32, np.float32).view(np.uint32).astype(np.int64)
            frac = (u + bits.astype(np.int64)) & 0xFFFF
            err = (4 * _ulp32(w_old) + 8 * _ulp32(step_size * upd)).cpu().numpy()
            k = np.ceil(err / _ulp32(w64).cpu().numpy()) + 2
            ambiguous = (frac < k) | (frac > 0xFFFF - k)
            mism = (got16 != want) & ~ambiguous
            assert not mism.any(), f"table {t}: {int(mism.sum())} bf16 weights rounded the other way than the bits choose"


# ------------------------------------------------------------------------------------------------- path coverage
def _first_seed(path):
    for s in E.SEEDS:
        if path in E.make_case(s).paths:
            return s
    raise AssertionError(f"no seed of the list takes the {path} path")


def test_seed_list_reaches_every_path(monkeypatch):
    """Independent of test order and -k: for every path one seed the generator marks as taking it is run and the path is seen taken."""
    from news_recsys_amd import ops
    from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
    lib = _lib()
    # both forward families: the knob the fixture turns is live
    prev = lib.nrx_set_small_batch_max(1 << 20)
    assert lib.nrx_set_small_batch_max(0) == (1 << 20) and lib.nrx_set_small_batch_max(prev) == 0
    for p in ("small", "sorted", "atomic"):
        case = E.make_case(_first_seed(f"dense_{p}"))
        with monkeypatch.context() as mp:
            _set_knobs(mp, case)
            _, info = _backward(case, case.plan(), "auto", mp)
        assert info["paths"][p] >= 1, (p, info["paths"], case.spec())
    case = E.make_case(_first_seed("fwd_split"))
    ins, ws = _dev(case)
    assert len(ops.PreparedEmbed(case.plan(), _tables(case), ins, ws, out_ld=case.out_ld).calls) > 1
    case = E.make_case(_first_seed("fm_bwd_concat"))
    with monkeypatch.context() as mp:
        _set_knobs(mp, case)
        _, info = _backward(case, case.plan(), "sink", mp)
    assert info["fm_concat"] is True
    case = E.make_case(_first_seed("csr_sink"))
    with monkeypatch.context() as mp:
        _set_knobs(mp, case)
        _, info = _backward(case, case.plan(), "sink", mp)
    assert info["pending"] and any(s.flags & NRX_FEAT_BAG_CSR for s in case.slots)
    case = E.make_case(_first_seed("adam_two_groups"))
    with monkeypatch.context() as mp:
        _set_knobs(mp, case)
        _, info = _backward(case, case.plan(), "sink", mp)
    sink = ops.SparseGradSink()
    sink.pending.extend(info["pending"])
    dims = [e["dim"] for e in sink.pending]
    assert any(dims.count(d) >= 2 for d in dims)
    opt = FusedSparseAdam(sink, lr=LR)
    opt.step()
    assert len(opt._maps) > 0
