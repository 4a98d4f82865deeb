"""Generated bound sharded steps (tests/shard_cases.py) at world 1 on the GPU against their float64 truth and the direct path.

Per seed and form: the step's own attributes take the predicted paths (placed groups, direct-gradient groups, the nrx_embed_bwd fallback,
the FM pass, the fork, the planning mode, the pooled routing, the replicated backward), its capacities are the generator's; the concat, wide
columns, FM logit and the table gradients lie within the bound of embed_cases against float64 (copies bit for bit); the non-pooled columns,
the wide columns, the fused FM logit and every (key, value) of a table no pooled bag feeds equal the direct bound path (PreparedEmbed +
PreparedSparseBackward on full tables) word for word; two runs give the same bits; the dummy row and the global padding row stay zero and
the padding row is never keyed; nothing is written outside the concat; one FusedSparseAdam step matches float64 Adam on the step's own
gradient.  Forward-only cases (> 64 features) check the refusal of bind_backward.  World 2 / 3: test_shard_generated_multirank_one_gpu.py."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

from tests import embed_cases as E
from tests import shard_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASK = (1 << 40) - 1
SENTINEL = -12345.678
LR, BETAS, ADAM_EPS = 0.01, (0.9, 0.999), 1e-8
W1_SEEDS = [sd for sd in S.SEEDS if S.case(sd).world == 1]


@contextlib.contextmanager
def applied(case, form):
    """The form's environment (NRX_ROUTE_BAGS, NRX_SHARD_OVERLAP, NRX_SHARD_PLAN: read when the step binds and first runs) and the
    case's ops.* knobs, restored afterwards."""
    from news_recsys_amd import ops
    env = {"NRX_ROUTE_BAGS": form["route_bags"], "NRX_SHARD_OVERLAP": form["overlap"], "NRX_SHARD_PLAN": form["plan"]}
    old_env = {k: os.environ.get(k) for k in env}
    old_knobs = {k: getattr(ops, k) for k in case.knobs}
    os.environ.update(env)
    for k, v in case.knobs.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for k, v in old_knobs.items():
            setattr(ops, k, v)


def _ulp32(x):
    return torch.clamp(x.abs(), min=2.0 ** -126) * 2.0 ** -23


def _entries_np(entries, names_of):
    got = []
    for e in entries:
        nu = int(e["counts"][0])
        got.append(([names_of[id(t)] for t in e["tables"]], e["dim"], e["uniq"][:nu].cpu().numpy(), e["values"][:nu].cpu().numpy().copy()))
    return got


def _observed_paths(step, case, form):
    p = set()
    placed = [g for g in step.groups if g.get("placed")]
    if placed:
        p.add("placed")
    if step.fm_pass is not None:
        p.add("fm_pass")
    if not step.single:
        p.add("fwd_split")
    rep = {f.table for f in case.feats if f.replicated}
    if any(a.shape[0] == 1 for t, a in step.keep[2].items() if t not in rep):
        p.add("empty_shard")                        # (this rank's shard of a routed table is the dummy row alone)
    for g in step.groups:
        if g["pooled"]:
            p.add("route_bags:runs" if g.get("runs_state") is not None else "route_bags:one" if g.get("rstate") is not None else "route_bags:legacy")
    if step.bwd is not None:
        p.add(f"plan:{step.plan_mode}")
        if step._overlap:
            p.add("forked")
        for b in step.bwd:
            if b["pooled"]:
                p.add("pooled_binary" if b["binary"] else "pooled_expand")
            elif b["direct"]:
                p.add("direct_grad")
            else:
                p.add("bwd_scatter" if b["scatter_ok"] else "bwd_fallback")
        if step.rep is not None:
            p.add("replicated_fold" if "lay" in step.rep else "replicated_w1")
    return sorted(p)


def rank_run(case, form, rank, eng, barrier=None):
    """Bind the case's step on this rank in `form`, run it (twice, or once with the overflow report), check what one rank can check, and
    return the rank's results as numpy (out, wide, fm, entries) for the float64 and direct-path comparisons."""
    from news_recsys_amd import ops, shard_step
    from news_recsys_amd.model.model_utils.optim import FusedSparseAdam
    W, B = case.world, case.B
    groups, pooled, plan = case.plan()
    ld = case.ld
    rep_tables = {f.table for f in case.feats if f.replicated}
    arenas = {}
    for t, x in sorted(case.tables.items()):
        full = torch.from_numpy(x).to(DEV)
        arenas[t] = full.clone() if t in rep_tables else shard_step.make_arena(x.shape[0], x.shape[1], rank, W, DEV, full=full)
    names_of = {id(a): t for t, a in arenas.items()}
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in case.inputs[rank]]
    ws = [None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(DEV) for w in case.weights[rank]]
    big = torch.full((B + 3, ld), SENTINEL, dtype=torch.float32, device=DEV)
    bigfm = torch.full((B + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    step = shard_step.PreparedShardedStep(eng, case.sharded_features(), ins, ws, arenas, out_ld=case.out_ld, out=big[:B],
                                          fm=bigfm[:B] if plan.use_fm else None, train=not case.forward_only, slack=case.slack,
                                          one_sided=form["one_sided"], binary_masks=form["binary_masks"], check_index=form["check_index"],
                                          replicated_grads=bool(rep_tables))
    assert step.plan_mode == form["plan"]
    assert [s.out_col for s in step.plan.slots] == [s.out_col for s in plan.slots]
    assert [g["cap"] if g["pooled"] else g["capf"] for g in step.groups] == case.caps, case.spec()
    g_out = torch.from_numpy(case.g_out[rank]).to(DEV)
    g_wide = None if case.g_wide[rank] is None else torch.from_numpy(case.g_wide[rank]).to(DEV)
    g_fm = None if case.g_fm[rank] is None else torch.from_numpy(case.g_fm[rank]).to(DEV)
    train = not case.forward_only and not case.overflow
    if case.forward_only:
        with pytest.raises(ValueError, match="64 features"):
            step.bind_backward(g_out, g_fm, direct_grad=form["direct_grad"], g_wide=g_wide)
        step.bwd = None
    elif train:
        step.bind_backward(g_out, g_fm, direct_grad=form["direct_grad"], g_wide=g_wide)
    runs = []
    for it in range(1 if case.overflow else 2):
        out, wide, fm = step.run()
        entries = step.backward() if train else []
        torch.cuda.synchronize()
        if barrier is not None:
            barrier()                   # (one-sided: every peer's placing launch has finished before anyone reads its buffer)
        runs.append((out.cpu().numpy().copy(), None if wide is None else wide.cpu().numpy().copy(),
                     None if fm is None else fm.cpu().numpy().copy(), _entries_np(entries, names_of)))
    res = dict(rank=rank, paths=_observed_paths(step, case, form), out=runs[-1][0], wide=runs[-1][1], fm=runs[-1][2], entries=runs[-1][3])
    # the overflow report: this rank's own blocks (overflowed(), no collective), then check() on every rank together
    from oracle import ref_np as R
    mine = False
    for gi, idxs in enumerate(groups):
        if gi not in pooled:
            mine |= R.route_feat([case.inputs[rank][i] for i in idxs], W, max(1, B))[4] > case.caps[gi]
    step.run()
    torch.cuda.synchronize()
    assert step.overflowed() == mine
    step.run()
    if case.overflow:
        with pytest.raises(RuntimeError, match="overflowed"):
            step.check()
    else:
        step.check()
    torch.cuda.synchronize()
    if barrier is not None:
        barrier()
    # writes stay inside the concat (its stride padding and the rows past B keep the sentinel)
    W_out = plan.out_width
    assert bool((big[:B, W_out:] == SENTINEL).all()) and bool((big[B:] == SENTINEL).all()), "a write outside the concat"
    assert bool((bigfm[B:] == SENTINEL).all()) and (plan.use_fm or bool((bigfm == SENTINEL).all()))
    if case.overflow:
        return res
    # two runs: the same bits
    a, b = runs
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), "two runs differ (concat)"
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert (x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)), "two runs differ (wide / fm)"
    assert len(a[3]) == len(b[3])
    for (n0, d0, k0, v0), (n1, d1, k1, v1) in zip(a[3], b[3]):
        assert n0 == n1 and np.array_equal(k0, k1) and np.array_equal(v0.view(np.int32), v1.view(np.int32)), "two runs differ (keys, values)"
    if not train:
        return res
    # the dummy row (and the padding row of a replicated table) carries no gradient; the global padding row (rank 0's arena row 1) is never keyed
    for tn, dim, keys, vals in res["entries"]:
        t_of = np.array([tn[k] for k in (keys >> 40)]) if keys.size else np.zeros(0, object)
        rows = keys & MASK
        assert not vals[rows == 0].any(), "a padding / dummy row has a gradient"
        if rank == 0:
            assert not np.any((rows == 1) & np.array([t not in rep_tables for t in t_of], bool)), "the global padding row was keyed"
    # one FusedSparseAdam step on the arenas against float64 Adam applied to the step's own gradient values
    if W == 1 or not (form["one_sided"] or form["direct_grad"]):
        before = {t: x.clone() for t, x in arenas.items()}
        sink = ops.SparseGradSink()
        sink.pending.extend(entries)
        opt = FusedSparseAdam(sink, lr=LR, betas=BETAS, eps=ADAM_EPS)
        g64 = {t: torch.zeros(x.shape, dtype=torch.float64, device=DEV) for t, x in arenas.items()}
        looked = {t: torch.zeros(x.shape[0], dtype=torch.bool, device=DEV) for t, x in arenas.items()}
        for e in entries:
            nu = int(e["counts"][0])
            k, v = e["uniq"][:nu], e["values"][:nu].double()
            for ti, tab in enumerate(e["tables"]):
                sel = (k >> 40) == ti
                if not bool(sel.any()):
                    continue
                t = names_of[id(tab)]
                g64[t].index_add_(0, k[sel] & MASK, v[sel])
                looked[t][k[sel] & MASK] = True
        opt.step()
        torch.cuda.synchronize()
        b1, b2 = (float(np.float32(x)) for x in BETAS)
        step_size = float(np.float32(LR * math.sqrt(1.0 - BETAS[1]) / (1.0 - BETAS[0])))
        for t, tab in arenas.items():
            lk = looked[t]
            assert torch.equal(tab[~lk].view(torch.int32), before[t][~lk].view(torch.int32)), f"{t}: an untouched row moved"
            assert float(tab[0].abs().max()) == 0.0, f"{t}: the dummy / padding row moved"
            if rank == 0 and t not in rep_tables and tab.shape[0] > 1:
                assert float(tab[1].abs().max()) == 0.0, f"{t}: the global padding row moved"
            if not bool(lk.any()):
                continue
            g = g64[t][lk]
            m64, v64 = (1 - b1) * g, (1 - b2) * g * g
            upd = m64 / (v64.sqrt() + ADAM_EPS)
            w64 = before[t][lk].double() - step_size * upd
            gerr = 4 * _ulp32(g)
            tol = 4 * _ulp32(w64) + 8 * _ulp32(step_size * upd) + step_size * 1e-6 * (gerr / (g.abs() + ADAM_EPS)).clamp(max=1)
            err = (tab[lk].double() - w64).abs()
            assert bool((err <= tol).all()), f"{t}: weights beyond a few ulp of float64 Adam: max {float(err.max())}\n{case.spec()}"
        res["adam"] = True
    return res


def _dense_grads(case, results):
    """Per table the float64 sum of the ranks' (key, value) pieces over GLOBAL rows; the replicated tables' entries from rank 0 (equal on
    every rank: checked word for word)."""
    rep_tables = {f.table for f in case.feats if f.replicated}
    W = case.world
    g = {t: np.zeros(x.shape, np.float64) for t, x in case.tables.items()}
    rep_lists = {}
    for res in results:
        r = res["rank"]
        mine = []
        for tn, dim, keys, vals in res["entries"]:
            t_of = [tn[k] for k in (keys >> 40)]
            rows = keys & MASK
            for t in set(t_of):
                sel = np.array([x == t for x in t_of], bool)
                if t in rep_tables:
                    mine.append((t, keys[sel], vals[sel]))
                    if r == 0:
                        np.add.at(g[t], rows[sel], vals[sel].astype(np.float64))
                    continue
                live = sel & (rows > 0)
                np.add.at(g[t], (rows[live] - 1) * W + r, vals[live].astype(np.float64))
        rep_lists[r] = sorted(mine, key=lambda x: x[0])
    for r in range(1, W):
        assert len(rep_lists[r]) == len(rep_lists[0])
        for (t0, k0, v0), (t1, k1, v1) in zip(rep_lists[0], rep_lists[r]):
            assert t0 == t1 and np.array_equal(k0, k1) and np.array_equal(v0.view(np.int32), v1.view(np.int32)), \
                f"replicated entries of {t0} differ between rank 0 and rank {r}"
    return g


def _direct(case):
    """The direct bound path on full tables over the rank-major concatenation: (out, wide, fm, {(table, row): value})."""
    from news_recsys_amd import ops
    ec = S.truth_case(case)
    names = case.table_names
    tabs = [torch.from_numpy(case.tables[t]).to(DEV) for t in names]
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in ec.inputs]
    ws = [None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(DEV) for w in ec.weights]
    plan = ec.plan()
    single = len(plan.slots) <= 64
    sums = None
    if plan.use_fm and single:
        sums = torch.empty((ec.B, max(s.dim for s in ec.slots if s.fm_field)), dtype=torch.float32, device=DEV)
    fwd = ops.PreparedEmbed(plan, tabs, ins, ws, out_ld=case.ld, fm_sums=sums)
    out, wide, fm = fwd.run()
    kv = None
    if single:
        groups = ops.PreparedSparseBackward(fwd, torch.from_numpy(ec.g_out).to(DEV), g_fm=None if ec.g_fm is None else torch.from_numpy(ec.g_fm).to(DEV),
                                            g_wide=None if ec.g_wide is None else torch.from_numpy(ec.g_wide).to(DEV)).run()
        kv = {}
        for g in groups:
            nu = int(g["counts"][0])
            for k, v in zip(g["uniq"][:nu].cpu().numpy(), g["values"][:nu].cpu().numpy()):
                if k & MASK:
                    kv[(names[k >> 40], int(k & MASK))] = v
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if wide is None else wide.cpu().numpy(), None if fm is None else fm.cpu().numpy(), kv


def _within(got, ref, A, n, what, case):
    if not torch.is_tensor(got):
        got = torch.from_numpy(np.ascontiguousarray(got))
    got = got.to(ref.device)
    ex, i = E.excess(got, ref, A, n)
    idx = np.unravel_index(max(i, 0), tuple(ref.shape)) if ref.numel() else ()
    assert ex <= 0, f"{what}: element {tuple(int(x) for x in idx)} beyond the bound by {ex:.3g}: got {float(got.reshape(-1)[i])} " \
                    f"want {float(ref.reshape(-1)[i])} (A {float(A.reshape(-1)[i]):.3g}, n {n})\n{case.spec()}"


def check_results(case, form, results):
    """The ranks' results (rank order) against the float64 truth and the direct path on the concatenated batch."""
    assert sorted(res["rank"] for res in results) == list(range(case.world))
    results = sorted(results, key=lambda r: r["rank"])
    routed_rows = [case.tables[f.table].shape[0] for f in case.feats if f.table and not f.replicated]
    for res in results:
        r = res["rank"]
        want = sorted((set(form["paths"]) - {"empty_shard"}) | ({"empty_shard"} if any(n <= r for n in routed_rows) else set()))
        assert res["paths"] == want, f"rank {r} took {res['paths']}, predicted {want}\n{case.spec()}"
    if case.overflow:
        return
    groups, pooled, plan = case.plan()
    W_out = plan.out_width
    ref = S.restate(case, DEV, grads=not case.forward_only)
    n_out, n_fm, n_grads = S.chains(case, ref)
    out = np.concatenate([r["out"][:, :W_out] for r in results])
    cc = ref.copy_cols
    if cc:
        assert np.array_equal(out[:, cc], ref.out[:, cc].float().cpu().numpy()), f"copied columns differ\n{case.spec()}"
    _within(out, ref.out, ref.A_out, n_out, "concat", case)
    if plan.wide_width:
        wide = np.concatenate([r["wide"] for r in results])
        _within(wide, ref.wide, ref.A_wide, n_out, "wide", case)
    if plan.use_fm:
        fm = np.concatenate([r["fm"] for r in results])
        _within(fm, ref.fm, ref.A_fm, n_fm, "fm", case)
    # the direct path: non-pooled columns, wide, the fused FM logit and the (key, value) of every table no pooled bag feeds, word for word
    d_out, d_wide, d_fm, d_kv = _direct(case)
    pooled_feat = [f.kind in S.BAGS and not f.replicated for f in case.feats]
    cols = [c for i, s in enumerate(plan.slots) if not pooled_feat[i]
            for c in range(s.out_col, s.out_col + s.dim - (1 if s.wide_col >= 0 else 0))]
    assert np.array_equal(out[:, cols].view(np.int32), d_out[:, cols].view(np.int32)), f"non-pooled columns != the direct path\n{case.spec()}"
    if plan.wide_width:
        assert np.array_equal(wide.view(np.int32), d_wide.view(np.int32)), "wide != the direct path"
    if plan.use_fm and "fm_pass" not in form["paths"]:
        assert np.array_equal(fm.view(np.int32), d_fm.view(np.int32)), "fused FM logit != the direct path"
    if case.forward_only:
        return
    g = _dense_grads(case, results)
    names = case.table_names
    for t, name in enumerate(names):
        got = torch.from_numpy(g[name]).to(DEV)
        _within(got, ref.grads[t], ref.A_grads[t], n_grads[t], f"gradient of table {name}", case)
        assert bool((got[ref.A_grads[t] == 0] == 0).all()), f"a row that was not looked up has a gradient ({name})"
    # word for word where the step's reduction is the direct path's launch: routed tables whose width no bag feature shares (a bag in the
    # direct path's launch of that width doubles its long-row threshold: other rows go to the tree-summed work lists), and at world 1 the
    # replicated tables whose width no routed bag shares (above world 1 they are the rank-order fold of the ranks' sums)
    W = case.world
    rep_tables = {f.table for f in case.feats if f.replicated}
    bag_dims = {f.dim for f in case.feats if f.kind in S.BAGS}
    routed_bag_dims = {f.dim for f, pf in zip(case.feats, pooled_feat) if pf}
    bagged = {t for t, x in case.tables.items()
              if (x.shape[1] in bag_dims if t not in rep_tables else (W > 1 or x.shape[1] in routed_bag_dims))}
    got_kv = {}
    for res in results:
        for tn, dim, keys, vals in res["entries"]:
            for k, v in zip(keys, vals):
                t, row = tn[k >> 40], int(k & MASK)
                if t in bagged or row == 0 or (t in rep_tables and res["rank"] > 0):     # (replicated: equal on every rank, checked above)
                    continue
                key = (t, row) if t in rep_tables else (t, (row - 1) * W + res["rank"])
                assert key not in got_kv, f"{key} keyed twice"
                got_kv[key] = v
    want = {k: v for k, v in d_kv.items() if k[0] not in bagged}
    assert set(got_kv) == set(want), f"keys != the direct path: {sorted(set(got_kv) ^ set(want))[:5]}\n{case.spec()}"
    for key, v in want.items():
        assert np.array_equal(got_kv[key].view(np.int32), v.view(np.int32)), f"{key}: value != the direct path\n{case.spec()}"


# ------------------------------------------------------------------------------------------------- world 1
@pytest.mark.parametrize("seed", W1_SEEDS)
def test_world_1_step_against_float64_and_the_direct_path(seed):
    from news_recsys_amd.sharding import RowShardedEmbedding
    case = S.case(seed)
    for form in case.forms:
        with applied(case, form):
            eng = RowShardedEmbedding(0, 1, slack=case.slack, overflow_policy="defer")
            res = rank_run(case, form, 0, eng)
            check_results(case, form, [res])
            if not case.forward_only:
                assert res.get("adam")


def test_seed_list_reaches_every_path():
    """Independent of test order and -k: for every predicted world-1 path, the first seed that predicts it is bound and the step's own
    attributes show the path taken."""
    from news_recsys_amd.sharding import RowShardedEmbedding
    done = set()
    for sd in W1_SEEDS:
        case = S.case(sd)
        for form in case.forms:
            if set(form["paths"]) <= done:
                continue
            with applied(case, form):
                res = rank_run(case, form, 0, RowShardedEmbedding(0, 1, slack=case.slack, overflow_policy="defer"))
            assert res["paths"] == form["paths"], (sd, res["paths"], form["paths"])
            done |= set(form["paths"])
    assert {"placed", "direct_grad", "bwd_scatter", "bwd_fallback", "fwd_split", "fm_pass", "forked", "pooled_binary", "pooled_expand",
            "route_bags:runs", "route_bags:one", "route_bags:legacy", "plan:inline", "plan:backward", "plan:forward", "replicated_w1"} <= done


@pytest.mark.parametrize("how", ["runs", "one", "legacy"])
@pytest.mark.parametrize("D", [17, 24, 33, 300])
def test_regression_pooled_partials_of_widths_past_the_lane_group(D, how, monkeypatch):
    """Regression (generated seeds 2, 18, 38): nrx_pool_inbox_fwd(_runs) hands each run's {row, weight} words across the lane group with
    __shfl; the lanes whose columns lay past D (D = 17, 24, 33, 300) left the column loop and fed stale words to the others -- wrong pooled
    columns for every bag longer than the active lanes' share of entries.  The pooled columns against float64, every routing form."""
    from news_recsys_amd import shard_step
    from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN
    from news_recsys_amd.sharding import RowShardedEmbedding, ShardedFeature
    monkeypatch.setenv("NRX_ROUTE_BAGS", how)
    rng = np.random.default_rng(D)
    B, L, rows = 300, 50, 5000
    table = rng.standard_normal((rows, D)).astype(np.float32)
    table[0] = 0
    mask = (rng.random((B, L)) < 0.8).astype(np.float32)
    mask[: 4] = 1                                          # full bags: runs of L entries
    ids = rng.integers(1, rows, (B, L)) * mask.astype(np.int64)
    arenas = {"t": shard_step.make_arena(rows, D, 0, 1, DEV, full=torch.from_numpy(table).to(DEV))}
    step = shard_step.PreparedShardedStep(RowShardedEmbedding(0, 1, overflow_policy="defer"), [ShardedFeature("h", NRX_BAG_MASKED_MEAN, "t", D, L)],
                                          [torch.from_numpy(ids).to(DEV)], [torch.from_numpy(mask).to(DEV)], arenas, train=False)
    out = step.run()[0].cpu().numpy()
    m = mask.astype(np.float64)
    want = (table[ids].astype(np.float64) * m[:, :, None]).sum(1) / (m.sum(1, keepdims=True) + 1e-8)
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-5)


def test_the_sharded_step_refuses_bf16_tables():
    from news_recsys_amd import shard_step
    full = torch.zeros((10, 16), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(NotImplementedError, match="bf16"):
        shard_step.make_arena(10, 16, 0, 1, DEV, full=full)
