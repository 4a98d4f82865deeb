"""CPU checks of the generated sharded steps (tests/shard_cases.py): the generator is deterministic, its seed list covers every generator
feature and every predicted path, its block sizes follow the step's formulas and the oracle's routing, and the float64 truth it builds
(embed_cases.restate over the concatenated batch, the step's final-plan columns) agrees with the oracle's fp32 definitions."""
import numpy as np
import pytest

from oracle import ref_np as R
from tests import embed_cases as E
from tests import shard_cases as S
from tests.test_embed_cases import _check, _oracle_fp32

F32 = np.float32


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and np.array_equal(a, b)


def test_the_generator_is_deterministic():
    for sd in (0, 5, 9, 18, 47):
        a, b = S.make_case(sd), S.make_case(sd)
        assert a.feats == b.feats and a.forms == b.forms and a.knobs == b.knobs and a.paths == b.paths
        assert (a.world, a.B, a.slack, a.out_ld, a.edge, a.caps, a.block_max) == (b.world, b.B, b.slack, b.out_ld, b.edge, b.caps, b.block_max)
        assert sorted(a.tables) == sorted(b.tables) and all(np.array_equal(a.tables[t], b.tables[t]) for t in a.tables)
        for r in range(a.world):
            assert all(_same(x, y) for x, y in zip(a.inputs[r], b.inputs[r]))
            assert all(_same(x, y) for x, y in zip(a.weights[r], b.weights[r]))
            assert _same(a.g_out[r], b.g_out[r]) and _same(a.g_wide[r], b.g_wide[r]) and _same(a.g_fm[r], b.g_fm[r])
        assert a.spec() == b.spec()


REQUIRED = [
    "world:1", "world:2", "world:3", "batch:<64", "batch:64", "batch:<=4096", "batch:>4096",
    "kind:sparse", "kind:masked_mean", "kind:mean", "kind:sum", "kind:dense",
    "kind:sparse:replicated", "kind:masked_mean:replicated", "kind:mean:replicated", "kind:sum:replicated",
    "ids:int32", "ids:int64", "table_shared", "table_shared_by_id_and_bag", "empty_shard",
    "bag:empty", "bag:float_weights", "bag:binary_mask", "wide", "fm_field:routed", "fm_field:replicated", "fm:placeable", "fm:on",
    "out_ld:padded_x4", "out_ld:padded_odd", "forward_only", "slack:overflow_free", "edge:capf", "edge:capf+1",
    "form:all_to_all/buffered", "form:all_to_all/direct", "form:one_sided/buffered", "form:one_sided/direct", "form:binary_masks",
    "overlap:1", "overlap:0", "overlap:fwd", "overlap:bwd",
    "knob:PLAN_LDS=0", "knob:PLAN_LDS=1", "knob:PAD_SPLIT=0", "knob:PAD_SPLIT=1", "knob:SPARSE_PLACE=False",
    "knob:DENSE_SORTED_MIN=lowered", "knob:DENSE_LDS_MIN=lowered", "knob:PAD_SPLIT_MIN=lowered",
] + [f"width:{w}" for w in S.WIDTHS] + [f"bag_len:{L}" for L in S.BAG_LENS]

PATHS = ["placed", "direct_grad", "bwd_scatter", "bwd_fallback", "fwd_split", "fm_pass", "forked", "route_bags:runs", "route_bags:one",
         "route_bags:legacy", "pooled_binary", "pooled_expand", "plan:inline", "plan:backward", "plan:forward", "replicated_w1",
         "replicated_fold", "empty_shard"]


def test_seed_list_covers_every_generator_feature_and_path():
    cov = S.coverage()
    missing = [k for k in REQUIRED + [f"path:{p}" for p in PATHS] if not cov.get(k)]
    assert not missing, f"no seed of the list shows {missing}"
    # the paths the GPU tests run in process (world 1) -- and those only the rank processes reach
    w1 = {p for sd in S.SEEDS for p in S.make_case(sd).paths if S.make_case(sd).world == 1}
    assert {"placed", "direct_grad", "bwd_fallback", "fwd_split", "fm_pass", "forked", "replicated_w1"} <= w1
    assert cov["edge:capf+1"] and all(S.make_case(sd).world > 1 for sd in cov["edge:capf+1"] + cov["path:replicated_fold"])


@pytest.mark.parametrize("seed", S.SEEDS)
def test_block_sizes_follow_the_step_and_the_oracle_routing(seed):
    """caps = the step's formulas (capf of a single-valued group, capacity_for of a pooled one); block_max of a single-valued group =
    the largest count of oracle.ref_np.route_feat over the ranks; the overflow-free slack leaves every block within its cap; the edge seeds
    fill their largest block to exactly capf (+ 1)."""
    c = S.make_case(seed)
    groups, pooled, plan = c.plan()
    assert len(c.caps) == len(groups) == len(c.block_max)
    for gi, idxs in enumerate(groups):
        if gi in pooled:
            assert c.caps[gi] == S.pooled_cap_of(c.B * sum(c.feats[i].bag_len for i in idxs), c.world, c.slack)
            assert len({c.feats[i].table for i in idxs}) == 1                       # one table per pooled group
            continue
        capf = S.capf_of(c.B, c.world, c.slack)
        assert c.caps[gi] == capf and capf % (64 if c.world > 1 else 1) == 0
        worst = 0
        for r in range(c.world):
            _, _, slot, counts, mx = R.route_feat([c.inputs[r][i] for i in idxs], c.world, capf)
            assert mx == int(counts.max())
            assert ((slot == -1).sum() > 0) == (mx > capf)                         # a block past capf drops lookups
            worst = max(worst, mx)
        assert worst == c.block_max[gi]
        assert len({c.inputs[0][i].dtype for i in idxs}) == 1                       # one id dtype per exchange group
    if not c.edge:
        assert not c.overflow
    else:
        assert c.block_max[0] == c.caps[0] + (1 if c.edge == "capf+1" else 0)
        assert c.overflow == (c.edge == "capf+1")
        assert all(m <= cap for m, cap in zip(c.block_max[1:], c.caps[1:]))
    for t, x in c.tables.items():
        assert not x[0].any()                                                       # row 0 zero, as make_arena leaves it
    for r in range(c.world):
        for f, x in zip(c.feats, c.inputs[r]):
            if f.kind != 0 and f.table and c.B >= 4:
                assert (x == 0).any()                                               # the padding id in every feature


def _cheap(k):
    out = []
    for sd in S.SEEDS:
        c = S.make_case(sd)
        if c.lookups() * max(f.dim for f in c.feats) <= 1 << 20 and not c.edge:
            out.append(sd)
    picked = [sd for sd in out if S.make_case(sd).world > 1][:k] + [sd for sd in out if S.make_case(sd).world == 1][:k]
    return sorted(picked)


@pytest.mark.parametrize("seed", _cheap(3))
def test_the_truth_agrees_with_the_oracle(seed):
    """truth_case (the step as one launch over the rank-major concatenation, the step's final-plan columns) restated in float64 against
    the oracle's fp32 definitions of the same launch: copies bit for bit, everything else within the bound -- with the sharded chains
    (chains()) at least as long as restate's own."""
    import torch
    case = S.make_case(seed)
    ec = S.truth_case(case)
    _, _, plan = case.plan()
    assert [s.out_col for s in ec.slots] == [s.out_col for s in plan.slots] and ec.out_width == plan.out_width
    assert ec.B == case.world * case.B and ec.g_out.shape == (ec.B, case.ld)
    ref = S.restate(case)
    n_out, n_fm, n_grads = S.chains(case, ref)
    assert n_out >= ref.n_out and n_fm >= ref.n_fm and all(a >= b for a, b in zip(n_grads, ref.n_grads))
    out, wide, fm, grads = _oracle_fp32(ec, order_seed=seed)
    cc = ref.copy_cols
    assert np.array_equal(out[:, cc], ref.out[:, cc].numpy().astype(F32)), case.spec()
    _check(out, ref.out, ref.A_out, ref.n_out, "concat")
    if ec.wide_width:
        _check(wide, ref.wide, ref.A_wide, ref.n_out, "wide")
    if ec.use_fm:
        _check(fm, ref.fm, ref.A_fm, ref.n_fm, "fm")
    for t, g in enumerate(grads):
        _check(g, ref.grads[t], ref.A_grads[t], ref.n_grads[t], f"grad of table {t}")
        assert torch.all((ref.A_grads[t] == 0) <= (ref.grads[t] == 0))
    # the concatenation is rank-major: rank r's samples are rows r * B .. (r + 1) * B of the truth
    for r in range(case.world):
        for i, f in enumerate(case.feats):
            assert np.array_equal(ec.inputs[i][r * case.B:(r + 1) * case.B], case.inputs[r][i])


def test_regression_seeds_still_draw_what_found_their_bug():
    for sd in S.REGRESSIONS["pooled_width_past_the_lane_group"]:
        c = S.make_case(sd)
        assert any(f.kind in S.BAGS and not f.replicated and f.dim % 16 and f.bag_len > 16 for f in c.feats), c.spec()


def test_forward_only_cases_exceed_the_backward_limit_and_split_the_exchange():
    for sd in S.SEEDS:
        c = S.make_case(sd)
        groups, _, _ = c.plan()
        if c.forward_only:
            assert len(c.feats) > E.NRX_MAX_FEATURES and len(groups) >= 2 and all(len(g) <= 64 for g in groups)
            assert "fwd_split" in c.paths
