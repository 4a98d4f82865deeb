"""Generated bound sharded training steps and their float64 truth (a helper of the tests, not a conftest).

make_case(seed) draws one PreparedShardedStep (news_recsys_amd/shard_step.py) from numpy's default_rng(seed), using only what the step
accepts: routed single-valued features of widths 1 to 300 (tables shared between features, tables with fewer rows than ranks, uniform or
Zipf ids with the padding id and the last row in every feature, one id dtype per embedding width), pooled bags (masked mean, mean, sum;
lengths 1 to 130; 0/1 masks, float weights, empty bags, padded histories; one table per pooled group), replicated tables (single ids and
bags, wide columns, FM fields), dense features, an FM epilogue that does and does not qualify for one-sided placement, a padded `out_ld`,
per-rank batches from 1 to 20 000, and forward-only cases of 65-70 features.  Each case names its world (1, 2 or 3), its per-rank batches
and upstream gradients, its `slack` (no block overflows, except the edge seeds that fill the largest (owner, feature) block to exactly
capf or capf + 1), the forms to run (one_sided, direct_grad, binary_masks, NRX_ROUTE_BAGS, NRX_SHARD_OVERLAP, NRX_SHARD_PLAN) and the
ops.* planner knobs, rotated as embed_cases rotates them.

form_paths(case, form) predicts the step's code paths from the same rules shard_step.py applies; expected_paths(case) is their union.

truth_case(case) / restate(case) is the float64 restatement of the whole step: an embed_cases.Case over the rank-major concatenation of the ranks' batches,
with the step's final-plan columns, whose restate() gives the concat, wide, FM and table gradients and the error scale A.  chains(case,
ref) lengthens its rounding chains for the sharded order: + world for pooled columns (the requester adds the owners' partials) and for
the tables fed by pooled or replicated features (the owners' reduction of expanded bag entries, the rank-order fold).

REGRESSIONS names the seeds that found a bug in the product code.

    python -m tests.shard_cases SEED      prints the case
"""
from __future__ import annotations

import functools
import sys
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np

from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM, NRX_DENSE, NRX_MAX_FEATURES, NRX_SPARSE
from tests import embed_cases as E

KIND_NAMES = E.KIND_NAMES
BAGS = (NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM)
WIDTHS = (1, 2, 5, 8, 16, 17, 32, 33, 64, 128, 256, 300)
PLACE_WIDTHS = (16, 32, 64, 128, 256)          # one-sided placement (shard_step.py: placed_groups)
DIRECT_WIDTHS = (16, 32, 64)                   # direct_grad and the placement pass of nrx_embed_bwd_scatter
BATCHES = (1, 63, 64, 65, 700, 4095, 4096, 4097, 9000, 20000)
BAG_LENS = (1, 2, 7, 33, 130)
ROWS = (2, 3, 50, 1000, 30000, 200000)
MAX_LOOKUPS = 300_000                 # over all ranks: the float64 restatement and the host-staged exchanges stay well under a second
MAX_GATHERED = 1 << 22                # lookups x dim over all ranks
MAX_TABLE_ELEMS = 1 << 21
SLACKS = (0.05, 0.3, 1.0)             # the smallest under which no block overflows is taken (world - 1 always fits)
SEEDS = tuple(range(48))
ROUTE_BAGS = ("runs", "one", "legacy")
OVERLAP = ("1", "0", "fwd", "bwd")
PLAN_MODES = ("inline", "backward", "forward")
RF_TILE = 4096                        # ids per block of the routing launches (csrc/nrx_route_feat.hip)


@dataclass
class FeatSpec:
    """One feature (the fields of sharding.ShardedFeature)."""
    name: str
    kind: int
    table: str                         # '' for dense
    dim: int
    bag_len: int = 0
    wide: bool = False
    fm: bool = False
    replicated: bool = False


@dataclass
class ShardCase:
    seed: int
    style: str
    world: int
    B: int                                          # per rank
    feats: List[FeatSpec]
    tables: Dict[str, np.ndarray]                   # full float32 [rows, dim], row 0 zero
    inputs: List[List[np.ndarray]]                  # [rank][feature]: ids [B] | [B, L]; dense values float32 [B]
    weights: List[List[Optional[np.ndarray]]]       # [rank][feature]: None | float32 [B, L]
    g_out: List[np.ndarray]                         # [rank]: float32 [B, ld] (the stride padding holds values no backward may read)
    g_wide: List[Optional[np.ndarray]]
    g_fm: List[Optional[np.ndarray]]
    out_ld: Optional[int]                           # None: the plan's width
    slack: float
    forward_only: bool
    edge: str = ""                                  # "" | "capf" | "capf+1": the largest single-valued block filled to capf (+ 1)
    forms: List[dict] = field(default_factory=list)
    knobs: Dict[str, object] = field(default_factory=dict)
    caps: List[int] = field(default_factory=list)          # per exchange group: capf (single-valued) or cap (pooled), as the step computes it
    block_max: List[int] = field(default_factory=list)     # per exchange group: the largest (owner, feature) / (owner) block over the ranks
    paths: List[str] = field(default_factory=list)

    @property
    def table_names(self) -> List[str]:
        return sorted(self.tables)

    @property
    def overflow(self) -> bool:
        return any(m > c for m, c in zip(self.block_max, self.caps))

    def sharded_features(self):
        from news_recsys_amd.sharding import ShardedFeature
        return [ShardedFeature(f.name, f.kind, f.table, f.dim, f.bag_len, f.wide, f.fm, f.replicated) for f in self.feats]

    def engine(self, rank: int = 0, **kw):
        from news_recsys_amd.sharding import RowShardedEmbedding
        return RowShardedEmbedding(rank, self.world, slack=self.slack, overflow_policy="defer", **kw)

    def plan(self):
        """(groups, pooled group indices, the step's final plan) -- what PreparedShardedStep computes from the features."""
        eng = self.engine()
        feats = self.sharded_features()
        groups, pooled = eng.plan_groups(feats)
        return groups, pooled, eng._final_plan(feats, groups, pooled)

    @property
    def ld(self) -> int:
        return self.out_ld if self.out_ld else self.plan()[2].out_width

    def lookups(self) -> int:
        return self.world * self.B * sum(max(1, f.bag_len) for f in self.feats if f.kind != NRX_DENSE)

    def spec(self) -> str:
        groups, pooled, plan = self.plan()
        head = (f"seed {self.seed} ({self.style}): world={self.world} B={self.B}/rank  features={len(self.feats)}  out_width={plan.out_width} "
                f"out_ld={self.out_ld}  wide_width={plan.wide_width}  fm={plan.use_fm}  slack={self.slack}  edge={self.edge or '-'}  "
                f"forward_only={self.forward_only}  lookups={self.lookups()}")
        lines = [head, f"  knobs: {self.knobs}", f"  paths: {self.paths}"]
        for k, fm in enumerate(self.forms):
            lines.append(f"  form {k}: {fm}")
        for gi, idxs in enumerate(groups):
            lines.append(f"  group {gi}: {'pooled' if gi in pooled else 'single'} feats={idxs} cap={self.caps[gi]} block_max={self.block_max[gi]}")
        for t in self.table_names:
            lines.append(f"  table {t}: rows={self.tables[t].shape[0]} dim={self.tables[t].shape[1]}")
        for i, f in enumerate(self.feats):
            x, w = self.inputs[0][i], self.weights[0][i]
            wdesc = "-" if w is None else ("0/1 mask" if np.all((w == 0) | (w == 1)) else "weights")
            lines.append(f"  {f.name}: {KIND_NAMES[f.kind]} table={f.table or '-'} dim={f.dim} L={f.bag_len} col={plan.slots[i].out_col} "
                         f"wide={f.wide} fm={f.fm} rep={f.replicated} ids={x.dtype}{list(x.shape)} w={wdesc}")
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------- the step's sizes (copies of its formulas)
def capf_of(B: int, world: int, slack: float) -> int:
    """shard_step.PreparedShardedStep: the capacity of one (owner, feature) block of a single-valued exchange group."""
    return B if world == 1 else (int(B / world * (1.0 + slack)) + 64 + 63) // 64 * 64


def pooled_cap_of(n_total: int, world: int, slack: float) -> int:
    """sharding.RowShardedEmbedding.capacity_for: the capacity of one owner's block of a pooled group (all its features)."""
    if world == 1:
        return max(64, n_total)
    return (int(n_total / world * (1.0 + slack)) + 256 + 63) // 64 * 64


def _block_max(case: ShardCase, groups, pooled) -> List[int]:
    """Per group, the largest block any rank's routing fills: single-valued groups from oracle.ref_np.route_feat's counts, pooled groups
    from the entries with a non-zero weight per owner (what nrx_route_bags* send)."""
    from oracle import ref_np as R
    W = case.world
    out = []
    for gi, idxs in enumerate(groups):
        worst = 0
        for r in range(W):
            if gi in pooled:
                fill = np.zeros(W, np.int64)
                for i in idxs:
                    x = np.asarray(case.inputs[r][i], np.int64)
                    w = case.weights[r][i]
                    live = np.ones(x.shape, bool) if (w is None or case.feats[i].kind == NRX_BAG_MEAN) else (w != 0)
                    fill += np.bincount((x[live] % W).reshape(-1), minlength=W)
                worst = max(worst, int(fill.max()))
            else:
                worst = max(worst, R.route_feat([case.inputs[r][i] for i in idxs], W, max(1, case.B))[4])      # (counts: whatever capf)
        out.append(worst)
    return out


def _caps(case: ShardCase, groups, pooled, slack: float) -> List[int]:
    caps = []
    for gi, idxs in enumerate(groups):
        if gi in pooled:
            caps.append(pooled_cap_of(sum(case.B * case.feats[i].bag_len for i in idxs), case.world, slack))
        else:
            caps.append(capf_of(case.B, case.world, slack))
    return caps


# ------------------------------------------------------------------------------------------------- generator
def _ids(rng, rows: int, shape, zipf: bool) -> np.ndarray:
    return E._ids(rng, rows, shape, zipf)


def _rows(rng, dim: int, world: int) -> int:
    return max(2, min(int(rng.choice(ROWS)), max(2, MAX_TABLE_ELEMS // dim)))


def _draw_features(rng, style: str, world: int):
    """Features and table shapes of one case: ({name: (rows, dim)}, [FeatSpec])."""
    tables: Dict[str, tuple] = {}
    feats: List[FeatSpec] = []
    rep_tables = set()
    if style == "many":                                   # forward only: 65-70 single-valued routed features of one width, few shared tables
        n_feat = int(rng.integers(NRX_MAX_FEATURES + 1, 71))
        dim = int(rng.choice([4, 8, 16]))
        n_tab = int(rng.integers(1, 4))
        for t in range(n_tab):
            tables[f"t{t}"] = (int(rng.choice([50, 1000, 30000])), dim)
        fm = rng.random() < 0.5
        for f in range(n_feat):
            feats.append(FeatSpec(f"f{f:02d}", NRX_SPARSE, f"t{int(rng.integers(0, n_tab))}", dim, fm=fm))
        return tables, feats
    if style == "fm_placed":                              # every feature an FM field of one placeable width: fm_ok
        dim = int(rng.choice(PLACE_WIDTHS))
        n_feat = int(rng.integers(2, 9))
        n_tab = int(rng.integers(1, n_feat + 1))
        for t in range(n_tab):
            tables[f"t{t}"] = (_rows(rng, dim, world), dim)
        for f in range(n_feat):
            feats.append(FeatSpec(f"f{f:02d}", NRX_SPARSE, f"t{min(f, n_tab - 1) if f < n_tab else int(rng.integers(0, n_tab))}", dim, fm=True))
        return tables, feats
    if style == "edge":                                   # an (owner, feature) block filled to exactly capf (+ 1): one routed group
        dim = int(rng.choice([16, 17, 32]))
        n_feat = int(rng.integers(1, 4))
        for f in range(n_feat):
            tables[f"t{f}"] = (int(rng.choice([1000, 30000])), dim)
            feats.append(FeatSpec(f"f{f:02d}", NRX_SPARSE, f"t{f}", dim))
        return tables, feats
    # "mixed" / "tower" / "wide" / "fm_mixed"
    n_tab = int(rng.integers(1, 6))
    for t in range(n_tab):
        dim = int(rng.choice(WIDTHS))
        rep = rng.random() < (0.6 if style == "wide" else 0.25)
        rows = _rows(rng, dim, world)
        if world == 3 and not rep and rng.random() < 0.25:
            rows = 2                                      # fewer rows than ranks: rank 2's shard is empty
        if rep:
            rows = min(rows, 30000)
            rep_tables.add(f"t{t}")
        tables[f"t{t}"] = (rows, dim)
    if style == "tower":                                  # DSSM: an id and a history bag over one table, a user id
        dim = int(rng.choice([16, 32, 17]))
        tables = {"news": (int(rng.choice([50, 30000])), dim), "user": (int(rng.choice([1000, 200000])), dim)}
        rep_tables = set()
        L = int(rng.choice(BAG_LENS[1:]))
        feats = [FeatSpec("item_id", NRX_SPARSE, "news", dim), FeatSpec("history", int(rng.choice(BAGS)), "news", dim, L),
                 FeatSpec("user_id", NRX_SPARSE, "user", dim)]
        return tables, feats
    names = sorted(tables)
    n_feat = int(rng.choice([1, 2, 3, 5, 8, 12]))
    bag_table: Dict[int, str] = {}                        # one table per pooled group (routed bags of one width)
    for f in range(n_feat):
        if rng.random() < 0.1:
            feats.append(FeatSpec(f"f{f:02d}", NRX_DENSE, "", 1))
            continue
        t = str(rng.choice(names))
        rows, dim = tables[t]
        kind = int(rng.choice([NRX_SPARSE, NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM], p=[0.5, 0.2, 0.12, 0.18]))
        rep = t in rep_tables
        if kind != NRX_SPARSE and not rep:
            t = bag_table.setdefault(dim, t)
        L = 0 if kind == NRX_SPARSE else int(rng.choice(BAG_LENS))
        feats.append(FeatSpec(f"f{f:02d}", kind, t, dim, L, replicated=rep))
    if not any(f.kind != NRX_DENSE for f in feats):
        feats[0] = FeatSpec("f00", NRX_SPARSE, names[0], tables[names[0]][1], replicated=names[0] in rep_tables)
    # wide columns: replicated features only (the step refuses routed ones); never on an FM field
    if style == "wide" or rng.random() < 0.2:
        for f in feats:
            if f.replicated and f.dim >= 2 and rng.random() < 0.6:
                f.wide = True
    if style == "fm_mixed" or rng.random() < 0.15:
        # FM fields: single-valued routed features and replicated features of one width (a routed pooled bag is not an FM field here)
        dims = sorted({f.dim for f in feats if f.kind != NRX_DENSE and 2 <= f.dim <= 256})
        if dims:
            fm_dim = int(rng.choice(dims))
            cands = [f for f in feats if f.dim == fm_dim and f.kind != NRX_DENSE and not f.wide and (f.kind == NRX_SPARSE or f.replicated)]
            for f in cands:
                if rng.random() < 0.7 or f is cands[0]:
                    f.fm = True
    return tables, feats


def _bag(rng, kind: int, rows: int, B: int, L: int, zipf: bool, mode: float):
    """ids [B, L] and weights (None | [B, L]) of one bag feature on one rank: empty bags, padded histories, 0/1 masks and float weights
    (`mode`, drawn once per feature, picks the weights' form: the same on every rank)."""
    x = _ids(rng, rows, (B, L), zipf)
    valid = np.arange(L)[None, :] < rng.integers(0, L + 1, (B, 1))
    w = None
    if kind == NRX_BAG_MASKED_MEAN:
        x = x * valid                                     # padded histories: id 0 behind the valid entries
        w = valid.astype(np.float32) if mode < 0.6 else (valid * rng.uniform(0.25, 1.0, (B, L))).astype(np.float32)
    elif kind == NRX_BAG_SUM:
        if mode < 0.35:
            x = x * valid
            w = (valid * rng.uniform(-1.0, 1.0, (B, L))).astype(np.float32)
        elif mode < 0.7:
            x = x * valid
            w = valid.astype(np.float32)
    elif mode < 0.5:                                      # mean over L, padding included (row 0 is read)
        x = x * valid
    return x, w


def _binary_ok(case: ShardCase) -> bool:
    """binary_masks: every routed bag's non-zero weights are equal (0/1 masks; mean pooling)."""
    for r in range(case.world):
        for f, w in zip(case.feats, case.weights[r]):
            if f.kind in BAGS and not f.replicated and f.kind != NRX_BAG_MEAN and w is not None and not np.all((w == 0) | (w == 1)):
                return False
    return True


def make_case(seed: int) -> ShardCase:
    rng = np.random.default_rng(seed)
    style = str(rng.choice(["mixed", "tower", "wide", "fm_placed", "fm_mixed", "many", "edge"], p=[0.38, 0.12, 0.12, 0.14, 0.1, 0.08, 0.06]))
    if seed in EDGE_SEEDS:
        style = "edge"
    world = int(rng.choice([1, 2, 3], p=[0.5, 0.25, 0.25]))
    if style == "edge":
        world = int(rng.choice([2, 3]))
    tshapes, feats = _draw_features(rng, style, world)
    # ---- batch: drawn from the edge list, then the largest listed size within the lookup caps
    per_sample = sum(max(1, f.bag_len) for f in feats if f.kind != NRX_DENSE)
    per_sample_el = sum(max(1, f.bag_len) * f.dim for f in feats if f.kind != NRX_DENSE)
    B = int(rng.choice(BATCHES))
    if style == "edge":
        B = int(rng.choice([2000, 4096, 9000]))
    fitting = [b for b in BATCHES if world * b * per_sample <= MAX_LOOKUPS and world * b * per_sample_el <= MAX_GATHERED]
    if style != "edge" and B not in fitting:
        B = max(fitting) if fitting else 1
    # ---- tables (row 0 zero: what make_arena leaves)
    tables = {}
    for t, (rows, dim) in sorted(tshapes.items()):
        x = rng.standard_normal((rows, dim)).astype(np.float32)
        x[0] = 0
        tables[t] = x
    # ---- ids: one dtype per embedding width (exchange groups, and the direct path's backward groups)
    dts = {d: (np.int32 if rng.random() < 0.4 else np.int64) for d in sorted({f.dim for f in feats})}
    zipf = {f.name: style != "edge" and rng.random() < 0.35 for f in feats}
    wmode = {f.name: float(rng.random()) for f in feats}
    inputs, weights = [], []
    for r in range(world):
        ins, ws = [], []
        for f in feats:
            if f.kind == NRX_DENSE:
                ins.append(rng.standard_normal(B).astype(np.float32))
                ws.append(None)
                continue
            rows = tables[f.table].shape[0]
            if f.kind == NRX_SPARSE:
                ins.append(_ids(rng, rows, (B,), zipf[f.name]).astype(dts[f.dim]))
                ws.append(None)
            else:
                x, w = _bag(rng, f.kind, rows, B, f.bag_len, zipf[f.name], wmode[f.name])
                ins.append(x.astype(dts[f.dim]))
                ws.append(w)
        inputs.append(ins)
        weights.append(ws)
    case = ShardCase(seed, style, world, B, feats, tables, inputs, weights, [], [], [], None, 0.0, style == "many")
    groups, pooled, plan = case.plan()
    # ---- the edge seeds: rank 0's feature 0 sends exactly capf (+ 1) ids to owner 0 (every other block stays below capf)
    if style == "edge":
        case.slack = float(rng.choice([0.05, 0.2]))
        capf = capf_of(B, world, case.slack)
        case.edge = "capf+1" if seed == EDGE_SEEDS[-1] else "capf"
        k = capf + (1 if case.edge == "capf+1" else 0)
        rows = tables[feats[0].table].shape[0]
        dt = inputs[0][0].dtype
        own0 = rng.integers(0, rows // world, B) * world                     # owned by rank 0 (the padding id included)
        other = rng.integers(0, rows // world, B) * world + rng.integers(1, world, B)
        other = np.where(other < rows, other, 1)
        sel = rng.permutation(B) < k
        inputs[0][0] = np.where(sel, own0, other).astype(dt)
        inputs[0][0][np.flatnonzero(~sel)[:1]] = rows - 1 if (rows - 1) % world else 1
    # ---- out_ld: the plan's width, or padded to a width that is / is not a multiple of 4
    r = rng.random()
    if r < 0.3 and style != "fm_placed":
        case.out_ld = plan.out_width + int(rng.integers(1, 8))
    elif r < 0.5:
        case.out_ld = (plan.out_width + 4) // 4 * 4
    ld = case.ld
    # ---- upstream gradients
    for _ in range(world):
        case.g_out.append(rng.standard_normal((B, ld)).astype(np.float32))
        case.g_wide.append(rng.standard_normal((B, plan.wide_width)).astype(np.float32) if plan.wide_width else None)
        case.g_fm.append(rng.standard_normal(B).astype(np.float32) if plan.use_fm else None)
    # ---- slack: the smallest listed under which no block overflows (edge seeds: drawn above)
    case.block_max = _block_max(case, groups, pooled)
    if style != "edge":
        for s in SLACKS + (float(world - 1),):
            if all(m <= c for m, c in zip(case.block_max, _caps(case, groups, pooled, s))):
                case.slack = s
                break
    case.caps = _caps(case, groups, pooled, case.slack)
    case.knobs = _draw_knobs(rng, case)
    case.forms = _draw_forms(rng, case)
    case.paths = expected_paths(case)
    return case


@functools.lru_cache(maxsize=None)
def case(seed: int) -> ShardCase:
    """make_case(seed), drawn once per process (the tests' parametrisations and workers share it; nothing mutates a case)."""
    return make_case(seed)


# named regression seeds: the bug each one found (the fix lives in the product code; the seeds stay in SEEDS)
REGRESSIONS = {
    # nrx_pool_inbox_fwd(_runs): lanes whose columns lay past D (17, 33, ...) left the column loop and fed stale {row, weight} words to the
    # lane group's __shfl -- wrong pooled columns for bags longer than the active lanes' share of entries
    "pooled_width_past_the_lane_group": (2, 18, 38),
}
EDGE_SEEDS = (46, 47)          # (edge seeds besides those drawn) the last one fills its block to capf + 1


def _draw_knobs(rng, case: ShardCase) -> Dict[str, object]:
    return E._draw_knobs(rng, SimpleNamespace(seed=case.seed, lookups=lambda: case.B * case.world))


def _draw_forms(rng, case: ShardCase) -> List[dict]:
    """The forms a case runs: the drawn one, and (when the drawn one is not) the buffered form (one_sided=False, direct_grad=False)."""
    W = case.world
    p = 0.6 if W == 1 else 0.2
    form = dict(one_sided=bool(rng.random() < p), direct_grad=bool(rng.random() < p),
                binary_masks=bool(_binary_ok(case) and rng.random() < 0.6),
                route_bags=ROUTE_BAGS[case.seed % 3], overlap=OVERLAP[(case.seed // 3) % 4], plan=PLAN_MODES[(case.seed // 2) % 3],
                check_index=bool(case.seed % 2))
    if case.style == "fm_placed" and W == 1:
        form["one_sided"] = True          # (the FM pass over the finished concat)
    if case.overflow:                     # (dropped lookups: the forward and the overflow report only, in the buffered form)
        form.update(one_sided=False, direct_grad=False)
    forms = [form]
    if form["one_sided"] or form["direct_grad"]:
        forms.append(dict(form, one_sided=False, direct_grad=False))
    for f in forms:
        f["paths"] = form_paths(case, f)
    return forms


# ------------------------------------------------------------------------------------------------- paths
def form_paths(case: ShardCase, form: dict) -> List[str]:
    """The step's code paths for this form (the rules of shard_step.py and sharding.py, restated)."""
    groups, pooled, plan = case.plan()
    feats, W, k = case.feats, case.world, case.knobs
    ld = case.ld
    p = []
    if len(feats) > NRX_MAX_FEATURES:
        p.append("fwd_split")
    fm_ok = plan.use_fm and all(f.fm and f.kind == NRX_SPARSE and not f.replicated for f in feats) and len({f.dim for f in feats}) == 1 \
        and len(feats) <= NRX_MAX_FEATURES
    placed = set()
    if form["one_sided"] and (not plan.use_fm or fm_ok) and ld % 4 == 0 and plan.wide_width == 0:
        for gi, idxs in enumerate(groups):
            if gi not in pooled and feats[idxs[0]].dim in PLACE_WIDTHS and all(plan.slots[i].out_col % 4 == 0 for i in idxs):
                placed.add(gi)
        if plan.use_fm and len(placed) != len(groups):
            placed = set()
    if placed:
        p.append("placed")
        if plan.use_fm:
            p.append("fm_pass")
    if any(f.kind != NRX_DENSE and not f.replicated and case.tables[f.table].shape[0] < W for f in feats):
        p.append("empty_shard")
    for gi, idxs in enumerate(groups):
        if gi in pooled:
            how = form["route_bags"]
            lens = [feats[i].bag_len for i in idxs]
            if how == "runs" and not all(1 <= L <= RF_TILE and (RF_TILE // L) * W <= RF_TILE for L in lens):
                how = "one"
            p.append(f"route_bags:{how}")
    if case.forward_only or case.overflow:      # (an overflowing case runs its forward and the overflow report only)
        return sorted(set(p))
    p.append(f"plan:{form['plan']}")
    single = [gi for gi in range(len(groups)) if gi not in pooled]
    if W == 1 and len(groups) > 1 and form["overlap"] != "0" and len(single) <= 1:
        p.append("forked")
    sums_ld = max([f.dim for f in feats if f.fm] + [0])
    for gi in single:
        idxs = groups[gi]
        n, D = len(idxs), feats[idxs[0]].dim
        Bp = W * case.caps[gi]
        shift = max(1, (2 * n * Bp - 1).bit_length())
        aligned = ld % 4 == 0 and all(plan.slots[i].out_col % 4 == 0 for i in idxs)
        if form["direct_grad"] and D in DIRECT_WIDTHS and aligned and shift <= 30 and W <= (1 << (31 - shift)) and k["SPARSE_PLACE"]:
            p.append("direct_grad")
            continue
        # nrx_embed_bwd_scatter's placement pass: D = 16 / 32 / 64; with the FM term folded in, aligned columns and FM buffers too
        fast = D in DIRECT_WIDTHS and (not plan.use_fm or (aligned and sums_ld % 4 == 0 and sums_ld >= D))
        p.append("bwd_scatter" if fast else "bwd_fallback")
    if any(gi in pooled for gi in range(len(groups))):
        p.append("pooled_binary" if form["binary_masks"] else "pooled_expand")
    if any(f.replicated and f.kind != NRX_DENSE for f in feats):
        p.append("replicated_w1" if W == 1 else "replicated_fold")
    return sorted(set(p))


def expected_paths(case: ShardCase) -> List[str]:
    return sorted({q for f in case.forms for q in f["paths"]})


# ------------------------------------------------------------------------------------------------- float64 truth
def truth_case(case: ShardCase) -> E.Case:
    """The whole step as one embed_cases.Case: the step's final-plan columns, the rank-major concatenation of the ranks' batches."""
    _, _, plan = case.plan()
    names = case.table_names
    slots = []
    for f, s in zip(case.feats, plan.slots):
        t = -1 if f.kind == NRX_DENSE else names.index(f.table)
        slots.append(E.SlotSpec(f.name, f.kind, t, f.dim, f.bag_len, s.out_col, s.wide_col, int(f.fm)))
    W = case.world
    inputs = [np.concatenate([case.inputs[r][i] for r in range(W)]) for i in range(len(case.feats))]
    weights = [None if case.weights[0][i] is None else np.concatenate([case.weights[r][i] for r in range(W)]) for i in range(len(case.feats))]
    g_wide = np.concatenate(case.g_wide) if plan.wide_width else None
    g_fm = np.concatenate(case.g_fm) if plan.use_fm else None
    return E.Case(case.seed, case.style, W * case.B, slots, plan.out_width, case.ld, False, plan.wide_width, plan.use_fm, False,
                  [case.tables[t] for t in names], inputs, weights, np.concatenate(case.g_out), g_wide, g_fm)


def chains(case: ShardCase, ref: "E.Restated"):
    """(n_out, n_fm, n_grads): restate's rounding chains lengthened for the sharded order."""
    W = case.world
    names = case.table_names
    pooled_feat = [f.kind in BAGS and not f.replicated for f in case.feats]
    n_out = ref.n_out + (W if any(pooled_feat) else 0)
    n_grads = list(ref.n_grads)
    for t, name in enumerate(names):
        fed = [f for f, pf in zip(case.feats, pooled_feat) if f.table == name and (pf or f.replicated)]
        if fed:
            n_grads[t] += W
    return n_out, ref.n_fm, n_grads


def restate(case: ShardCase, device: str = "cpu", grads: bool = True):
    return E.restate(truth_case(case), device, grads=grads)


# ------------------------------------------------------------------------------------------------- coverage
def coverage(seeds=SEEDS) -> Dict[str, List[int]]:
    """Which seeds show each generator feature and each predicted path (the CPU tests require every one of them)."""
    cov: Dict[str, List[int]] = {}

    def mark(k, sd):
        cov.setdefault(k, [])
        if sd not in cov[k]:
            cov[k].append(sd)

    for sd in seeds:
        c = make_case(sd)
        groups, pooled, plan = c.plan()
        mark(f"style:{c.style}", sd)
        mark(f"world:{c.world}", sd)
        mark(f"batch:{'<64' if c.B < 64 else '64' if c.B == 64 else '<=4096' if c.B <= 4096 else '>4096'}", sd)
        mark("slack:overflow_free" if not c.edge else f"edge:{c.edge}", sd)
        for f in c.feats:
            mark(f"kind:{KIND_NAMES[f.kind]}{':replicated' if f.replicated else ''}", sd)
            if f.kind != NRX_DENSE:
                mark(f"width:{f.dim}", sd)
            if f.wide:
                mark("wide", sd)
            if f.fm:
                mark("fm_field:replicated" if f.replicated else "fm_field:routed", sd)
        for gi, idxs in enumerate(groups):
            if gi not in pooled and len({c.feats[i].table for i in idxs}) < len(idxs):
                mark("table_shared", sd)
            if gi in pooled and any(c.feats[i].kind == NRX_SPARSE and c.feats[i].table == c.feats[idxs[0]].table for i in range(len(c.feats))):
                mark("table_shared_by_id_and_bag", sd)
        for r in range(c.world):
            for f, x, w in zip(c.feats, c.inputs[r], c.weights[r]):
                if f.kind == NRX_DENSE:
                    continue
                mark(f"ids:{x.dtype}", sd)
                if f.bag_len:
                    mark(f"bag_len:{f.bag_len}", sd)
                    if w is not None and (w.sum(1) == 0).any():
                        mark("bag:empty", sd)
                    if w is not None and not np.all((w == 0) | (w == 1)):
                        mark("bag:float_weights", sd)
                    elif w is not None:
                        mark("bag:binary_mask", sd)
        if any(t.shape[0] < c.world for n, t in c.tables.items() if any(f.table == n and not f.replicated for f in c.feats)):
            mark("empty_shard", sd)
        if any(f.kind != NRX_DENSE and f.fm for f in c.feats):
            mark("fm:placeable" if "fm_pass" in c.paths else "fm:on", sd)
        if c.out_ld:
            mark("out_ld:padded_x4" if c.out_ld % 4 == 0 else "out_ld:padded_odd", sd)
        if c.forward_only:
            mark("forward_only", sd)
        for p in c.paths:
            mark(f"path:{p}", sd)
        for f in c.forms:
            mark(f"form:{'one_sided' if f['one_sided'] else 'all_to_all'}/{'direct' if f['direct_grad'] else 'buffered'}", sd)
            if f["binary_masks"]:
                mark("form:binary_masks", sd)
            mark(f"overlap:{f['overlap']}", sd)
        for kk, v in c.knobs.items():
            if v != E.KNOB_DEFAULTS[kk]:
                mark(f"knob:{kk}={v if not isinstance(v, int) or isinstance(v, bool) else 'lowered'}", sd)
    return cov


if __name__ == "__main__":
    for a in sys.argv[1:] or ["0"]:
        print(make_case(int(a)).spec())
