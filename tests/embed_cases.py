"""Generated embedding launches and their float64 restatement (a helper of the tests, not a conftest).

make_case(seed) draws one launch of ops.embed_apply from numpy's default_rng(seed): feature kinds (single ids, dense values, masked-mean /
mean / sum bags, padded or CSR), shared tables, uniform or Zipf ids of both widths, widths from 1 to 300, the FM epilogue, wide columns, a
padded output stride, up to 70 features and batch sizes on both sides of the kernels' block and dispatch edges.  It also names the ops.*
knobs (planner, padding split, placement, size thresholds) the GPU tests set for the seed, and the dispatch paths the seed should take.

restate(case) is the same launch in float64 under torch autograd, written from the reference's definitions (oracle/ref_np.py: gather,
array_pool, the FM logit of fm/model.py, the wide split, csr_bag_to_padded).  It returns the concat, wide, fm and table gradients (padding
row zeroed) together with an error scale A: the same computation with every table, weight and upstream gradient replaced by its absolute
value and the FM's difference of squares by their sum.  A float32 evaluation of n terms, summed in any order, then satisfies

    |got - ref| <= C * n * 2**-24 * A        (element-wise: `bound`, `excess`)

where n counts the longest chain of roundings behind the element: for a table gradient the lookups of the table's hottest row, plus the
longest bag (its mask sum divides every term), plus the FM fields for an FM table.

    python -m tests.embed_cases SEED      prints the case
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from news_recsys_amd._lib import (NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM, NRX_DENSE, NRX_FEAT_BAG_CSR, NRX_FEAT_TABLE_BF16,
                                  NRX_MAX_FEATURES, NRX_SPARSE)

KIND_NAMES = {NRX_SPARSE: "sparse", NRX_DENSE: "dense", NRX_BAG_MASKED_MEAN: "masked_mean", NRX_BAG_MEAN: "mean", NRX_BAG_SUM: "sum"}
WIDTHS = (1, 2, 4, 5, 8, 12, 16, 17, 32, 33, 64, 128, 256, 300)
FM_WIDTHS = (2, 4, 5, 8, 12, 16, 17, 32, 33, 64, 128, 256)          # the fused FM epilogue takes dims <= 256; w + at least one v column
BATCHES = (1, 63, 64, 65, 257, 2048, 2049, 4096, 4097, 9000, 30000)
BAG_LENS = (1, 2, 5, 17, 50)
ROWS = (2, 3, 50, 1000, 30000, 300000)
MAX_LOOKUPS = 250_000                 # per case: a case's ~15 launches and its float64 restatement stay well under a second
MAX_GATHERED = 1 << 22                # lookups x dim per case (the float64 restatement's gathered rows)
MAX_TABLE_ELEMS = 1 << 21             # rows x dim per table
EPS32 = 2.0 ** -24
C_BOUND = 2.0                         # the constant of the error bound
SEEDS = tuple(range(60))              # the seeds the tests run

# defaults of the ops.* knobs a case may change (the GPU tests set every one of them per seed)
KNOB_DEFAULTS = dict(PLAN_LDS="auto", PAD_SPLIT="auto", SPARSE_PLACE=True, DENSE_SORTED_MIN=3 << 18, DENSE_LDS_MIN=1 << 16,
                     PLAN_AHEAD_MIN=1 << 20, PAD_SPLIT_MIN=3 << 19)


@dataclass
class SlotSpec:
    """One feature (the fields of ops.Slot)."""
    name: str
    kind: int
    table: int
    dim: int
    bag_len: int = 0
    out_col: int = 0
    wide_col: int = -1
    fm_field: int = 0
    flags: int = 0


@dataclass
class Case:
    seed: int
    style: str
    B: int
    slots: List[SlotSpec]
    out_width: int
    out_ld: int
    narrow: bool
    wide_width: int
    use_fm: bool
    bf16: bool
    tables: List[np.ndarray]                 # float32 [rows, dim] (bf16 cases: values a bf16 holds exactly)
    inputs: List[np.ndarray]                 # ids int32 / int64 [B] | [B, L] | CSR [nnz]; dense values float32 [B]
    weights: List[Optional[np.ndarray]]      # None | float32 mask / weights [B, L] | CSR int64 offsets [B + 1]
    g_out: np.ndarray                        # float32 [B, out_ld] (the stride padding holds values no backward may read)
    g_wide: Optional[np.ndarray]             # float32 [B, wide_width]
    g_fm: Optional[np.ndarray]               # float32 [B]
    knobs: Dict[str, object] = field(default_factory=dict)
    paths: List[str] = field(default_factory=list)

    @property
    def n_feats(self) -> int:
        return len(self.slots)

    def lookups(self) -> int:
        return sum(self.B * max(1, s.bag_len) for s in self.slots if s.kind != NRX_DENSE)

    def spec(self) -> str:
        head = (f"seed {self.seed} ({self.style}): B={self.B}  features={self.n_feats}  tables={len(self.tables)}  out_width={self.out_width} "
                f"out_ld={self.out_ld}{' narrow' if self.narrow else ''}  wide_width={self.wide_width}  fm={self.use_fm}  bf16={self.bf16}  "
                f"lookups={self.lookups()}")
        lines = [head, f"  knobs: {self.knobs}", f"  paths: {self.paths}"]
        for t, tab in enumerate(self.tables):
            lines.append(f"  table {t}: rows={tab.shape[0]} dim={tab.shape[1]}")
        for s, x, w in zip(self.slots, self.inputs, self.weights):
            csr = bool(s.flags & NRX_FEAT_BAG_CSR)
            wdesc = "-" if w is None else ("offsets" if csr else ("binary mask" if np.all((w == 0) | (w == 1)) else "weights"))
            lines.append(f"  {s.name}: {KIND_NAMES[s.kind]}{' csr' if csr else ''} table={s.table} dim={s.dim} L={s.bag_len} "
                         f"out_col={s.out_col} wide_col={s.wide_col} fm={s.fm_field} ids={x.dtype}{list(x.shape)} w={wdesc}")
        return "\n".join(lines)

    def plan(self):
        from news_recsys_amd import ops
        return ops.EmbedPlan([ops.Slot(s.name, s.kind, s.table, s.dim, s.bag_len, s.out_col, s.wide_col, s.fm_field, s.flags)
                              for s in self.slots], out_width=self.out_width, wide_width=self.wide_width, use_fm=self.use_fm)


# ------------------------------------------------------------------------------------------------- generator
def _bf16_exact(a: np.ndarray) -> np.ndarray:
    """Round float32 values to the nearest bf16 (ties to even), kept as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _ids(rng, rows: int, shape, zipf: bool) -> np.ndarray:
    if zipf:
        x = np.minimum(rng.zipf(float(rng.choice([1.1, 1.3, 1.6])), shape) - 1, rows - 1)
    else:
        x = rng.integers(0, rows, shape)
    x = np.asarray(x, np.int64).reshape(shape)
    flat = x.reshape(-1)
    if flat.size >= 4:                        # the last row, the padding id and duplicates in every feature
        k = rng.integers(0, flat.size, 4)
        flat[k[0]] = rows - 1
        flat[k[1]] = 0
        flat[k[2]] = flat[k[3]]
    return x


def _table_rows(rng, dim: int, small: bool = False) -> int:
    cap = max(2, MAX_TABLE_ELEMS // dim)
    r = int(rng.choice(ROWS[:4] if small else ROWS))
    return max(2, min(r, cap))


def _draw_kind(rng, bags: bool = True) -> int:
    if not bags:
        return NRX_SPARSE
    return int(rng.choice([NRX_SPARSE, NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM], p=[0.45, 0.2, 0.15, 0.2]))


def make_case(seed: int) -> Case:
    rng = np.random.default_rng(seed)
    style = str(rng.choice(["mixed", "fm_wide", "many_fm", "many_shared", "bf16"], p=[0.5, 0.16, 0.1, 0.1, 0.14]))
    use_fm = False
    fm_dim = 0
    # ---- tables
    if style in ("many_fm", "many_shared"):
        n_feat = int(rng.integers(NRX_MAX_FEATURES + 1, 71))
        dim = int(rng.choice([2, 4, 8, 16] if style == "many_fm" else [8, 16, 32]))
        n_tab = int(rng.integers(1, 4))
        dims = [dim] * n_tab
        use_fm = style == "many_fm"
        fm_dim = dim if use_fm else 0
    else:
        n_feat = int(rng.choice([1, 2, 3, 5, 8, 12, 20, 40], p=[0.12, 0.12, 0.15, 0.17, 0.17, 0.12, 0.1, 0.05]))
        n_tab = int(rng.integers(1, min(n_feat, 6) + 1))
        dims = [int(rng.choice(WIDTHS)) for _ in range(n_tab)]
        if style == "fm_wide" or (style != "bf16" and rng.random() < 0.15):
            use_fm = True
            fm_dim = int(rng.choice(FM_WIDTHS))
            dims[0] = fm_dim
    small_rows = style in ("many_fm", "many_shared")
    rows = [_table_rows(rng, d, small_rows) for d in dims]
    # ---- features
    slots: List[SlotSpec] = []
    for f in range(n_feat):
        if style in ("many_fm", "many_shared"):
            t = 0 if (style == "many_shared" and rng.random() < 0.8) else int(rng.integers(0, n_tab))
            kind = _draw_kind(rng, bags=rng.random() < 0.3)
        elif style != "bf16" and rng.random() < 0.08:
            slots.append(SlotSpec(f"f{f:02d}", NRX_DENSE, -1, 1))
            continue
        else:
            t = int(rng.integers(0, n_tab))
            kind = _draw_kind(rng)
        L = 0 if kind == NRX_SPARSE else int(rng.choice(BAG_LENS))
        flags = NRX_FEAT_BAG_CSR if (L and rng.random() < 0.3) else 0
        slots.append(SlotSpec(f"f{f:02d}", kind, t, dims[t], L, flags=flags))
    if not any(s.kind != NRX_DENSE for s in slots):
        slots[0] = SlotSpec("f00", NRX_SPARSE, 0, dims[0])
    if use_fm:
        cands = [i for i, s in enumerate(slots) if s.kind != NRX_DENSE and s.dim == fm_dim]
        if not cands:
            slots[0] = SlotSpec("f00", NRX_SPARSE, 0, fm_dim)
            cands = [0]
        if style == "many_fm":
            chosen = cands
        else:
            chosen = [i for i in cands if rng.random() < 0.7] or cands[:1]
        for i in chosen:
            slots[i].fm_field = 1
    # wide columns (never on an FM field: the kernels refuse that)
    wide_width = 0
    if style == "fm_wide" or (style in ("mixed", "bf16") and rng.random() < 0.25):
        for s in slots:
            if not s.fm_field and s.kind != NRX_DENSE and s.dim >= 2 and rng.random() < 0.5:
                s.wide_col = wide_width
                wide_width += 1
    # ---- columns: the features laid out in a permuted order (slot order != column order, odd columns everywhere)
    if style == "many_fm":
        order = list(range(n_feat))          # the FM over more than 64 fields reads the concat as [B, F, D] from column 0
    else:
        order = [int(i) for i in rng.permutation(n_feat)]
    col = 0
    for i in order:
        s = slots[i]
        s.out_col = col
        col += s.dim - (1 if s.wide_col >= 0 else 0)
    out_width = col
    out_ld = out_width + (int(rng.integers(1, 8)) if rng.random() < 0.3 else 0)
    narrow = bool(out_ld > out_width and not use_fm and rng.random() < 0.5)
    # ---- batch: drawn from the edge list, then the largest listed size within the lookup cap
    per_sample = sum(max(1, s.bag_len) for s in slots if s.kind != NRX_DENSE)
    per_sample_el = sum(max(1, s.bag_len) * s.dim for s in slots if s.kind != NRX_DENSE)
    B = int(rng.choice(BATCHES))
    fitting = [b for b in BATCHES if b * per_sample <= MAX_LOOKUPS and b * per_sample_el <= MAX_GATHERED]
    if B not in fitting:
        B = max(fitting) if fitting else 1
    # ---- tables' values
    tables = []
    for r, d in zip(rows, dims):
        t = rng.standard_normal((r, d)).astype(np.float32)
        if style == "bf16":
            t = _bf16_exact(t)
        tables.append(t)
    # ---- inputs
    inputs, weights = [], []
    case_dt = None if rng.random() < 0.5 else (np.int32 if rng.random() < 0.4 else np.int64)      # None: the widths mixed per feature
    for s in slots:
        if s.kind == NRX_DENSE:
            inputs.append(rng.standard_normal(B).astype(np.float32))
            weights.append(None)
            continue
        r = rows[s.table]
        zipf = rng.random() < 0.35
        dt = case_dt or (np.int32 if rng.random() < 0.4 else np.int64)
        L = s.bag_len
        if s.flags & NRX_FEAT_BAG_CSR:
            lens = rng.integers(0, L + L // 2 + 2, B)            # empty bags and bags longer than L (cut to their first L)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            vals = _ids(rng, r, (int(off[-1]),), zipf) if off[-1] else np.zeros(0, np.int64)
            inputs.append(vals.astype(dt))
            weights.append(off)
            continue
        if L == 0:
            inputs.append(_ids(rng, r, (B,), zipf).astype(dt))
            weights.append(None)
            continue
        x = _ids(rng, r, (B, L), zipf)
        n_valid = rng.integers(0, L + 1, (B, 1))                 # empty bags included
        valid = np.arange(L)[None, :] < n_valid
        w = None
        if s.kind == NRX_BAG_MASKED_MEAN:
            x = x * valid                                        # padded histories: id 0 behind the valid entries
            if rng.random() < 0.5:
                w = valid.astype(np.float32)
            else:                                                # non-binary masks: weights in [0.25, 1] (a mask sum far above 1e-8)
                w = (valid * rng.uniform(0.25, 1.0, (B, L))).astype(np.float32)
        elif s.kind == NRX_BAG_SUM and rng.random() < 0.6:
            x = x * valid
            w = (valid * rng.uniform(-1.0, 1.0, (B, L))).astype(np.float32)
        elif s.kind == NRX_BAG_MEAN and rng.random() < 0.5:
            x = x * valid                                        # mean over L, padding included (row 0 is read)
        inputs.append(x.astype(dt))
        weights.append(w)
    # ---- upstream gradients
    g_out = rng.standard_normal((B, out_ld)).astype(np.float32)
    g_wide = rng.standard_normal((B, wide_width)).astype(np.float32) if wide_width else None
    g_fm = rng.standard_normal(B).astype(np.float32) if use_fm else None
    if style == "bf16":
        for s in slots:
            if s.kind != NRX_DENSE:
                s.flags |= NRX_FEAT_TABLE_BF16
    case = Case(seed, style, B, slots, out_width, out_ld, narrow, wide_width, use_fm, style == "bf16", tables, inputs, weights,
                g_out, g_wide, g_fm)
    case.knobs = _draw_knobs(rng, case)
    case.paths = expected_paths(case)
    return case


def _draw_knobs(rng, case: Case) -> Dict[str, object]:
    """The ops.* knobs of the seed: the planner, the padding split and the placement in rotation, and (some seeds) the size thresholds
    lowered under the launch's lookup count so that a small case takes the paths a large launch takes."""
    k = dict(KNOB_DEFAULTS)
    k["PLAN_LDS"] = ("auto", "0", "1")[case.seed % 3]
    k["PAD_SPLIT"] = ("auto", "1", "0")[(case.seed // 3) % 3]
    k["SPARSE_PLACE"] = case.seed % 5 != 4
    n = case.lookups()
    r = rng.random()
    if r < 0.3:                       # the planned dense reduction from this launch's size on, planned ahead on the side stream
        k["DENSE_SORTED_MIN"] = max(1, n // 2)
        k["PLAN_AHEAD_MIN"] = max(1, n // 4)
    elif r < 0.45:                    # the one-kernel planner's dense form
        k["DENSE_LDS_MIN"] = max(1, n // 2)
    if rng.random() < 0.4:
        k["PAD_SPLIT_MIN"] = max(1, n // 4)
    return k


def _table_lookups(case: Case) -> Dict[int, int]:
    per: Dict[int, int] = {}
    for s in case.slots:
        if s.kind != NRX_DENSE:
            per[s.table] = per.get(s.table, 0) + case.B * max(1, s.bag_len)
    return per


def expected_paths(case: Case) -> List[str]:
    """Dispatch paths this seed takes for certain (a subset: where the rule is simple).  The coverage test runs a seed of each and
    checks the path was taken -- a threshold that moves must not quietly stop testing a path."""
    MF = NRX_MAX_FEATURES
    k = case.knobs
    p = []
    n = case.lookups()
    csr = any(s.flags & NRX_FEAT_BAG_CSR for s in case.slots)
    if case.n_feats > MF:
        p.append("fwd_split")
    if case.use_fm and case.n_feats > MF:
        p.append("fm_bwd_concat")
    if csr:
        p.append("csr_sink")
    if case.n_feats > MF:
        dims = {}
        for s in case.slots:
            if s.kind != NRX_DENSE:
                dims.setdefault(s.dim, []).append(s.table)
        if any(len(ts) > MF and set(ts[:MF]) & set(ts[MF:]) for ts in dims.values()):
            p.append("adam_two_groups")
    if case.bf16 or n == 0 or len(case.tables) > MF:
        return p
    # dense gradients in auto mode
    if n >= k["DENSE_SORTED_MIN"]:
        p.append("dense_sorted")
        return p
    lds_possible = (k["PLAN_LDS"] != "0" and k["SPARSE_PLACE"] and n >= max(k["DENSE_LDS_MIN"], 1)
                    and all(s.kind in (NRX_SPARSE, NRX_DENSE) for s in case.slots))
    if lds_possible:
        return p
    per = _table_lookups(case)
    one_width = len({x.dtype for s, x in zip(case.slots, case.inputs) if s.kind != NRX_DENSE}) == 1
    if (case.B <= 4096 and case.n_feats <= MF and not csr and max(per.values()) <= 4096 and one_width
            and all(s.dim <= 256 for s in case.slots)):
        p.append("dense_small")
    elif case.B > 4096:
        p.append("dense_atomic")
    return p


# ------------------------------------------------------------------------------------------------- float64 restatement
def csr_to_padded(values: np.ndarray, offsets: np.ndarray, L: int):
    from oracle import ref_np as R
    return R.csr_bag_to_padded(values, offsets, L)


@dataclass
class Restated:
    out: "object"           # torch float64 [B, out_width]
    wide: "object"          # [B, wide_width] | None
    fm: "object"            # [B] | None
    grads: list             # per table [rows, dim] (row 0 zero)
    A_out: "object"
    A_wide: "object"
    A_fm: "object"
    A_grads: list
    n_out: int              # rounding-chain lengths of the bound (see the module's docstring)
    n_fm: int
    n_grads: List[int]
    copy_cols: List[int]    # concat columns that are plain copies (single ids, dense values): bit-exact
    wide_copy_cols: List[int]  # wide columns of single-valued features: bit-exact


def _forward64(case: Case, tabs, absmode: bool, dev):
    import torch
    B = case.B
    out = torch.zeros((B, case.out_width), dtype=torch.float64, device=dev)
    wide = torch.zeros((B, case.wide_width), dtype=torch.float64, device=dev) if case.wide_width else None
    parts_out, parts_wide = [], []
    fm_vecs = []
    for s, x, w in zip(case.slots, case.inputs, case.weights):
        if s.kind == NRX_DENSE:
            e = torch.from_numpy(x.astype(np.float64)).to(dev)[:, None]        # base_model.py:264-265
            if absmode:
                e = e.abs()
        else:
            t = tabs[s.table]
            if s.flags & NRX_FEAT_BAG_CSR:
                ids, mask = csr_to_padded(x, w, s.bag_len)
                wt = None if s.kind == NRX_BAG_MEAN else mask            # every entry counts with weight 1 (nrx_embed.h)
            else:
                ids, wt = x, w
            ids_t = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
            e = t[ids_t]
            if s.kind != NRX_SPARSE:                                     # array_pool (base_model.py:273-282) and the owner-side sum
                if s.kind == NRX_BAG_MEAN:
                    e = e.mean(1)
                else:
                    m = None if wt is None else torch.from_numpy(wt.astype(np.float64)).to(dev)
                    if m is not None and absmode:
                        m = m.abs()
                    if s.kind == NRX_BAG_SUM:
                        e = e.sum(1) if m is None else (e * m[:, :, None]).sum(1)
                    else:
                        e = (e * m[:, :, None]).sum(1) / (m.sum(1, keepdim=True) + 1e-8)
        if s.wide_col >= 0:                                              # widedeep/model.py:58-66 (oracle wide_split)
            parts_wide.append((s.wide_col, e[:, :1]))
            parts_out.append((s.out_col, e[:, 1:]))
        else:
            parts_out.append((s.out_col, e))
        if s.fm_field:
            fm_vecs.append(e)
    cols_o = torch.cat([p for _, p in parts_out], 1) if parts_out else out
    idx_o = torch.cat([torch.arange(c, c + p.shape[1]) for c, p in parts_out]).to(dev)
    out = out.index_copy(1, idx_o, cols_o)
    if wide is not None and parts_wide:
        idx_w = torch.tensor([c for c, _ in parts_wide], device=dev)
        wide = wide.index_copy(1, idx_w, torch.cat([p for _, p in parts_wide], 1))
    fm = None
    if case.use_fm:                                                      # fm/model.py:18-26 without bias / sigmoid (oracle fm_logit)
        E = torch.stack(fm_vecs, 1)                                      # [B, F, D]
        w_, v_ = E[:, :, 0], E[:, :, 1:]
        sv, sq = v_.sum(1), (v_ * v_).sum(1)
        second = 0.5 * ((sv * sv + sq) if absmode else (sv * sv - sq)).sum(1)
        fm = w_.sum(1) + second
    return out, wide, fm


def restate(case: Case, device: str = "cpu", grads: bool = True) -> Restated:
    import torch
    dev = torch.device(device)
    res = []
    for absmode in (False, True):
        tabs = [torch.from_numpy(np.abs(t) if absmode else t).to(dev, torch.float64).requires_grad_(grads) for t in case.tables]
        out, wide, fm = _forward64(case, tabs, absmode, dev)
        gs = [None] * len(tabs)
        if grads:
            go = case.g_out[:, :case.out_width]
            terms = [(out * torch.from_numpy(np.abs(go) if absmode else go).to(dev, torch.float64)).sum()]
            if wide is not None:
                terms.append((wide * torch.from_numpy(np.abs(case.g_wide) if absmode else case.g_wide).to(dev, torch.float64)).sum())
            if fm is not None:
                terms.append((fm * torch.from_numpy(np.abs(case.g_fm) if absmode else case.g_fm).to(dev, torch.float64)).sum())
            need = [t for t in tabs]
            got = torch.autograd.grad(sum(terms), need, allow_unused=True)
            gs = []
            for g, t in zip(got, tabs):
                g = torch.zeros_like(t) if g is None else g.detach().clone()
                g[0] = 0                                                 # padding_idx = 0: the padding row never trains
                gs.append(g)
        res.append((out.detach(), None if wide is None else wide.detach(), None if fm is None else fm.detach(), gs))
    (out, wide, fm, gs), (A_out, A_wide, A_fm, A_gs) = res
    # rounding chains
    max_L = max([s.bag_len for s in case.slots] + [1])
    n_fm_fields = sum(1 for s in case.slots if s.fm_field)
    fm_dim = max([s.dim for s in case.slots if s.fm_field] + [0])
    n_grads = []
    hot = _hot_rows(case)
    for t in range(len(case.tables)):
        L_t = max([s.bag_len for s in case.slots if s.kind != NRX_DENSE and s.table == t] + [1])
        fm_t = any(s.fm_field and s.table == t for s in case.slots)
        n_grads.append(hot[t] + L_t + (n_fm_fields + fm_dim + max_L if fm_t else 0) + 3)
    copy_cols = []
    for s in case.slots:
        if s.kind in (NRX_SPARSE, NRX_DENSE):
            c0 = s.out_col
            copy_cols.extend(range(c0, c0 + s.dim - (1 if s.wide_col >= 0 else 0)))
    wide_copy = [s.wide_col for s in case.slots if s.kind == NRX_SPARSE and s.wide_col >= 0]
    return Restated(out, wide, fm, gs, A_out, A_wide, A_fm, A_gs, max_L + 3, n_fm_fields + fm_dim + max_L + 3, n_grads, copy_cols, wide_copy)


def _hot_rows(case: Case) -> List[int]:
    """Per table: the lookups of its hottest row other than the padding row (CSR bags: of the entries within the first L)."""
    counts = [np.zeros(t.shape[0], np.int64) for t in case.tables]
    for s, x, w in zip(case.slots, case.inputs, case.weights):
        if s.kind == NRX_DENSE:
            continue
        ids = csr_to_padded(x, w, s.bag_len)[0] if s.flags & NRX_FEAT_BAG_CSR else x
        counts[s.table] += np.bincount(np.asarray(ids, np.int64).reshape(-1), minlength=case.tables[s.table].shape[0])
    return [int(c[1:].max()) if c.size > 1 else 0 for c in counts]


def bound(A, n: int):
    """The element-wise error allowance of a float32 result with rounding chains of length n against the float64 reference."""
    return C_BOUND * n * EPS32 * A


def excess(got, ref, A, n: int):
    """max(|got - ref| - bound) over the elements (<= 0: within the bound), and the flat index of the worst element."""
    import torch
    d = (got.to(torch.float64) - ref).abs() - bound(A, n)
    if d.numel() == 0:
        return 0.0, -1
    i = int(torch.argmax(d))
    return float(d.reshape(-1)[i]), i


def coverage(seeds=SEEDS) -> Dict[str, List[int]]:
    """Which seeds show each generator feature (the CPU tests require every one of them)."""
    cov: Dict[str, List[int]] = {}

    def mark(k, sd):
        cov.setdefault(k, [])
        if sd not in cov[k]:
            cov[k].append(sd)

    for sd in seeds:
        c = make_case(sd)
        mark(f"style:{c.style}", sd)
        mark(f"batch:{c.B}", sd)
        kinds_by_table: Dict[int, set] = {}
        for s, x, w in zip(c.slots, c.inputs, c.weights):
            mark(f"kind:{KIND_NAMES[s.kind]}", sd)
            if s.kind != NRX_DENSE:
                kinds_by_table.setdefault(s.table, set()).add(s.kind)
                mark(f"ids:{x.dtype}", sd)
                mark(f"width:{s.dim}", sd)
                if s.flags & NRX_FEAT_BAG_CSR:
                    mark("csr", sd)
                    lens = np.diff(w)
                    if (lens == 0).any():
                        mark("csr:empty_bag", sd)
                    if (lens > s.bag_len).any():
                        mark("csr:longer_than_L", sd)
                elif s.bag_len:
                    mark("padded_bag", sd)
                    if w is not None and (w.sum(1) == 0).any():
                        mark("padded:empty_bag", sd)
                if s.kind == NRX_BAG_MASKED_MEAN and w is not None and not (s.flags & NRX_FEAT_BAG_CSR) and not np.all((w == 0) | (w == 1)):
                    mark("masked_mean:non_binary", sd)
                if s.kind == NRX_BAG_SUM and not (s.flags & NRX_FEAT_BAG_CSR):
                    mark("sum:weighted" if w is not None else "sum:unweighted", sd)
            if s.out_col % 4:
                mark("col_not_multiple_of_4", sd)
            if s.wide_col >= 0:
                mark("wide", sd)
        if any(len(k) > 1 and NRX_SPARSE in k and (k - {NRX_SPARSE}) for k in kinds_by_table.values()):
            mark("table_shared_by_id_and_bag", sd)
        if len({x.dtype for s, x in zip(c.slots, c.inputs) if s.kind != NRX_DENSE}) > 1:
            mark("ids:mixed_in_launch", sd)
        for t in c.tables:
            if t.shape[0] == 2:
                mark("rows:2", sd)
            if t.shape[0] >= 100_000:
                mark("rows:100k+", sd)
        mark("fm:on" if c.use_fm else "fm:off", sd)
        if c.out_ld > c.out_width:
            mark("out_ld:narrow" if c.narrow else "out_ld:wide", sd)
        mark("feats:>64" if c.n_feats > NRX_MAX_FEATURES else "feats:<=64", sd)
        if c.bf16:
            mark("bf16", sd)
        for p in c.paths:
            mark(f"path:{p}", sd)
        for kk, v in c.knobs.items():
            if v != KNOB_DEFAULTS[kk]:
                mark(f"knob:{kk}={v if not isinstance(v, int) or isinstance(v, bool) else 'lowered'}", sd)
    return cov


if __name__ == "__main__":
    for a in sys.argv[1:] or ["0"]:
        print(make_case(int(a)).spec())
