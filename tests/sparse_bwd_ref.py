"""What the reduction kernels of the row-sparse embedding backward owe (csrc/nrx_embed.hip: the placement pass, the pair pass, the lane-group
walk, the work lists of the hot rows, the general kernel), for tests/test_sparse_bwd_kernels_gpu.py.  Held to oracle/ref_np.py, to float64
autograd and to the library's own size functions by tests/test_sparse_bwd_ref.py.  Backward of base_model.py:262-308 (+ fm/model.py:18-26,
widedeep/model.py:53-69).

  * DEFINITION (from include/nrx_embed.h, not from the kernels): values[u] = the sum over the sorted entries of unique row u of the lookup's
    upstream columns times 1 | w / (sum w + 1e-8) | 1 / L | w; a wide feature's column 0 comes from g_wide; an FM field adds g_fm to column 0
    and g_fm (S_k - v_k) to column k; zeros where the key's low 40 bits are 0.  int64 on integer inputs, float64 otherwise.
  * LAUNCH ARITHMETIC restated from the source as functions of the case: the fast-form condition, ql / tb / long_t, the decode forms, unal,
    bag_shape, placed, the lines form, rows per lane group, the walk grid and its caps, the pair blocks, the work items and their groups, the
    workspace sizes, and which instantiation of NRX_SF / NRX_SL / NRX_PL a launch takes.
  * A MODEL of the decomposition (placed rows, pair rows, walked rows, items, per-group partials, the final sum) that mistakes can be
    planted in.
  * CASE LISTS computed from that arithmetic.  Ids come from a multiplicity ladder: row r of table 0 is looked up exactly m_r times, the
    positions scattered over samples and features by a seed.

EXACTNESS.  Upstream gradients, FM values and g_fm are small integers; every sum a kernel can form has a sum of |terms| below 2^24
(`exact_margin`, asserted per case), so every float32 operation is exact in any order and grouping and the int64 result is owed word for
word.  Bags: NRX_BAG_SUM with small integer weights; NRX_BAG_MEAN with L a power of two; masked mean with 0/1 masks whose row sums are 0 or a
power of two -- bag_scale_kernel forms den = sum w + 1e-8f in float32, where 1e-8 is below half an ulp of any sum >= 1 (ulp(1) = 2^-23), so den
is the sum itself and w / den a power of two; a row sum of 0 gives 0 / 1e-8 = 0."""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import ref_np as R

SPARSE, MASKED, MEAN, SUM = 0, 2, 3, 4                     # enum nrx_feature_kind
MANY_PER_ROW = 4                                           # NRX_FEAT_MANY_PER_ROW
BLOCK = 256                                                # NRX_BLOCK
LONG_T = 16                                                # SORTED_LONG_T
CHUNK = 256                                                # SORTED_LONG_CHUNK: entries per work item
GROUP = 32                                                 # SORTED_LONG_GROUP: items counted in groups above this many
COOP = 4                                                   # rows of more items are written by the whole wavefront
WALK_CAP, PAIR_WALK_CAP, PAIR_CAP = 4096, 512, 512
ROW_MASK = (1 << 40) - 1
SIZEOF_ITEM, SIZEOF_MULTI = 24, 16                         # LongItem {i32, i32, i64, i32, i32}; LongMulti {i32 x 4}


# ------------------------------------------------------------------------------------------------- cases
class Feat:
    def __init__(self, kind=SPARSE, table=0, bag_len=0, out_col=0, wide_col=-1, fm=0, flags=0):
        self.kind, self.table, self.bag_len, self.out_col, self.wide_col, self.fm, self.flags = kind, table, bag_len, out_col, wide_col, fm, flags

    @property
    def per_sample(self):
        return 1 if self.kind == SPARSE else self.bag_len


class Case(NS):
    """name, dim, batch, feats, rows (per table), ids (per feature: [B] or [B, L]), weights (per feature or None), index_bits,
    g_out [B, out_w] / None, g_wide [B, wide_w] / None, fm: None or NS(g_fm [B], feat [B, out_w], sums [B, dim]),
    pads: NS(out, wide, feat, sums) extra columns of stride padding, shift: set of operand names that sit one element into their buffer,
    mode: 'sorted' | 'placed' | 'pairs', dense: bool, accumulate: 0 | 1, ws: workspace given (nrx_embed_bwd_workspace_for bytes),
    n_dev: None | 'equal' | int (the device-side count of unique rows -- or of walk rows when placed -- below the host bound),
    place_feats: mask."""

    @property
    def n_tables(self):
        return len(self.rows)

    @property
    def lens(self):
        return [self.batch * f.per_sample for f in self.feats]

    @property
    def n_lookups(self):
        return sum(self.lens)

    @property
    def integer(self):
        return all(f.kind in (SPARSE, SUM) for f in self.feats)


def mapped_ids(case, i):
    """Feature i's ids as the planner maps them: out-of-range ids fall on row 0."""
    ids = np.asarray(case.ids[i], np.int64).reshape(-1)
    return np.where((ids < 0) | (ids >= case.rows[case.feats[i].table]), 0, ids)


def lookup_terms(case, fm_col_bug=False):
    """Per flat lookup (feature-major): its contribution [n, dim] to its row and the sum of |products| that contribution was formed from.
    int64 on integer inputs; float64 (exact: power-of-two factors) with mean bags."""
    dt = np.int64 if case.integer else np.float64
    D, B = case.dim, case.batch
    terms, mags = [], []
    for i, f in enumerate(case.feats):
        L = f.per_sample
        b = np.repeat(np.arange(B), L)
        g = np.zeros((B * L, D), dt)
        if f.wide_col >= 0:
            if case.g_wide is not None:
                g[:, 0] = case.g_wide[b, f.wide_col]
            if case.g_out is not None:
                g[:, 1:] = case.g_out[b, f.out_col:f.out_col + D - 1]
        elif case.g_out is not None:
            g[:] = case.g_out[b, f.out_col:f.out_col + D]
        m = np.abs(g)
        if case.fm is not None and f.fm and f.wide_col < 0:
            gf = case.fm.g_fm[b].astype(dt)[:, None]
            s, v = case.fm.sums[b, :D].astype(dt), case.fm.feat[b, f.out_col:f.out_col + D].astype(dt)
            add = gf * (s - v)
            madd = np.abs(gf) * (np.abs(s) + np.abs(v))
            if not fm_col_bug:
                add[:, 0], madd[:, 0] = gf[:, 0], np.abs(gf[:, 0])
            else:
                add[:], madd[:] = gf, np.abs(gf)
            g, m = g + add, m + madd
        if f.kind == SUM and case.weights[i] is not None:
            w = np.asarray(case.weights[i]).reshape(-1).astype(dt)[:, None]
            g, m = g * w, m * np.abs(w)
        elif f.kind == MEAN:
            g, m = g / L, m / L
        elif f.kind == MASKED:
            w = np.asarray(case.weights[i], np.float64).reshape(B, L)
            den = w.sum(1, keepdims=True)
            sc = np.where(den > 0, w / np.where(den > 0, den, 1.0), 0.0).reshape(-1)[:, None]       # (0 / 1e-8 = 0; den >= 1: den + 1e-8 rounds to den)
            g, m = g * sc, m * sc
        terms.append(g)
        mags.append(m)
    return np.concatenate(terms), np.concatenate(mags)


def plan_of(case):
    """The host-built plan of a case: oracle/ref_np.py's arrays in the form the entry points take."""
    ids = [mapped_ids(case, i) for i in range(len(case.feats))]
    table_of = [f.table for f in case.feats]
    rows = [case.rows[t] for t in table_of]
    order, uniq, seg, counts = R.sparse_plan(ids, table_of, rows, case.n_tables)
    p = NS(order=order, uniq=uniq, seg=seg, counts=counts, dest=None, walk=None, pairs=None)
    n = len(order)
    if case.mode == "placed":
        _, _, _, _, p.dest, p.walk = R.sparse_plan_place(ids, table_of, rows, case.n_tables, [i for i in range(len(ids)) if (case.place_feats >> i) & 1])
    elif case.mode == "pairs":
        _, _, p.dest, recs, p.walk, _ = R.sparse_plan_pairs(ids, table_of, rows, case.n_tables)
        p.pairs = np.zeros((n // 2 + 1, 4), np.int32)
        p.pairs[:len(recs), :3] = recs
        p.n_pairs = len(recs)
    return p


def definition(case, plan=None, terms=None):
    """values [n_unique, dim] (int64 / float64) and the per-element sum of |terms| (the exactness margin is read off it)."""
    plan = plan or plan_of(case)
    T, M = terms if terms is not None else lookup_terms(case)
    nu = len(plan.uniq)
    vals = np.add.reduceat(T[plan.order], plan.seg[:-1], axis=0) if nu else np.zeros((0, case.dim), T.dtype)
    mag = np.add.reduceat(M[plan.order], plan.seg[:-1], axis=0) if nu else np.zeros((0, case.dim), M.dtype)
    pad = (plan.uniq & ROW_MASK) == 0
    vals[pad] = 0
    mag[pad] = 0
    return vals, mag


def exact_margin(case, mag):
    """The largest sum of |terms| any kernel sum can reach, in units of the smallest power of two the terms are multiples of: must stay
    below 2^24 for float32 to be exact in any order and grouping."""
    unit = 1
    for f in case.feats:
        if f.kind in (MEAN, MASKED):
            unit = max(unit, f.bag_len)
    return float(mag.max()) * unit if mag.size else 0.0


def dense_definition(case, plan, vals, before):
    """grad_tables[t][row] stored or added per `accumulate`; untouched rows keep their bits (`before`: list of [rows, dim] arrays)."""
    out = [b.copy() for b in before]
    for u, key in enumerate(plan.uniq):
        t, r = int(key >> 40), int(key & ROW_MASK)
        out[t][r] = vals[u] + (before[t][r] if case.accumulate else 0)
    return out


# ------------------------------------------------------------------------------------------------- launch arithmetic
def ceil_log2(x):
    return int(x - 1).bit_length() if x > 1 else 0


def long_slots(nchunks):
    ng = -(-nchunks // GROUP) if nchunks > GROUP else 0
    return nchunks + (ng + (ng + 3) // 4 if ng else 0)


def sorted_workspace(n, dim):
    """nrx_embed_bwd_sorted_workspace."""
    items, slots = n // LONG_T + 8, 2 * n // CHUNK + n // 2048 + 8
    return 32 + items * SIZEOF_ITEM + slots * SIZEOF_MULTI + slots * dim * 4 + 64 + 2 * (n * 4 + 64) + n // 8 + 128


def workspace_for(case):
    """nrx_embed_bwd_workspace_for."""
    gs = any(f.kind in (MASKED, MEAN) for f in case.feats)
    return sorted_workspace(case.n_lookups, case.dim) + 512 + (len(case.feats) * case.batch * case.dim * 4 if gs else 0)


def launch(case, plan=None):
    """sorted_bwd_pack / _classify / _run_fast / _launch_place / _launch_walk restated.  Operands are 128-byte aligned unless named in
    case.shift (then one element in)."""
    D, F, B = case.dim, len(case.feats), case.batch
    s = NS()
    has_fm = case.fm is not None
    al = lambda name: name not in case.shift
    out_ld = (case.g_out.shape[1] if case.g_out is not None else 0) + case.pads.out
    s.ql = min(ceil_log2((D + 3) // 4), 6)
    s.tb = BLOCK >> s.ql
    fast = D == (4 << s.ql) and 2 <= s.ql <= 4 and al("values")
    if has_fm:
        feat_ld, sums_ld = case.fm.feat.shape[1] + case.pads.feat, case.fm.sums.shape[1] + case.pads.sums
        fast = fast and al("feat") and feat_ld % 4 == 0 and al("sums") and sums_ld % 4 == 0 and sums_ld >= D
    unal = not (case.g_out is None or (al("g_out") and out_ld % 4 == 0))
    has_bag = False
    for f in case.feats:
        if not fast:
            break
        unal |= f.wide_col >= 0 or f.out_col % 4 != 0
        if f.wide_col >= 0:
            fast = f.kind == SPARSE
        has_bag |= f.kind != SPARSE
    if unal:
        fast = fast and not has_fm                       # (one element in is still 4-byte aligned)
    if has_bag:
        fast = fast and case.ws and not has_fm
    s.long_t = LONG_T
    if has_bag or any(f.flags & MANY_PER_ROW for f in case.feats):
        s.long_t = 2 * LONG_T
    lens = case.lens
    uniform = lens[0] if all(x == lens[0] for x in lens) and lens[0] >= 2 else 0
    stride = case.feats[1].out_col - case.feats[0].out_col if F > 1 else D
    regular = uniform > 0 and F > 4 and all(f.kind == SPARSE and f.wide_col < 0 and f.out_col == case.feats[0].out_col + i * stride and
                                             bool(f.fm and has_fm) == bool(case.feats[0].fm and has_fm) for i, f in enumerate(case.feats))
    s.has_fm, s.fast, s.unal, s.has_bag = has_fm, fast, unal, has_bag
    s.placed = fast and case.mode in ("placed", "pairs")
    s.bag_shape = has_bag and not unal and not has_fm
    s.reg = regular and (case.g_out is not None or has_fm) and not unal
    s.few = F <= 4
    s.dec = 1 if s.reg else (2 if s.few else 0)
    s.refused = case.mode == "pairs" and not (s.placed and not has_bag)
    s.general_grid = -(-len(plan.uniq) // s.tb) if plan is not None else None
    if not fast or plan is None:
        return s
    # ---- sorted_bwd_run_fast
    n_rows, off = len(plan.uniq), case.n_lookups
    placed_feats = [i for i in range(F) if (case.place_feats >> i) & 1] if s.placed else []
    if s.placed:
        placeable = B * len(placed_feats)
        n_rows = min(n_rows, placeable // 2 + (off - placeable) + F + 1)
    s.n_rows = n_rows
    s.place_runs = s.placed and len(placed_feats) > 0
    # ---- the placement pass
    if s.place_runs:
        lines = s.ql == 2 and not unal and (case.g_out is not None or has_fm) and (case.g_out is None or out_ld % 32 == 0) and len(placed_feats) <= 64
        if lines and has_fm:
            lines = al("feat") and (case.fm.feat.shape[1] + case.pads.feat) % 32 == 0
        for k, i in enumerate(placed_feats):
            f = case.feats[i]
            if f.wide_col >= 0:
                lines = False
            if (f.out_col % 32 != 0) if k % 2 == 0 else (f.out_col != case.feats[placed_feats[k - 1]].out_col + 16):
                lines = False
        s.lines = lines
        s.place_grid = -(-B // 32) if lines else -(-B // s.tb)
        if lines:
            s.place_inst = ("lines", has_fm or case.g_out is None, case.dense, case.g_out is not None)
        else:
            s.place_inst = ("rows", has_fm, unal and not has_fm, case.dense)
    # ---- pair blocks
    s.pair_blocks, s.pairs_alone = 0, False
    if case.mode == "pairs":
        s.pair_blocks = min(PAIR_CAP, -(-(off // 2 + 1) // s.tb))
        s.pair_grid = s.pair_blocks
        if unal:
            s.pairs_alone, s.pair_blocks = True, 0
    # ---- the walk
    wide_pass = s.bag_shape or s.placed
    s.R = 2 if wide_pass else 4
    s.groups = -(-n_rows // s.R)
    grid = -(-s.groups // s.tb)
    if (case.n_dev is not None or s.placed) and grid > WALK_CAP:
        grid = WALK_CAP
    if case.mode == "pairs" and grid > PAIR_WALK_CAP:
        grid = PAIR_WALK_CAP
    s.grid = grid
    pb, fm, reg, few, bag = s.pair_blocks != 0, has_fm, s.reg, s.few, has_bag
    d = 2 if few else 0
    if pb:
        s.walk_inst = (2, fm, False, False, 4, 1 if reg else 0, True)
    elif s.placed and fm and reg:
        s.walk_inst = (2, True, False, False, 4, 1, False)
    elif s.placed and not bag and not unal and not fm and reg:
        s.walk_inst = (2, False, False, False, 4, 1, False)
    elif not s.placed and fm and reg:
        s.walk_inst = (4, True, False, False, 1, 1, False)
    elif not s.placed and not fm and not unal and not bag and reg:
        s.walk_inst = (4, False, False, False, 1, 1, False)
    elif s.placed and fm:
        s.walk_inst = (2, True, False, False, 4, d, False)
    elif s.placed and unal:
        s.walk_inst = (2, False, True, True, 4, d, False)
    elif s.placed and not bag:
        s.walk_inst = (2, False, False, False, 4, d, False)
    elif fm:
        s.walk_inst = (4, True, False, False, 1, d, False)
    elif unal:
        s.walk_inst = (4, False, True, True, 1, d, False)
    elif bag:
        s.walk_inst = (2, False, True, False, 4, d, False)
    else:
        s.walk_inst = (4, False, False, False, 1, d, False)
    assert s.walk_inst[0] == s.R, "the kernel's R and the grid's rows per lane group must agree"
    s.long_inst = None
    if case.ws:
        if fm and reg:
            s.long_inst = (True, False, False, 1)
        elif not fm and not unal and not bag and reg:
            s.long_inst = (False, False, False, 1)
        elif fm:
            s.long_inst = (True, False, False, d)
        elif unal:
            s.long_inst = (False, True, True, d)
        elif bag:
            s.long_inst = (False, True, False, d)
        else:
            s.long_inst = (False, False, False, d)
        Q = 1 << s.ql
        s.long_G, s.long_UL = 64 // Q, min(Q, 8)             # sorted_long_kernel: 64-entry order chunks, G lane groups, UL rows in flight
    return s


def row_items(length):
    """The work items of a row of `length` sorted entries: (first entry, entries) each, and its partial-sum slots."""
    n = -(-length // CHUNK)
    return [(c * CHUNK, min(CHUNK, length - c * CHUNK)) for c in range(n)], (long_slots(n) if n > 1 else 0)


# ------------------------------------------------------------------------------------------------- the model of the decomposition
BUGS = ("ge_long_t", "last_item_short", "group_dropped", "no_second_trip", "no_second_pair_trip", "padding_summed", "pair_second_dropped",
        "walk_index_as_unique", "fm_col0_everywhere")


def model(case, plan, sh, bug=None, terms=None):
    """(values [n_unique, dim] as the launches form them, NaN where no launch writes -- float64 throughout: exact on the cases' integers;
    the work lists' counters: items, rows of several items, partial-sum slots).
    General kernel: one lane group per unique row.  Fast form: the placement pass stores the placed rows; the pair blocks (striding over the
    records) store first + second; the walk's blocks stride over groups of R listed rows: a row past long_t entries (with a workspace) is cut
    into items of 256 entries, the items' partials are added per group of 32 when there are more than 32, the group partials last."""
    T = (terms if terms is not None else lookup_terms(case, fm_col_bug=bug == "fm_col0_everywhere"))[0].astype(np.float64)
    nu, D = len(plan.uniq), case.dim
    vals = np.full((nu, D), np.nan)
    S = np.concatenate([np.zeros((1, D)), np.cumsum(T[plan.order], axis=0)])           # prefix sums over the sorted entries (exact: integers < 2^53)
    seg, row = plan.seg, plan.uniq & ROW_MASK
    count = nu
    facts = NS(items=0, multi=0, slots=0)                   # what the walk leaves in the work lists' counters (long_ws[0..2])
    if not sh.fast:
        n = count if case.n_dev in (None, "equal") else min(count, case.n_dev)
        u = np.arange(n)
        vals[u] = S[seg[u + 1]] - S[seg[u]]
        if bug != "padding_summed":
            vals[u[row[u] == 0]] = 0
        return vals, facts
    if sh.placed and sh.place_runs:
        p = np.nonzero(plan.dest >= 0)[0]
        vals[plan.dest[p]] = T[p]
    if case.mode == "pairs":
        recs = plan.pairs[:plan.n_pairs]
        k = np.arange(len(recs))
        if bug == "no_second_pair_trip":
            k = k[k < (sh.pair_grid * sh.tb)]
        recs = recs[k]
        vals[recs[:, 0]] = T[recs[:, 1]] + (0 if bug == "pair_second_dropped" else T[recs[:, 2]])
    listed = plan.walk.astype(np.int64) if sh.placed else np.arange(nu)
    n = len(listed) if case.n_dev in (None, "equal") else min(len(listed), case.n_dev)
    n = min(n, sh.n_rows)
    i = np.arange(n)
    if bug == "no_second_trip":
        i = i[(i // sh.R) // sh.tb < sh.grid]
    u = i if bug == "walk_index_as_unique" else listed[i]
    lo, hi = seg[u], seg[u + 1]
    if bug != "padding_summed":
        hi = np.where(row[u] == 0, lo, hi)
    length = hi - lo
    lng = (length >= sh.long_t if bug == "ge_long_t" else length > sh.long_t) if case.ws else np.zeros(len(u), bool)
    vals[u[~lng]] = S[hi[~lng]] - S[lo[~lng]]
    for uu, l0, ln in zip(u[lng], lo[lng], length[lng]):
        items, slots = row_items(int(ln))
        facts.items, facts.multi, facts.slots = facts.items + len(items), facts.multi + (len(items) > 1), facts.slots + slots
        if bug == "last_item_short":
            items[-1] = (items[-1][0], items[-1][1] - 1)
        part = [S[l0 + a + b] - S[l0 + a] for a, b in items]
        if len(part) > GROUP:
            ng = len(part) // GROUP if bug == "group_dropped" else -(-len(part) // GROUP)
            part = [np.sum(part[g * GROUP:(g + 1) * GROUP], axis=0) for g in range(ng)]
        vals[uu] = np.sum(part, axis=0)
    return vals, facts


# ------------------------------------------------------------------------------------------------- case construction
def ladder_ids(slots, ladder, rows_needed, pad=0, oor=0, seed=0, first_row=1):
    """`slots` ids of one table: row first_row + j exactly ladder[j] times, `pad` zeros, `oor` ids that are no rows (they fall on row 0), the
    rest distinct rows looked up once; scattered over the slots by the seed.  Returns (ids, rows of the table)."""
    body = [np.full(m, first_row + j, np.int64) for j, m in enumerate(ladder)]
    used = sum(ladder) + pad + oor
    assert used <= slots, (used, slots)
    nxt = first_row + len(ladder)
    rest = np.arange(nxt, nxt + slots - used, dtype=np.int64)
    rows = max(rows_needed, nxt + slots - used + 1)
    bad = np.array([rows + 5, -3, rows, -(1 << 40)][:oor] + [rows + 7] * max(0, oor - 4), np.int64)
    ids = np.concatenate(body + [np.zeros(pad, np.int64), bad, rest])
    return ids[np.random.default_rng(seed).permutation(slots)], rows


def _ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def make_case(name, dim, batch, variant="plain", n_feats=1, shared=False, uneven=False, ladder=(), pad=1, oor=0, mode="sorted", dense=False,
              accumulate=0, ws=True, n_dev=None, bag=None, bag_len=4, index_bits=64, pads=(0, 0, 0, 0), shift=(), many=False, seed=0,
              place_mask=None, pad_table1=0, wide_feats=None, lines=False, glim=3):
    """One case.  variant: plain | fm | fm_nog (FM without g_out) | wide (column routing) | bag (feature 1 of >= 2 is a bag of kind `bag`).
    shared: every feature reads table 0 (else feature i reads table i).  uneven: a gap of 4 columns after feature 1 (no regular spacing).
    The ladder goes to table 0; the other tables are looked up at distinct rows plus pad_table1 zeros."""
    rng = np.random.default_rng(seed + 1000 * dim + n_feats)
    feats, col, wcol = [], 0, 0
    wide_feats = (1,) if wide_feats is None and variant == "wide" else (wide_feats or ())
    for i in range(n_feats):
        kind, L = SPARSE, 0
        if variant == "bag" and i == min(1, n_feats - 1):
            kind, L = bag or MASKED, bag_len
        f = Feat(kind, 0 if shared else i, L, col, fm=int(variant in ("fm", "fm_nog") and kind == SPARSE), flags=MANY_PER_ROW if many else 0)
        if i in wide_feats and kind == SPARSE:
            f.wide_col, wcol = wcol, wcol + 1
            col += dim - 1
        else:
            col += dim
        if lines and dim == 16 and i % 2 == 1:
            col = -(-col // 32) * 32
        if uneven and i == 1:
            col += 4
        feats.append(f)
    n_tables = 1 if shared else n_feats
    slots = [sum(batch * f.per_sample for f in feats if f.table == t) for t in range(n_tables)]
    ids_t, rows = [], []
    for t in range(n_tables):
        a, r = ladder_ids(slots[t], ladder if t == 0 else (), 8, pad if t == 0 else pad_table1, oor if t == 0 else 0, seed + t)
        ids_t.append(a)
        rows.append(r)
    ids, taken = [], [0] * n_tables
    for f in feats:
        k = batch * f.per_sample
        a = ids_t[f.table][taken[f.table]:taken[f.table] + k]
        taken[f.table] += k
        ids.append(a.reshape(batch, f.bag_len) if f.kind != SPARSE else a)
    weights = [None] * n_feats
    for i, f in enumerate(feats):
        if f.kind == MASKED:                                 # 0/1 masks whose row sums are 0 or a power of two; zero weights on live ids too
            k = 2 ** rng.integers(0, ceil_log2(f.bag_len) + 1, batch)
            k = np.where(rng.random(batch) < 0.1, 0, np.minimum(k, 2 ** (f.bag_len.bit_length() - 1)))
            weights[i] = (np.argsort(rng.random((batch, f.bag_len)), axis=1) < k[:, None]).astype(np.float32)
        elif f.kind == SUM:
            weights[i] = rng.integers(0, 3, (batch, f.bag_len)).astype(np.float32)
    out_w = max(col, 1)
    if lines:
        out_w = -(-out_w // 32) * 32
    c = Case(name=name, dim=dim, batch=batch, feats=feats, rows=rows, ids=ids, weights=weights, index_bits=index_bits,
             g_out=None if variant == "fm_nog" else _ints(rng, (batch, out_w), glim), g_wide=_ints(rng, (batch, wcol), glim) if wcol else None, fm=None,
             pads=NS(out=pads[0], wide=pads[1], feat=pads[2], sums=pads[3]), shift=set(shift), mode=mode, dense=dense, accumulate=accumulate,
             ws=ws, n_dev=n_dev, place_feats=0, variant=variant)
    if mode != "sorted":
        c.place_feats = place_mask if place_mask is not None else sum(1 << i for i, f in enumerate(feats) if f.kind == SPARSE)
    if variant in ("fm", "fm_nog"):                          # a consistent forward: integer tables, feat = the rows read, sums over the fields
        tables = [rng.integers(-2, 3, (r, dim)).astype(np.float32) for r in rows]
        for t in tables:
            t[0] = 0
        feat = np.zeros((batch, out_w), np.float32)
        sums = np.zeros((batch, dim), np.float32)
        for i, f in enumerate(feats):
            v = tables[f.table][mapped_ids(c, i)]
            feat[:, f.out_col:f.out_col + dim] = v
            sums += v
        c.fm = NS(g_fm=_ints(rng, (batch,), 2), feat=feat, sums=sums, tables=tables)
    return c


# ---- ladders
SHORT = (1, 2, 3, 4, 5, 8, 9, LONG_T - 1, LONG_T, LONG_T + 1, 2 * LONG_T - 1, 2 * LONG_T, 2 * LONG_T + 1, 63, 64, 65)
MID = (CHUNK - 1, CHUNK, CHUNK + 1, COOP * CHUNK, COOP * CHUNK + 1)
HOT = (GROUP * CHUNK, GROUP * CHUNK + 1)
HOTTEST = (66 * CHUNK + 77,)                                # 67 items: two full groups and a partial one of 3
VARIANTS = ("plain", "fm", "fm_nog", "wide", "bag")
GENERAL_DIMS = (1, 3, 5, 12, 17, 100, 256, 257, 300)


def _need(ladder, pad, per_sample_slots):
    return -(-(sum(ladder) + pad + 8) // per_sample_slots)


@functools.lru_cache(maxsize=None)
def _cases():
    cs = {}

    def add(c):
        assert c.name not in cs, c.name
        cs[c.name] = c

    # -- every branch of NRX_SF / NRX_SL / NRX_PL: dim x variant x decode form x entry point, on the short ladder
    for dim in (16, 32, 64):
        for variant in VARIANTS:
            for dec, (nf, shared, uneven) in dict(reg=(5, False, False), few=(3, False, False), gen=(6, True, True)).items():
                if dec == "reg" and variant in ("wide", "bag"):
                    continue                                    # (a regular launch has neither: those take the other two forms)
                modes = [("sorted", False, 0, True), ("sorted", False, 0, False), ("placed", False, 0, True), ("placed", True, 0, True),
                         ("placed", True, 1, True)]
                if variant != "bag":
                    modes += [("pairs", False, 0, True), ("pairs", True, 1, True)]
                for k, (mode, dense, acc, ws) in enumerate(modes):
                    L = 4
                    per = (nf + (L - 1 if variant == "bag" else 0)) if shared else 1
                    B = max(_need(SHORT, 2, per), 40) + (k % 3)
                    add(make_case(f"b-d{dim}-{variant}-{dec}-{mode}{'-dense%d' % acc if dense else ''}{'' if ws else '-nows'}", dim, B, variant, nf, shared,
                                  uneven, SHORT, pad=2, oor=2 if k % 2 else 0, mode=mode, dense=dense, accumulate=acc, ws=ws, bag_len=L,
                                  bag=(MASKED, MEAN, SUM)[(k + dim // 16) % 3], index_bits=(64, 32)[k % 2], seed=k + dim, pad_table1=1,
                                  n_dev="equal" if k % 2 else None))
    # -- long rows: every item edge, both thresholds, placed and not
    for dim, variant, many in ((16, "plain", False), (32, "fm", False), (64, "plain", True), (16, "bag", False)):
        for mode in ("sorted", "placed"):
            per = 2 + (3 if variant == "bag" else 0)
            add(make_case(f"mid-d{dim}-{variant}{'-many' if many else ''}-{mode}", dim, _need(SHORT + MID, 1, per), variant, 2, True, False, SHORT + MID,
                          mode=mode, many=many, bag=MEAN, seed=dim))
    add(make_case("hot-d16-plain-sorted", 16, _need(HOT + HOTTEST, 40, 3), "plain", 3, True, False, HOT + HOTTEST + (LONG_T + 1, 3), seed=1, glim=2))
    add(make_case("hot-d64-fm-placed", 64, _need(HOT + HOTTEST, 300, 2), "fm", 2, True, False, HOT + HOTTEST + (CHUNK + 1, 2), mode="placed", seed=2, glim=2))
    # -- padding rows: first of its table, among live rows of a lane group, longer than long_t (no item), in a second table, ids that are no rows
    add(make_case("pad-long-d16", 16, 200, "plain", 2, False, False, (3, 17, 2), pad=40, oor=4, pad_table1=35, seed=3))
    add(make_case("pad-long-d32-placed", 32, 200, "fm", 2, False, False, (3, 17, 2), pad=40, oor=4, pad_table1=35, mode="placed", seed=4))
    add(make_case("pad-long-d64-pairs", 64, 200, "plain", 2, False, False, (3, 17, 2), pad=40, oor=4, pad_table1=35, mode="pairs", seed=5))
    # -- unique-row counts around whole blocks of lane groups, and a device-side count below the host bound
    for dim, R_ in ((16, 4), (32, 4), (64, 2)):
        tb = BLOCK // (dim // 4)
        for nu in (R_ * tb - 1, R_ * tb, R_ * tb + 1, 3 * R_ * tb + 5):
            if R_ == 4:                                         # sorted: every unique row is walked -- nu - 1 distinct rows and the padding row
                add(make_case(f"count-d{dim}-R4-{nu}", dim, nu + 6, "plain", 1, True, False, (4, 3, 2), pad=1, seed=nu))
            else:                                               # placed: nu walk rows of two lookups each (one of them the padding row)
                add(make_case(f"count-d{dim}-R2-{nu}", dim, 2 * nu + 9, "plain", 1, True, False, (2,) * (nu - 1), pad=3, mode="placed", seed=nu))
    add(make_case("ndev-d16-sorted", 16, 300, "plain", 2, True, False, SHORT, n_dev=150, seed=6))
    add(make_case("ndev-d16-general", 12, 120, "plain", 2, True, False, SHORT[:8], n_dev=31, seed=6))
    add(make_case("ndev-d32-placed", 32, 300, "fm", 2, True, False, SHORT + (2,) * 40, n_dev=25, mode="placed", seed=7))
    # -- the strides, at dim 64 (tb = 16)
    add(make_case("stride-walk-d64", 64, WALK_CAP * 16 * 4 + 4 * 16 + 7, "plain", 1, True, False, (2, 3), n_dev="equal", seed=8))
    add(make_case("stride-pairs-d64", 64, 2 * (PAIR_CAP * 16 + 16 + 5) + 11, "plain", 1, True, False, (2,) * (PAIR_CAP * 16 + 16 + 5), mode="pairs", seed=9))
    add(make_case("stride-pairwalk-d64", 64, 3 * (PAIR_WALK_CAP * 16 * 2 + 2 * 16 + 3) + 13, "plain", 1, True, False,
                  (3,) * (PAIR_WALK_CAP * 16 * 2 + 2 * 16 + 3), mode="pairs", seed=10))
    # -- the placement pass: tb - 1 / tb / tb + 1 samples; the lines form at 31 / 32 / 33 samples, odd and even feature counts, 64 features
    for dim in (16, 32, 64):
        tb = BLOCK // (dim // 4)
        for B in (tb - 1, tb, tb + 1):
            add(make_case(f"place-d{dim}-B{B}", dim, B, "plain", 3, False, False, (2, 3), mode="placed", seed=B, dense=B == tb, accumulate=0))
    for nf in (1, 2, 7, 64):
        for B in (31, 32, 33):
            for variant in ("plain", "fm", "fm_nog"):
                if nf in (1, 64) and variant == "fm_nog" and B != 33:
                    continue
                add(make_case(f"lines-f{nf}-B{B}-{variant}", 16, B, variant, nf, False, False, (2, 3) if B > 8 else (), mode="placed",
                              dense=(B + nf) % 2 == 1, lines=True, seed=B + nf))
    add(make_case("lines-refused-ld", 16, 33, "plain", 4, False, False, (2, 3), mode="placed", lines=True, pads=(4, 0, 0, 0), seed=11))
    add(make_case("lines-refused-cols", 16, 33, "fm", 6, False, True, (2, 3), mode="placed", seed=12))
    # -- the general kernel
    for dim in GENERAL_DIMS:
        add(make_case(f"gen-d{dim}", dim, 70, "plain", 2, True, False, SHORT[:10], index_bits=(64, 32)[dim % 2], seed=dim, oor=2))
    add(make_case("gen-d1028-slow-loop", 1028, 24, "plain", 2, True, False, (1, 2, 3, 17), seed=13))
    add(make_case("gen-d1028-slow-loop-fm", 1028, 24, "fm", 2, True, False, (1, 2, 3, 17), seed=13))
    add(make_case("gen-d17-fm", 17, 60, "fm", 3, True, False, SHORT[:9], seed=14))
    add(make_case("gen-d16-fm-bag", 16, 60, "fm", 3, False, False, SHORT[:8], seed=15))      # (made FM + bag below)
    c = cs["gen-d16-fm-bag"]
    c.feats.append(Feat(MASKED, 0, 4, c.g_out.shape[1]))
    c.ids.append(ladder_ids(60 * 4, (5, 9), 8, pad=30, seed=16)[0].reshape(60, 4))
    c.rows[0] = max(c.rows[0], 60 * 4 + 8)
    c.fm.tables[0] = np.concatenate([c.fm.tables[0], np.ones((c.rows[0] - len(c.fm.tables[0]), 16), np.float32)])      # (rows only the bag reads)
    c.weights.append((np.arange(4)[None, :] < np.random.default_rng(1).choice([0, 1, 2, 4], 60)[:, None]).astype(np.float32))
    c.g_out = np.concatenate([c.g_out, _ints(np.random.default_rng(2), (60, 16), 3)], axis=1)
    c.fm.feat = np.concatenate([c.fm.feat, np.zeros((60, 16), np.float32)], axis=1)
    add(make_case("gen-d15-wide-odd", 15, 60, "wide", 3, False, False, SHORT[:8], wide_feats=(0, 2), seed=17))
    add(make_case("gen-d16-bag-nows", 16, 60, "bag", 2, True, False, SHORT[:8], ws=False, bag=SUM, seed=18))
    # -- layouts: padded strides (the padding poisoned), operands one element in (off the fast form, or onto its unaligned kernels)
    add(make_case("ld-d16-fm", 16, 90, "fm", 5, False, False, SHORT[:10], pads=(8, 0, 12, 4), mode="placed", seed=19))
    add(make_case("ld-d32-wide", 32, 90, "wide", 3, False, False, SHORT[:10], pads=(3, 2, 0, 0), mode="placed", seed=20))
    add(make_case("ld-d16-odd-out", 16, 90, "plain", 5, False, False, SHORT[:10], pads=(1, 0, 0, 0), seed=21))
    add(make_case("shift-values-d16", 16, 90, "plain", 5, False, False, SHORT[:10], shift=("values",), mode="placed", seed=22))
    add(make_case("shift-gout-d32", 32, 90, "plain", 3, False, False, SHORT[:10], shift=("g_out",), mode="placed", seed=23))
    add(make_case("shift-gout-d16-fm", 16, 90, "fm", 5, False, False, SHORT[:10], shift=("g_out",), seed=24))
    add(make_case("shift-feat-d16-fm", 16, 90, "fm", 5, False, False, SHORT[:10], shift=("feat",), mode="placed", seed=25))
    add(make_case("shift-sums-d64-fm", 64, 90, "fm", 3, False, False, SHORT[:10], shift=("sums",), seed=26))
    add(make_case("shift-values-d64-pairs", 64, 90, "plain", 3, False, False, SHORT[:10], shift=("values",), mode="pairs", seed=27))
    return cs


def cases():
    return _cases()


def case(name):
    return _cases()[name]


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, plan, launch shape, terms, (values, magnitudes)) of a listed case, computed once and shared."""
    c = case(name)
    p = plan_of(c)
    t = lookup_terms(c)
    return c, p, launch(c, p), t, definition(c, p, t)


def real_cases():
    """Real-valued inputs (randn) on a few of the id patterns: against float64 within a bound counted from the source."""
    out = {}
    for name in ("b-d16-fm-reg-placed", "b-d32-wide-few-sorted", "b-d64-bag-gen-placed", "mid-d32-fm-sorted", "hot-d16-plain-sorted",
                 "b-d64-plain-reg-pairs", "gen-d17-fm", "gen-d300"):
        c = Case(**vars(case(name)))
        rng = np.random.default_rng(len(name))
        c.g_out = rng.standard_normal(c.g_out.shape).astype(np.float32) if c.g_out is not None else None
        c.g_wide = rng.standard_normal(c.g_wide.shape).astype(np.float32) if c.g_wide is not None else None
        if c.fm is not None:
            feat = rng.standard_normal(c.fm.feat.shape).astype(np.float32)
            tables = [rng.standard_normal((r, c.dim)).astype(np.float32) for r in c.rows]
            c.fm = NS(g_fm=rng.standard_normal(c.batch).astype(np.float32), feat=feat, sums=c.fm.sums + 0, tables=tables)
            sums = np.zeros((c.batch, c.dim))
            for i, f in enumerate(c.feats):
                if f.fm:
                    v = tables[f.table][mapped_ids(c, i)]
                    feat[:, f.out_col:f.out_col + c.dim] = v
                    sums += v
            c.fm.sums = sums.astype(np.float32)
        c.weights = [None if w is None else (w if f.kind == MASKED else (w * rng.random(w.shape)).astype(np.float32)) for w, f in zip(c.weights, c.feats)]
        c.name = "real-" + name
        out[c.name] = c
    return out


def real_reference(case, plan):
    """float64 values and the bound C n 2^-24 sum|terms| per element (as tests/embed_cases.py counts it): n = the row's lookups + the FM
    fields (the field sums are float32 sums over the fields), C = 4: the products (fold, factor), the running sum, the tree over items."""
    D, B = case.dim, case.batch
    T, M = [], []
    nfm = sum(1 for f in case.feats if f.fm) if case.fm is not None else 0
    for i, f in enumerate(case.feats):
        L = f.per_sample
        b = np.repeat(np.arange(B), L)
        g = np.zeros((B * L, D))
        if f.wide_col >= 0:
            g[:, 0] = case.g_wide[b, f.wide_col]
            g[:, 1:] = case.g_out[b, f.out_col:f.out_col + D - 1]
        elif case.g_out is not None:
            g[:] = case.g_out[b, f.out_col:f.out_col + D]
        m = np.abs(g)
        if case.fm is not None and f.fm:
            gf = case.fm.g_fm[b].astype(np.float64)[:, None]
            s, v = case.fm.sums[b, :D].astype(np.float64), case.fm.feat[b, f.out_col:f.out_col + D].astype(np.float64)
            add, madd = gf * (s - v), np.abs(gf) * (np.abs(s) + np.abs(v))
            add[:, 0], madd[:, 0] = gf[:, 0], np.abs(gf[:, 0])
            g, m = g + add, m + madd
        if f.kind != SPARSE:
            w = np.ones((B, L)) if f.kind == MEAN or case.weights[i] is None else np.asarray(case.weights[i], np.float64)
            sc = w / (w.sum(1, keepdims=True) + 1e-8) if f.kind == MASKED else (w / L if f.kind == MEAN else w)
            g, m = g * sc.reshape(-1)[:, None], m * np.abs(sc.reshape(-1)[:, None])
        T.append(g)
        M.append(m)
    T, M = np.concatenate(T), np.concatenate(M)
    vals = np.add.reduceat(T[plan.order], plan.seg[:-1], axis=0)
    mag = np.add.reduceat(M[plan.order], plan.seg[:-1], axis=0)
    pad = (plan.uniq & ROW_MASK) == 0
    vals[pad], mag[pad] = 0, 0
    n = (plan.seg[1:] - plan.seg[:-1] + nfm + max([f.bag_len for f in case.feats] + [0]))[:, None]
    return vals, 4.0 * n * 2.0 ** -24 * mag
