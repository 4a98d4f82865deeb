"""Definitions, error bounds, an inbox generator and case lists for the pooled-bag inbox kernels of csrc/nrx_route.hip (nrx_pool_inbox_fwd / _runs
/ _bf16, nrx_pool_inbox_bwd, nrx_pool_inbox_expand, nrx_pool_inbox_owner_ids, nrx_pool_inbox_runs_words, nrx_pool_order_remap,
nrx_bag_norm_weights / _inv, nrx_bag_upstream_rows, nrx_make_table_keys).  numpy only: tests/test_pool_inbox_ref.py holds this file to
oracle/ref_np.py on the CPU, tests/test_pool_inbox_kernels_gpu.py holds the kernels to this file.

An inbox is what nrx_route_bags leaves at an owner: `world` blocks of `cap` slots; block s holds, in its first min(sum(recv2d[s]), cap) slots,
{local row, tag, weight} triples whose tags (tag = f * batch + sample) are non-decreasing, so that the entries of one tag form one RUN.

Three kinds of function:
  *32   the kernel's own float32 arithmetic in the kernel's own order (the forward: entry order, product then add, from +0; contraction is off in
        that loop) and single float32 operations (w * g, m / den): the GPU test asks for these bit for bit;
  *64   the definition in float64 on the same float32 inputs, with the sum of |terms| and the number of terms next to it;
  bounds   gamma(k) * sum |terms| with k counted from the kernel source (u = 2^-24): n products and n - 1 adds on the longest path of a
        sum of n terms is n roundings per term at the most.
"""
import functools
from types import SimpleNamespace

import numpy as np

F32 = np.float32
U = 2.0 ** -24
EPS32 = F32(1e-8)
NRX_BLOCK = 256
AHEAD = 16                               # rows in flight per lane group (NRX_POOL_AHEAD)
MAX_QLOG2 = 6
I32MAX = (1 << 31) - 1
GARBAGE_ROW, GARBAGE_TAG = 10 ** 9, -5   # what every slot past a block's count holds (weight: NaN)


def gamma(n):
    """(1 + u)^n - 1 <= n u / (1 - n u): the exact form of 'n roundings'."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------- launch arithmetic (nrx_route.hip)
def ceil_log2(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def qlog2(dim):
    """pool_ql: lanes per (source, tag) or per entry = 2^QLOG2 = the power of two >= the number of four-column chunks, at most 64."""
    return min(MAX_QLOG2, ceil_log2((dim + 3) // 4))


def lanes(dim):
    return 1 << qlog2(dim)


def tb(dim):
    """Lane groups (tags in the forward, entries in the backward and the expansion) per 256-thread block."""
    return NRX_BLOCK >> qlog2(dim)


def passes(dim):
    return -(-dim // (4 * lanes(dim)))


def epl(dim):
    """Entries a lane loads per AHEAD-entry trip before the group's exchange.  Q = 1 has no exchange (its own load path: all AHEAD entries)."""
    q = lanes(dim)
    return 1 if q >= AHEAD else AHEAD // q


def lanes_beyond_ahead(dim):
    """Lanes of a group that load no entry of a trip (u = q * EPL >= AHEAD) and still take part in the exchange."""
    return max(0, lanes(dim) - AHEAD)


def expand_vector_path(dim):
    """pool_inbox_expand_kernel: one float4 per lane when dim == 4 Q, else a scalar loop."""
    return dim == 4 * lanes(dim)


# ------------------------------------------------------------------------------------------------- case lists
FULL_DIMS = [4 << ql for ql in range(MAX_QLOG2 + 1)] + [2 * 4 * 64, 4 * 4 * 64]      # dim == 4 Q for every Q; two and four full passes
PAST_DIMS = [(4 << ql) + 1 for ql in (0, 2, 3, 5, 6)]                                # one column into the next lane-group width / pass
PART_DIMS = [1, 3, 12, 24, 100, 300]                                                 # dim % 4 != 0, idle lanes, a ragged second pass
DIMS = sorted(set(FULL_DIMS + PAST_DIMS + PART_DIMS))
RUN_MENU = [0, 1, 2, AHEAD - 1, AHEAD, AHEAD + 1, 2 * AHEAD - 1, 2 * AHEAD, 2 * AHEAD + 1, 3 * AHEAD + 2]
TABLE_ROWS = [37, 211]                   # two tables of different row counts
HOT = (1, 5)                             # (table, row) of the hot row
BF16_DIMS = [5, 17, 33, 4, 16, 300, 1024]                                            # scalar path with odd k0; 8-byte vector path


def run_class(n):
    """A run's class by the trips of AHEAD entries it takes."""
    return {0: "0", 1: "1", AHEAD - 1: "AHEAD-1", AHEAD: "AHEAD", AHEAD + 1: "AHEAD+1", 2 * AHEAD + 1: "2AHEAD+1"}.get(n, "other")


RUN_CLASSES = ["0", "1", "AHEAD-1", "AHEAD", "AHEAD+1", "2AHEAD+1"]                    # the issue's 0 / 1 / 15 / 16 / 17 / 33


def inbox_cases(dim):
    """(key, world, n_feats, batch, options) per dim: ntag = n_feats * batch = 1, TB - 1, TB, TB + 1, 3 TB + 5 (the one of TB - 1 / TB / TB + 1
    that 3 divides with three features) at worlds 1 and 2, and the main case -- world 3 with an empty middle block and a last block that
    overflows cap, three features on two tables, rows and tags out of range, a hot row -- at ntag = 3 (TB + 2)."""
    t = tb(dim)
    cases = [("ntag1", 1, 1, 1, {})]
    for x in (t - 1, t, t + 1):
        if x % 3 == 0:
            cases.append((f"ntag{x}", 2, 3, x // 3, {}))
        else:
            cases.append((f"ntag{x}", 2, 1, x, {}))
    cases.append((f"ntag{3 * t + 5}", 1, 1, 3 * t + 5, {}))
    cases.append(("main", 3, 3, t + 2, dict(empty=(1,), overflow=(2,), oob=True, hot=0.6)))
    return cases


def feat_table_of(n_feats):
    """Never the identity: one feature reads table 1, three features read tables 1, 0, 1."""
    return [1, 0, 1][:n_feats] if n_feats == 3 else [1] * n_feats


# ------------------------------------------------------------------------------------------------- the inbox
def mark_runs(tag, recv2d, world, cap, ntag):
    """pool_mark_kernel: run[s, t] = (first entry, one past the last entry) of tag t among block s's first min(sum(recv2d[s]), cap) entries; (0, 0)
    for a tag without one; an entry whose tag lies outside [0, ntag) belongs to no run."""
    tag = np.asarray(tag, np.int64).reshape(world, cap)
    total = np.minimum(np.asarray(recv2d, np.int64).reshape(world, -1).sum(1), cap)
    run = np.zeros((world, ntag, 2), np.int32)
    for s in range(world):
        t = tag[s, :total[s]]
        j = np.arange(t.size)
        ok = (t >= 0) & (t < ntag)
        first = ok & np.r_[True, t[1:] != t[:-1]]
        last = ok & np.r_[t[1:] != t[:-1], True]
        run[s, t[first], 0] = j[first]
        run[s, t[last], 1] = j[last] + 1
    return run


def build_inbox(seed, world, n_feats, batch, cap_slack, dim, table_rows, feat_table, run_menu, empty=(), overflow=(), oob=False, hot=0.0):
    """An inbox in nrx_route_bags' layout.  Every tag of every non-empty block gets a run whose length is drawn from run_menu (every ten
    consecutive tags hold the whole menu, in a random order).  cap = the longest block that fits + cap_slack, made odd (no multiple of a TB or
    of 256); a block of `overflow` holds cap + 20 entries (a run in its middle is lengthened), of which the kernels must see cap; a block of `empty`
    has a recv2d row of zeros.  Slots past a block's count hold garbage.  oob: inside the count, entries with a row outside [0, rows) -- with
    a weight, with weight 0, and one whole run of them -- and single entries with a tag outside [0, ntag), between two runs or at the block's end.
    hot: the fraction of table HOT[0]'s entries that name row HOT[1].  The weights are normal deviates (a few exact zeros)."""
    rng = np.random.default_rng([31, seed, world, n_feats, batch, dim])
    ntag = n_feats * batch
    menu = np.asarray(run_menu, np.int64)
    bad_tags = np.array([-1, GARBAGE_TAG, ntag, ntag + 7, I32MAX, -I32MAX - 1], np.int64)
    lens = {}
    for s in range(world):
        if s in empty:
            continue
        order = np.concatenate([rng.permutation(menu.size) for _ in range(-(-ntag // menu.size))])[:ntag]
        lens[s] = menu[order] if ntag > 1 else menu[[(seed + s + dim) % menu.size]]
    fits = [int(l.sum()) for s, l in lens.items() if s not in overflow]
    n_bad_tags = 5 if oob else 0
    cap = (max(fits, default=8) + n_bad_tags + cap_slack) | 1
    rows = np.full((world, cap), GARBAGE_ROW, np.int32)
    tag = np.full((world, cap), GARBAGE_TAG, np.int32)
    w = np.full((world, cap), np.nan, F32)
    recv2d = np.zeros((world, n_feats), np.int64)
    ft = np.asarray(feat_table, np.int64)
    tr = np.asarray(table_rows, np.int64)
    for s, l in lens.items():
        l = l.copy()
        if s in overflow:
            l[ntag // 2] += max(0, cap + 20 - n_bad_tags - int(l.sum()))
        t = np.repeat(np.arange(ntag, dtype=np.int64), l)
        if oob:                                                      # four single bad tags between runs of different tags, one at the end
            ends = np.cumsum(l)
            inner = np.unique(ends[:-1][(ends[:-1] > 0) & (ends[:-1] < t.size)])
            at = rng.choice(inner, min(4, inner.size), replace=False) if inner.size else np.zeros(0, np.int64)
            at = np.r_[np.sort(at), t.size]
            t = np.insert(t, at, bad_tags[rng.integers(0, bad_tags.size, at.size)])
        n = t.size
        good = (t >= 0) & (t < ntag)
        tix = np.where(good, ft[np.clip(t, 0, ntag - 1) // batch], 0)
        r = rng.integers(0, tr[tix])
        ww = rng.standard_normal(n).astype(F32)
        ww[ww == 0] = F32(1)
        ww[rng.random(n) < 0.02] = F32(0)
        if hot:
            r[(tix == HOT[0]) & good & (rng.random(n) < hot)] = HOT[1]
        if oob:
            outside = np.stack([tr[tix], np.full(n, -1), np.full(n, I32MAX), tr[tix] + 1000])[rng.integers(0, 4, n), np.arange(n)]
            pick = rng.random(n)
            with_w, without_w = pick < 0.03, (pick >= 0.03) & (pick < 0.06)
            cand = np.flatnonzero(good)
            if cand.size >= 8:                                       # at least two of each, early in the block (inside cap)
                with_w[cand[[1, 5]]] = True
                without_w[cand[[2, 6]]] = True
                with_w[cand[[2, 6]]] = False
            whole = np.flatnonzero(l >= 2)
            if whole.size:                                           # one run of nothing but rows out of range
                with_w |= t == whole[0]
            without_w &= ~with_w
            r = np.where(with_w | without_w, outside, r)
            ww[with_w & (ww == 0)] = F32(1)
            ww[without_w] = F32(0)
        recv2d[s] = np.bincount(np.clip(t, 0, ntag - 1)[good] // batch, minlength=n_feats)
        recv2d[s, n_feats - 1] += int((~good).sum())
        k = min(n, cap)
        rows[s, :k], tag[s, :k], w[s, :k] = r[:k], t[:k], ww[:k]
    ib = SimpleNamespace(world=world, n_feats=n_feats, batch=batch, cap=cap, dim=dim, ntag=ntag, table_rows=list(table_rows),
                         feat_table=list(feat_table), rows=rows.reshape(-1), tag=tag.reshape(-1), w=w.reshape(-1), recv2d=recv2d)
    ib.total = np.minimum(recv2d.sum(1), cap)
    ib.run = mark_runs(ib.tag, recv2d, world, cap, ntag)
    return ib


def inbox_from_arrays(world, n_feats, batch, cap, dim, table_rows, feat_table, rows, tag, w, recv2d):
    """An inbox from arrays that exist already (a routed batch)."""
    ib = SimpleNamespace(world=world, n_feats=n_feats, batch=batch, cap=cap, dim=dim, ntag=n_feats * batch, table_rows=list(table_rows),
                         feat_table=list(feat_table), rows=np.asarray(rows).astype(np.int32), tag=np.asarray(tag).astype(np.int32),
                         w=np.asarray(w, F32), recv2d=np.asarray(recv2d, np.int64).reshape(world, n_feats))
    ib.total = np.minimum(ib.recv2d.sum(1), cap)
    ib.run = mark_runs(ib.tag, ib.recv2d, world, cap, ib.ntag)
    return ib


def entries(ib):
    """Per slot e = s * cap + j: source s, inside the count, tag in range, the entry's table, row inside that table."""
    s = np.repeat(np.arange(ib.world), ib.cap)
    j = np.tile(np.arange(ib.cap), ib.world)
    counted = j < ib.total[s]
    t = ib.tag.astype(np.int64)
    tag_ok = counted & (t >= 0) & (t < ib.ntag)
    tix = np.where(tag_ok, np.asarray(ib.feat_table, np.int64)[np.clip(t, 0, ib.ntag - 1) // ib.batch], 0)
    row = ib.rows.astype(np.int64)
    row_ok = (row >= 0) & (row < np.asarray(ib.table_rows, np.int64)[tix])
    return SimpleNamespace(s=s, j=j, counted=counted, tag_ok=tag_ok, tix=tix, row=row, row_ok=row_ok, tag=t)


def inbox_facts(ib):
    """What an inbox reaches, by name."""
    e = entries(ib)
    ln = (ib.run[..., 1] - ib.run[..., 0]).reshape(-1)
    w_nz = np.nan_to_num(ib.w, nan=1.0) != 0
    return {
        "empty block": bool((ib.recv2d.sum(1) == 0).any()),
        "clipped block": bool((ib.recv2d.sum(1) > ib.cap).any()),
        "row out of range with weight": bool((e.tag_ok & ~e.row_ok & w_nz).any()),
        "row out of range without weight": bool((e.tag_ok & ~e.row_ok & ~w_nz).any()),
        "tag out of range": bool((e.counted & ~e.tag_ok).any()),
        "run of rows out of range only": bool(any(ib.run[s, t, 1] - ib.run[s, t, 0] >= 2
                                                  and not e.row_ok[s * ib.cap + ib.run[s, t, 0]:s * ib.cap + ib.run[s, t, 1]].any()
                                                  for s in range(ib.world) for t in range(ib.ntag))) if ib.ntag <= 4096 else False,
        "run classes": {run_class(int(n)) for n in np.unique(ln)},
        "hot row hits": int((e.tag_ok & (e.tix == HOT[0]) & (e.row == HOT[1])).sum()),
    }


@functools.lru_cache(maxsize=None)
def case_inbox(dim, key):
    for i, (k, world, n_feats, batch, opt) in enumerate(inbox_cases(dim)):
        if k == key:
            return build_inbox(i, world, n_feats, batch, 5, dim, TABLE_ROWS, feat_table_of(n_feats), RUN_MENU, **opt)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def case_tables(dim):
    """The two tables of a dim (row 0 is data here) and the upstream gradient's generator seed."""
    rng = np.random.default_rng([32, dim])
    return tuple(rng.standard_normal((r, dim)).astype(F32) for r in TABLE_ROWS)


def case_g_partial(ib):
    return np.random.default_rng([33, ib.dim, ib.world, ib.ntag]).standard_normal((ib.world, ib.ntag, ib.dim)).astype(F32)


def bf16_tables(dim):
    """uint16 bit patterns, all finite: table 0 with exponents within 2^+-20 of one, table 1 with one row in eight drawn from every finite
    pattern (zeros, subnormals and the largest magnitudes included).  Returns (patterns, the same values widened to float32)."""
    rng = np.random.default_rng([34, dim])
    out = []
    for i, r in enumerate(TABLE_ROWS):
        sign = rng.integers(0, 2, (r, dim)).astype(np.uint16) << 15
        man = rng.integers(0, 128, (r, dim)).astype(np.uint16)
        ex = rng.integers(107, 148, (r, dim)).astype(np.uint16)
        if i == 1:
            wild = (rng.random(r) < 0.125)[:, None]
            ex = np.where(wild, rng.integers(0, 255, (r, dim)).astype(np.uint16), ex)
        out.append((sign | (ex << 7) | man).astype(np.uint16))
    wide = [(b.astype(np.uint32) << 16).view(F32) for b in out]
    assert all(np.isfinite(x).all() for x in wide)
    return out, wide


# ------------------------------------------------------------------------------------------------- forward
def _pool_fwd(ib, tables, dtype):
    out = np.zeros((ib.world, ib.ntag, ib.dim), dtype)
    scale = np.zeros((ib.world, ib.ntag, ib.dim), np.float64)
    lo, hi = ib.run[..., 0].astype(np.int64), ib.run[..., 1].astype(np.int64)
    ss, tt = np.nonzero(hi > lo)
    l, h = lo[ss, tt], hi[ss, tt]
    tixs = np.asarray(ib.feat_table, np.int64)[tt // ib.batch]
    for k in range(int((h - l).max()) if l.size else 0):
        m = l + k < h
        s_, t_, x_ = ss[m], tt[m], tixs[m]
        e = s_ * ib.cap + l[m] + k
        row, w = ib.rows[e].astype(np.int64), ib.w[e]
        for x, table in enumerate(tables):
            sel = (x_ == x) & (row >= 0) & (row < table.shape[0])
            if not sel.any():
                continue
            term = table[row[sel]].astype(dtype) * w[sel].astype(dtype)[:, None]          # float32: rounded once, then added
            out[s_[sel], t_[sel]] = out[s_[sel], t_[sel]] + term
            if dtype is np.float64:
                scale[s_[sel], t_[sel]] += np.abs(term)
    return out, scale


def pool_fwd32(ib, tables):
    """pool_inbox_fwd_kernel: partial[s, tag] = sum over the run's entries, in entry order, of fp32(row * w), from +0.f; a row outside its table
    adds nothing; a tag without a run gives zeros."""
    return _pool_fwd(ib, tables, F32)[0]


def pool_fwd64(ib, tables):
    """The same sums in float64, sum |w row| per element, and the run length n [world, ntag]: |kernel - this| <= gamma(n) * scale."""
    out, scale = _pool_fwd(ib, tables, np.float64)
    return out, scale, (ib.run[..., 1] - ib.run[..., 0]).astype(np.int64)


def oob_reports(ib):
    """What nrx_report_oob may leave in status[1:4]: (table, slot e, row) of every entry of a run whose row lies outside its table and whose
    weight is not zero -- status[0] counts them, the first to arrive writes its own triple."""
    e = entries(ib)
    hit = np.flatnonzero(e.tag_ok & ~e.row_ok & (np.nan_to_num(ib.w, nan=1.0) != 0))
    return [(int(e.tix[i]), int(i), int(np.int32(e.row[i]))) for i in hit]


# ------------------------------------------------------------------------------------------------- backward
def live_entries(ib, skip_row0, table_rows=None):
    """Entries that reach a table row: inside the count, tag in range, row inside the table (table_rows: the ONE row count the single-table
    launches take for every feature), not row 0 under skip_row0."""
    e = entries(ib)
    row_ok = e.row_ok if table_rows is None else (e.row >= 0) & (e.row < table_rows)
    return e, e.tag_ok & row_ok & ~((e.row == 0) & bool(skip_row0))


def pool_bwd64(ib, g_partial, skip_row0):
    """Dense form: grad_table[tix][row] += w * g_partial[s][tag] over the live entries, in float64.  Per table: (grad, number of terms n per row,
    sum |w g| per element, fp32(w g) of the row's only entry where n == 1).  Any order of n float32 atomic adds of fp32(w g) from 0 stays inside
    gamma(n + 1) * sum |w g| (one rounding per product, at most n - 1 inexact adds)."""
    e, live = live_entries(ib, skip_row0)
    out = []
    for x, nrows in enumerate(ib.table_rows):
        i = np.flatnonzero(live & (e.tix == x))
        g = g_partial[e.s[i], e.tag[i]]
        term = ib.w[i].astype(np.float64)[:, None] * g.astype(np.float64)
        grad, scale = np.zeros((nrows, ib.dim)), np.zeros((nrows, ib.dim))
        np.add.at(grad, e.row[i], term)
        np.add.at(scale, e.row[i], np.abs(term))
        n = np.bincount(e.row[i], minlength=nrows)
        single = np.zeros((nrows, ib.dim), F32)
        one = n[e.row[i]] == 1
        single[e.row[i][one]] = (g[one] * ib.w[i][one][:, None]).astype(F32) + F32(0)
        out.append((grad, n, scale, single))
    return out


def pool_expand(ib, table_rows, skip_row0, g_partial=None):
    """nrx_pool_inbox_expand: owner_ids[e] = row + 1 for a live entry, else 0; g_rows[e] = fp32(w g_partial[s][tag]) for the live entries
    (NaN here where the kernel writes nothing)."""
    e, live = live_entries(ib, skip_row0, table_rows)
    ids = np.where(live, e.row + 1, 0).astype(np.int32)
    g_rows = None
    if g_partial is not None:
        g_rows = np.full((ib.world * ib.cap, ib.dim), np.nan, F32)
        i = np.flatnonzero(live)
        g_rows[i] = (g_partial[e.s[i], e.tag[i]] * ib.w[i][:, None]).astype(F32)
    return ids, live, g_rows


def pool_payload(ib, table_rows, skip_row0):
    """nrx_pool_inbox_owner_ids' payload: s * n_feats * batch + tag for a live entry, else 0."""
    e, live = live_entries(ib, skip_row0, table_rows)
    return np.where(live, e.s * ib.ntag + e.tag, 0).astype(np.uint32)


def runs_words(ib, table_rows, skip_row0):
    """nrx_pool_inbox_runs_words on the inbox's run bounds: (tag_out, oid_out, payload_out) with -1 (all bits set) where the launch writes nothing
    -- tag_out outside the runs; oid / payload on the entries inside a block's count that lie in no run (their tag was out of range: the runs
    form, whose bounds come from the source, has no such entry)."""
    e, live = live_entries(ib, skip_row0, table_rows)
    in_run = e.tag_ok
    tag_out = np.where(in_run, e.tag, -1).astype(np.int32)
    oid = np.where(~e.counted, 0, np.where(in_run, np.where(live, e.row + 1, 0), -1)).astype(np.int32)
    pay = np.where(~e.counted, 0, np.where(in_run, np.where(live, e.s * ib.ntag + e.tag, 0), -1)).astype(np.int64).astype(np.uint32)
    return tag_out, oid, pay


def order_remap(order, n_entries, tag, cap, n_tags, world):
    """nrx_pool_order_remap: entry e = s * cap + j -> row s * n_tags + tag[e] of the block of sample gradients (tag outside [0, n_tags): 0 in
    its place); an e outside [0, n_entries) and a row at or past world * n_tags give 0."""
    e = np.asarray(order, np.int64)
    ok = (e >= 0) & (e < n_entries)
    t = np.asarray(tag, np.int64)[np.where(ok, e, 0)]
    r = np.where(ok, (e // cap) * n_tags + np.where((t >= 0) & (t < n_tags), t, 0), 0)
    return np.where(r < world * n_tags, r, 0).astype(np.int64)


# ------------------------------------------------------------------------------------------------- norm weights
NORM_LS = [1, AHEAD - 1, AHEAD, AHEAD + 1, 50, 64, 65, 128, 130]
NORM_KINDS = ["masked_mean", "mean", "sum"]
NARROW_MAX_L = 64


def norm_pb(L):
    """Samples per block: 16 lanes per sample up to 64 entries, a wavefront per sample beyond."""
    return NRX_BLOCK // (16 if L <= NARROW_MAX_L else 64)


def norm_batches(L):
    pb = norm_pb(L)
    return [1, pb - 1, pb, pb + 1, 3 * pb + 5]


def norm_masks(B, L):
    """A binary mask [B, L] (row 0 empty, row 1 full, the others a random subset) and a weighted one, (0, 1] * binary."""
    rng = np.random.default_rng([35, B, L])
    n = rng.integers(0, L + 1, B)
    n[0] = 0
    if B > 1:
        n[1] = L
    rank = rng.random((B, L)).argsort(axis=1).argsort(axis=1)
    binary = (rank < n[:, None]).astype(F32)
    weighted = ((1.0 - rng.random((B, L))).astype(F32) * binary).astype(F32)
    return binary, weighted


def norm_weights32(mask, B, L, kind):
    """bag_norm_weights_kernel where every sum is exact (0 / 1 masks, no mask): out = fp32(m / den), inv = fp32(1 / den), 0 for an empty masked
    bag; den = fp32(count + 1e-8f) | float(L) | 1."""
    m = np.ones((B, L), F32) if (mask is None or kind == "mean") else np.asarray(mask, F32)
    if kind == "masked_mean":
        assert np.all((m == 0) | (m == 1)), "the restatement pins the bits for 0 / 1 masks only"
        den = (m.sum(1, dtype=np.float64).astype(F32) + EPS32).astype(F32)
        inv = np.where(den <= EPS32, F32(0), (F32(1) / den).astype(F32)).astype(F32)
    else:
        den = np.full(B, F32(L) if kind == "mean" else F32(1), F32)
        inv = (F32(1) / den).astype(F32)
    return (m / den[:, None]).astype(F32), inv


def norm_weights64(mask, B, L):
    """Masked mean in float64: m / (sum m + 1e-8f), 1 / (sum m + 1e-8f).  The kernel's sum of L non-negative numbers has at most L - 1 inexact
    adds in any order, then + 1e-8f and the division: L + 1 roundings, gamma(L + 2) |ref| with the second-order terms."""
    m = np.asarray(mask, np.float64)
    den = m.sum(1) + np.float64(EPS32)
    return m / den[:, None], 1.0 / den


# ------------------------------------------------------------------------------------------------- the element-wise launches
UPSTREAM_GRID_CAP, KEYS_GRID_CAP, OWNER_IDS_GRID_CAP, RUNS_WORDS_GRID_CAP, REMAP_GRID_CAP = 4096, 4096, 2048, 8192, 8192
# (dim, batch, col, ld - col - dim, copies, copy_stride - batch * dim, scale)
UPSTREAM_CASES = [(d, b, col, pad, copies, gap, sc)
                  for d in (1, 16, 257) for b, col, pad, copies, gap, sc in ((1, 3, 2, 1, 0, True), (37, 5, 3, 3, 7, True), (37, 1, 1, 3, 1, False))]
UPSTREAM_WRAP = (16, UPSTREAM_GRID_CAP * NRX_BLOCK // 16 + 1, 5, 3, 1, 0, True)      # batch * dim = 4096 * 256 + 16


def upstream_inputs(dim, batch, col, pad):
    rng = np.random.default_rng([36, dim, batch, col])
    return rng.standard_normal((batch, col + dim + pad)).astype(F32), rng.standard_normal(batch).astype(F32)


def upstream_rows(g_out, col, dim, scale, copies):
    """nrx_bag_upstream_rows: dst[c][b][k] = fp32(g_out[b][col + k] * scale[b]), a plain copy without scale -> [copies, batch, dim]."""
    v = g_out[:, col:col + dim]
    if scale is not None:
        v = (v * scale[:, None]).astype(F32)
    return np.broadcast_to(v[None], (copies,) + v.shape).copy()


def table_keys(ids, table_of):
    """nrx_make_table_keys: keys[p] = (table_of[f] << 40) | id over the features' ids laid end to end; a negative id is row 0."""
    parts = [(np.int64(t) << 40) | (np.maximum(np.asarray(x, np.int64), 0) & ((1 << 40) - 1)) for x, t in zip(ids, table_of)]
    return np.concatenate(parts).astype(np.int64)


def keys_inputs(bits, lens):
    rng = np.random.default_rng([37, bits] + list(lens))
    hi = I32MAX if bits == 32 else (1 << 40) - 1
    dt = np.int32 if bits == 32 else np.int64
    ids = []
    for n in lens:
        x = rng.integers(0, hi, n, dtype=np.int64)
        x[rng.random(n) < 0.05] = -rng.integers(1, 1000)
        if n:
            x[0], x[-1] = hi, -1
        ids.append(x.astype(dt))
    return ids


KEYS_TABLE_OF = [5, 0, 5]                                                            # 3 features on 2 tables
KEYS_LENS_SMALL = [300, 0, 77]
KEYS_LENS_WRAP = [70001, 0, KEYS_GRID_CAP * NRX_BLOCK - 70001 + 300]                 # total = 4096 * 256 + 300
