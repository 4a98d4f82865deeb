"""The fixed-capacity exchange of single-valued ids (csrc/nrx_route.hip: route_hist / route_scan / route_place / route_single on the source,
inbox_kernel and inbox_gather_ring_kernel on the owner) in numpy, three times over:
  * DEFINITIONS of the results as include/nrx_embed.h states them (route_def, slot_features / gather_index, place_index, scatter_def);
  * the LAUNCH ARITHMETIC restated from the source (chunks, scan steps, lane-group widths, tiles, work items, which form a gather takes);
  * MODELS of each kernel's decomposition (per-chunk histogram -> stepped scan with carry -> cell prefixes -> ballot rank; per-source prefix
    search; the classic tiles; the ring's persistent walk with its resolve pass), with switches that plant one mistake each.
The case lists at the end are computed from the arithmetic: the smallest shapes that reach each edge.  tests/test_route_inbox_ref.py holds this
file to oracle/ref_np.py and shows the lists have teeth; tests/test_route_inbox_kernels_gpu.py holds the kernels to the definitions.
numpy only."""
from types import SimpleNamespace

import numpy as np

I32MAX = (1 << 31) - 1
CHUNK = 2048                    # ids per route block, of ONE feature
NRX_BLOCK = 256
SCAN_STEP = 256                 # chunks a wavefront scans per step (64 lanes x 4)
SCAN_WAVES = NRX_BLOCK // 64    # owners o, o + 4, ... per wavefront
CELL = 64                       # ids per (round, wavefront) cell of a chunk: position order IS cell order
INBOX_R, INBOX_NC = 8, 4
RING_MIN_ITEMS = 512            # launch_inbox<false>: fewer work items -> the classic kernel
RING_GRID = 256 * 6             # persistent grid of the ring form
MAX_FEATURES = 64
GARBAGE = 10 ** 9               # what the slots past a block's count hold (rows and positions)
UNRESOLVED = -2                 # ring model: a slot walked whose LDS word no resolve pass of this block wrote
STALE = -3                      # ring model: ... or whose word an EARLIER work item of the block wrote


# ------------------------------------------------------------------------------------------------- launch arithmetic
def cdiv(a, b):
    return -(-a // b)


def chunk0(lens):
    """First chunk of every feature, and the chunk count behind the last (features without ids own no chunk)."""
    return np.concatenate([[0], np.cumsum([cdiv(int(n), CHUNK) for n in lens])]).astype(np.int64)


def nchunks(lens):
    return int(chunk0(lens)[-1])


def scan_steps(lens):
    return cdiv(nchunks(lens), SCAN_STEP)


def scan_trips(world):
    return cdiv(world, SCAN_WAVES)


def route_workspace(n_total, world):
    """nrx_route_workspace: int64 units for the int32 histogram [world][chunks], every feature ending in a partial chunk."""
    if n_total < 0 or world < 1:
        return -1
    return ((cdiv(n_total, CHUNK) + MAX_FEATURES) * world + 1) // 2 + 1


def ql(dim):
    q = cdiv(dim, 4)
    l = 0
    while (1 << l) < q:
        l += 1
    return min(6, l)


def tb(dim):
    return NRX_BLOCK >> ql(dim)


def k0_trips(dim):
    return cdiv(dim, 4 << ql(dim))


def classic_tile(dim):
    return INBOX_R * tb(dim)


def classic_grid(dim, cap, world):
    return cdiv(cap, classic_tile(dim)), world


def ring_item(dim):
    return INBOX_R * INBOX_NC * tb(dim)


def cps(dim, cap):
    return cdiv(cap, ring_item(dim))


def form(dim, cap, world, scatter=False):
    if not scatter and dim % 4 == 0 and dim <= 256 and ql(dim) >= 2 and cps(dim, cap) * world >= RING_MIN_ITEMS:
        return "ring"
    return "classic"


def ring_grid(dim, cap, world):
    return min(cps(dim, cap) * world, RING_GRID)


def place_shape_ok(dim, out_ld, feat_col):
    return dim % 4 == 0 and 16 <= dim <= 256 and out_ld % 4 == 0 and all(c >= 0 and c % 4 == 0 and c + dim <= out_ld for c in feat_col)


def resolve_trips(dim, parent=False):
    """Positions of a work item the ring's resolve pass covers: all NS * TB of them; the parent counted whole trips of the block."""
    n = ring_item(dim)
    return (n // NRX_BLOCK) * NRX_BLOCK if parent else n


# ------------------------------------------------------------------------------------------------- routing: definition
def _flatten(id_arrays):
    flat = [np.asarray(a).reshape(-1).astype(np.int64) for a in id_arrays]
    ids = np.concatenate(flat) if flat else np.zeros(0, np.int64)
    fid = np.repeat(np.arange(len(flat)), [a.size for a in flat])
    within = np.concatenate([np.arange(a.size) for a in flat]) if flat else ids
    return ids, fid, within


def split_ids(ids, world):
    lo, hi = ids < 0, ids > I32MAX
    owner = np.where(lo | hi, 0, ids % world)
    local = np.where(lo, -1, np.where(hi, I32MAX, ids // world))
    return owner, local


def route_def(id_arrays, world, cap, fill):
    """nrx_route_ids_pos as the header states it.  send_rows / send_pos [world * cap] int32 (`fill` where nothing is written: the slots past a
    block's count), slot [N] int32, counts2d [world, F] int64, the largest block count."""
    ids, fid, within = _flatten(id_arrays)
    F = len(id_arrays)
    owner, local = split_ids(ids, world)
    order = np.argsort(owner, kind="stable")
    per_owner = np.bincount(owner, minlength=world)
    start = np.cumsum(per_owner) - per_owner
    k = np.empty(ids.size, np.int64)
    k[order] = np.arange(ids.size) - start[owner[order]]
    ok = k < cap
    slot = np.where(ok, owner * cap + k, -1).astype(np.int32)
    send_rows, send_pos = np.full(world * cap, fill, np.int32), np.full(world * cap, fill, np.int32)
    send_rows[slot[ok]] = local[ok]
    send_pos[slot[ok]] = within[ok]
    counts2d = np.bincount(owner * F + fid, minlength=world * F).reshape(world, F).astype(np.int64)
    return SimpleNamespace(send_rows=send_rows, send_pos=send_pos, slot=slot, counts2d=counts2d, worst=int(per_owner.max()) if ids.size else 0)


# ------------------------------------------------------------------------------------------------- routing: the kernels' order
def scan_model(h, carry="ok"):
    """route_scan for one owner: exclusive scan of hist[o][:] in steps of 256 chunks; `running` carries the steps before.  carry = "none":
    every step starts from 0; "short": what is carried on misses the step's last chunk (the owner's total, taken at the end, is right in both)."""
    out, running = np.zeros_like(h), 0
    for c0 in range(0, h.size, SCAN_STEP):
        seg = h[c0:c0 + SCAN_STEP]
        out[c0:c0 + SCAN_STEP] = (0 if carry == "none" else running) + np.cumsum(seg) - seg
        running += int(seg[:-1].sum() if carry == "short" and c0 + SCAN_STEP < h.size else seg.sum())
    return out, int(h.sum())


def route_model(id_arrays, world, cap, fill, carry="ok"):
    """The three launches' decomposition: rank of an id inside its owner block = scanned chunk histogram + prefix of the chunk's 32 cells +
    lanes below it in its cell.  world == 1 is route_single: one narrowing pass in source order."""
    lens = [int(np.asarray(a).size) for a in id_arrays]
    F, c0s, nch = len(lens), chunk0(lens), nchunks(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    N = int(off[-1])
    send_rows, send_pos = np.full(world * cap, fill, np.int32), np.full(world * cap, fill, np.int32)
    slot = np.full(N, fill, np.int32)
    if world == 1:
        ids, _, within = _flatten(id_arrays)
        _, local = split_ids(ids, 1)
        p = np.arange(N)
        ok = p < cap
        slot[:] = np.where(ok, p, -1)
        send_rows[p[ok]], send_pos[p[ok]] = local[ok], within[ok]
        return SimpleNamespace(send_rows=send_rows, send_pos=send_pos, slot=slot, counts2d=np.asarray([lens], np.int64), worst=N)
    owner_c = np.full((nch, CHUNK), -1, np.int64)          # [chunk][position in chunk]; -1 past a feature's end
    local_c = np.zeros((nch, CHUNK), np.int64)
    within_c = np.zeros((nch, CHUNK), np.int64)
    flatp_c = np.full((nch, CHUNK), -1, np.int64)
    for f, a in enumerate(id_arrays):
        a = np.asarray(a).reshape(-1).astype(np.int64)
        if not a.size:
            continue
        o, l = split_ids(a, world)
        c, n = int(c0s[f]), cdiv(a.size, CHUNK)
        for dst, src in ((owner_c, o), (local_c, l), (within_c, np.arange(a.size)), (flatp_c, off[f] + np.arange(a.size))):
            dst[c:c + n].reshape(-1)[:a.size] = src
    counts2d = np.zeros((world, F), np.int64)
    worst = 0
    for o in range(world):
        m = (owner_c == o).reshape(nch, CHUNK // CELL, CELL)
        cell = m.sum(2)
        lane_rank = np.cumsum(m, 2) - m
        cell_pre = np.cumsum(cell, 1) - cell
        excl, running = scan_model(cell.sum(1), carry)
        at = lambda c: excl[c] if c < nch else running
        counts2d[o] = [at(int(c0s[f + 1])) - at(int(c0s[f])) for f in range(F)]
        worst = max(worst, running)
        k = (excl[:, None, None] + cell_pre[:, :, None] + lane_rank)[m]
        p, ok = flatp_c.reshape(m.shape)[m], k < cap
        slot[p] = np.where(ok, o * cap + k, -1)
        send_rows[(o * cap + k)[ok]] = local_c.reshape(m.shape)[m][ok]
        send_pos[(o * cap + k)[ok]] = within_c.reshape(m.shape)[m][ok]
    return SimpleNamespace(send_rows=send_rows, send_pos=send_pos, slot=slot, counts2d=counts2d, worst=worst)


def same_route(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("send_rows", "send_pos", "slot", "counts2d")) and a.worst == b.worst


# ------------------------------------------------------------------------------------------------- inbox: generator
def make_inbox(world, cap, counts, table_rows, feat_table, seed, out_rows=0, bad=True, garbage_row=GARBAGE):
    """An owner's inbox with the given counts per (source, feature) (a source's sum may pass cap: the block is clipped).  Live slots hold
    rows of their feature's table -- every 29th a row that is none (-1, rows, INT32_MAX) when `bad` -- and, with out_rows > 0, positions that are
    distinct inside a (source, feature) -- every 31st one outside [0, out_rows) (-1, out_rows, INT32_MAX).  The other slots hold garbage."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64).reshape(world, -1)
    ib = SimpleNamespace(world=world, cap=cap, n_feats=counts.shape[1], recv2d=counts, table_rows=list(table_rows), feat_table=list(feat_table),
                         out_rows=out_rows, rows=np.full(world * cap, garbage_row, np.int32), pos=np.full(world * cap, GARBAGE, np.int32))
    flat, feat = slot_features(ib)
    nrows = np.asarray(table_rows, np.int64)[np.asarray(feat_table)[feat]]
    rows = (rng.random(flat.size) * nrows).astype(np.int64)
    n = np.arange(flat.size)
    if bad:
        hit = n % 29 == 7
        rows[hit] = np.choose(n[hit] // 29 % 3, [-1, nrows[hit], I32MAX])
    ib.rows[flat] = rows
    if out_rows:
        pos = np.zeros(flat.size, np.int64)
        key = (flat // cap) * ib.n_feats + feat
        for k in np.unique(key):
            sel = key == k
            assert sel.sum() <= out_rows, "more ids of one (source, feature) than samples"
            pos[sel] = rng.permutation(out_rows)[:sel.sum()]
        if bad:
            hit = n % 31 == 11
            pos[hit] = np.choose(n[hit] // 31 % 3, [-1, out_rows, I32MAX])
        ib.pos[flat] = pos
    return ib


# ------------------------------------------------------------------------------------------------- inbox: definitions
def totals(ib):
    return np.minimum(ib.recv2d.sum(1), ib.cap)


def slot_features(ib):
    """(flat slot s * cap + j, feature) of every slot in a block's valid prefix min(sum_f recv2d[s, f], cap): features lie behind each other."""
    flat, feat = [], []
    for s in range(ib.world):
        f = np.repeat(np.arange(ib.n_feats), ib.recv2d[s])[:ib.cap]
        flat.append(s * ib.cap + np.arange(f.size))
        feat.append(f)
    return np.concatenate(flat), np.concatenate(feat)


def gather_index(ib):
    """Definition of nrx_gather_inbox as index arrays: slot `flat` receives row `row` of table `tab` (row 0 where the inbox names none: `bad`,
    counted in status[0]).  reports: the (table, slot, row) triples status[1..3] may hold."""
    flat, feat = slot_features(ib)
    tab = np.asarray(ib.feat_table)[feat]
    raw = ib.rows[flat].astype(np.int64)
    bad = (raw < 0) | (raw >= np.asarray(ib.table_rows, np.int64)[tab])
    reports = {(int(t), int(np.int32(p)), int(r)) for t, p, r in zip(tab[bad], flat[bad], raw[bad])}
    return SimpleNamespace(flat=flat, feat=feat, tab=tab, row=np.where(bad, 0, raw), bad=bad, reports=reports)


def place_index(ib):
    """Definition of nrx_gather_inbox_place: gather_index, and slot `flat` goes to row `at` of source flat // cap's buffer unless `at` lies outside
    [0, out_rows) (`dropped`: counted and reported too, with the position in the place of the row)."""
    g = gather_index(ib)
    at = ib.pos[g.flat].astype(np.int64)
    g.dropped = (at < 0) | (at >= ib.out_rows)
    g.at, g.src = at, g.flat // ib.cap
    g.reports |= {(int(t), int(np.int32(p)), int(a)) for t, p, a in zip(g.tab[g.dropped], g.flat[g.dropped], at[g.dropped])}
    g.n_reports = int(g.bad.sum() + g.dropped.sum())
    return g


def gather_def(ib, tables, dim, fill=np.nan):
    g = gather_index(ib)
    out = np.full((ib.world * ib.cap, dim), fill, np.float32)
    for t, T in enumerate(tables):
        sel = g.tab == t
        out[g.flat[sel]] = T[g.row[sel]]
    return out


def scatter_def(ib, g_rows, grads, skip_row0):
    """Definition of nrx_scatter_add_inbox in int64: grads[table][row] += g_rows[slot] over the valid prefixes; rows that are none are dropped
    silently, local row 0 is skipped iff skip_row0.  Returns (tables, per-row sum of |terms| including what the table held)."""
    g = gather_index(ib)
    keep = ~g.bad & ~((g.row == 0) & bool(skip_row0))
    out = [np.asarray(t).astype(np.int64) for t in grads]
    mag = [np.abs(t) for t in out]
    gi = np.asarray(g_rows).astype(np.int64)
    for t in range(len(out)):
        sel = keep & (g.tab == t)
        np.add.at(out[t], g.row[sel], gi[g.flat[sel]])
        np.add.at(mag[t], g.row[sel], np.abs(gi[g.flat[sel]]))
    return out, mag


# ------------------------------------------------------------------------------------------------- inbox: the kernels' order
def prefix_of(ib, s):
    return np.concatenate([[0], np.cumsum(ib.recv2d[s])])


def prefix_search(pre, j, strict=False):
    """The kernels' search: the last f with pre[f] <= j (zero-count features share a prefix with their successor and lose).  strict: `<`."""
    j = np.asarray(j, np.int64)
    lo, hi = np.zeros(j.shape, np.int64), np.full(j.shape, pre.size - 1, np.int64)
    while (hi - lo > 1).any():
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        le = pre[mid] < j if strict else pre[mid] <= j
        lo, hi = np.where(act & le, mid, lo), np.where(act & ~le, mid, hi)
    return lo


def classic_model(ib, dim, clamp=True, strict=False, floor_grid=False):
    """inbox_kernel: blocks (tile, source) of 8 tb slots; a thread leaves when its first slot is past the total.  Returns (flat, feature) sorted by
    flat.  clamp=False: the total is not held to cap; floor_grid: the grid misses the partial last tile."""
    T = classic_tile(dim)
    gx = ib.cap // T if floor_grid else cdiv(ib.cap, T)
    flat, feat = [], []
    for s in range(ib.world):
        pre = prefix_of(ib, s)
        total = min(int(pre[-1]), ib.cap) if clamp else int(pre[-1])
        j = np.arange(min(total, gx * T))
        flat.append(s * ib.cap + j)
        feat.append(prefix_search(pre, j, strict))
    return np.concatenate(flat), np.concatenate(feat)


def ring_model(ib, dim, place=False, parent_trips=False, rebuild=True, strict=False):
    """inbox_gather_ring_kernel: a persistent grid of blocks, each walking work items (source, chunk of 32 tb slots) work = block, block + grid,
    ...; the feature prefix in LDS is rebuilt when the source changes; an item's slots are resolved into LDS (resolve_trips positions), then
    walked.  Returns (flat, feature) sorted by flat, feature = UNRESOLVED / STALE where the walk reads a word this item's resolve pass did not
    write, and the facts of the walk.  parent_trips: the trip count NS * TB // 256 of the parent commit; rebuild=False: the prefix of the block's
    first source is kept."""
    I, c = ring_item(dim), cps(dim, ib.cap)
    nwork = ib.world * c
    grid = min(nwork, RING_GRID) if place else ring_grid(dim, ib.cap, ib.world)
    covered = resolve_trips(dim, parent_trips)
    flat, feat = [], []
    facts = SimpleNamespace(grid=grid, nwork=nwork, skipped=0, switches_live=0, past_wrap_live=0, unresolved=0)
    for b in range(grid):
        s_cur, pre, lds, served = -1, None, np.full(I, UNRESOLVED, np.int64), 0
        for work in range(b, nwork, grid):
            s, chunk = divmod(work, c)
            if s != s_cur and (rebuild or s_cur < 0):
                pre = prefix_of(ib, s)
            switched, s_cur = s_cur >= 0 and s != s_cur, s
            total = min(int(pre[-1]), ib.cap)
            base = chunk * I
            if base >= total:
                facts.skipped += 1
                continue
            pos = np.arange(I)
            j = base + pos
            lds = np.where(lds == UNRESOLVED, UNRESOLVED, STALE)
            res = pos < covered
            lds[res] = np.where(j[res] < total, prefix_search(pre, j[res], strict), -1)
            live = j < total
            flat.append(s * ib.cap + j[live])
            feat.append(lds[live])
            facts.unresolved += int((lds[live] < 0).sum())
            facts.switches_live += int(switched and served > 0)
            facts.past_wrap_live += int(work >= grid)
            served += 1
    flat, feat = np.concatenate(flat), np.concatenate(feat)
    order = np.argsort(flat, kind="stable")
    return flat[order], feat[order], facts


# ------------------------------------------------------------------------------------------------- case lists: routing
FEATURE_LENS = [0, 1, 2047, 2048, 2049]
BAD_IDS_64 = [-1, -(1 << 63), 1 << 31, I32MAX, 1 << 40, (1 << 63) - 1]
BAD_IDS_32 = [-1, -(1 << 31), I32MAX]


def route_cases():
    """name -> world, lens, index bits and what is special.  cap: None = the largest block count + 3 (every block keeps unused slots);
    "over1": that count - 1 (one owner overflows by exactly 1)."""
    edge = [0, 0, 1, 2047, 0, 2048, 2049, 0, 0]                  # empty features leading, between and trailing
    c = {
        "w1-edges": dict(world=1, lens=edge, bits=64, bad=True),
        "w1-over": dict(world=1, lens=[5, 0, 2049], bits=32, cap=2050),
        "w2-edges": dict(world=2, lens=edge, bits=32, bad=True),
        "w5-edges": dict(world=5, lens=edge, bits=64, bad=True),
        "w64-edges": dict(world=64, lens=[1, 2049, 0, 4097], bits=64, bad=True),
        "w5-f64": dict(world=5, lens=[FEATURE_LENS[(3 * f + 1) % 5] for f in range(64)], bits=32),
        "w2-scan2": dict(world=2, lens=[SCAN_STEP * CHUNK + 1], bits=32),
        "w2-scan3": dict(world=2, lens=[2 * SCAN_STEP * CHUNK + 1], bits=32),
        "w5-scan3": dict(world=5, lens=[5, 2 * SCAN_STEP * CHUNK + 1, 0, 3], bits=32, bad=True),
        "w5-over1": dict(world=5, lens=[2049, 700], bits=64, cap="over1"),
        "w5-skew": dict(world=5, lens=[3000, 0, 41], bits=32, skew=3, cap=1000),
        "w2-view": dict(world=2, lens=[2049, 1], bits=32, view=1),
        "w3-view64": dict(world=3, lens=[700, 2048], bits=64, view=1),
    }
    return c


def route_case(name):
    """(id arrays in their index type, world, cap, view offset in elements)."""
    spec = route_cases()[name]
    rng = np.random.default_rng(sorted(route_cases()).index(name) + 700)
    world, dt = spec["world"], np.int64 if spec["bits"] == 64 else np.int32
    ids = []
    for n in spec["lens"]:
        a = rng.integers(0, 1 << 20, n).astype(np.int64)
        if "skew" in spec:
            a = a // world * world + spec["skew"]
        if spec.get("bad") and n >= 2047:
            bad = BAD_IDS_64 if spec["bits"] == 64 else BAD_IDS_32
            at = rng.choice(n, len(bad), replace=False)
            a[at] = bad
            a[[0, n - 1]] = bad[0], bad[-1]                          # first and last position of the feature
        ids.append(a.astype(dt))
    cap = spec.get("cap")
    if cap is None or cap == "over1":
        worst = route_def(ids, world, 1, 0).worst
        cap = worst + 3 if cap is None else worst - 1
    return ids, world, int(cap), spec.get("view", 0)


ROUTE_REFUSALS = ["world 0", "world 65", "cap 0", "cap * world = 2^31", "n_feats 0", "n_feats 65", "index_bits 16", "null send_rows", "null slot",
                  "negative length", "null ids with a length", "null send_pos"]


# ------------------------------------------------------------------------------------------------- case lists: inbox
CLASSIC_DIMS = [1, 3, 4, 5, 8, 12, 16, 17, 32, 64, 100, 101, 256, 257, 260, 300]     # (101, 257: the scalar path at ql 5 and 6)
RING_DIMS = [12, 16, 20, 32, 36, 64, 68, 128, 132, 256]           # per ql 2..6: idle lanes (dim < 4 Q) and every lane busy
PLACE_DIMS = [16, 20, 32, 36, 64, 68, 128, 132, 256]              # (the placing form documents 16..256)
WRAP_DIMS = [16, 132]
TABLE_ROWS = [53, 31]
WRAP_CPS = 25
WRAP_LIVE = [0, 23, 62, 63]


def count_menu(T, cap):
    return [0, 1, T - 1, T, T + 1, 3 * T + 5, cap + 9]


def _spread(total, feats, n_feats, seed):
    """`total` ids of one source over the live features `feats` (the others get 0), every live feature >= 1 where total allows."""
    rng = np.random.default_rng(seed)
    row = np.zeros(n_feats, np.int64)
    cut = np.sort(rng.integers(0, total + 1, len(feats) - 1))
    row[feats] = np.diff(np.concatenate([[0], cut, [total]]))
    return row


def classic_cases(dim):
    """name -> (world, cap, counts [world, F], feat_table).  cap = 3 tiles + 7: no multiple of the tile or the block."""
    T = classic_tile(dim)
    cap = 3 * T + 7
    menu = count_menu(T, cap)
    live64 = [3, 17, 18, 40, 63]
    return {
        "w1-f1": (1, cap, [[T + 1]], [0]),
        "w3-f3": (3, cap, [_spread(3 * T + 5, [0, 1, 2], 3, dim), [0, 0, 0], [T, cap - T, 9]], [1, 0, 1]),
        "w64-f64": (64, cap, [_spread(menu[s % 7], live64, 64, 64 * dim + s) for s in range(64)], [f % 2 for f in range(64)]),
    }


def classic_case(dim, name, out_rows=0, **kw):
    world, cap, counts, feat_table = classic_cases(dim)[name]
    return make_inbox(world, cap, counts, TABLE_ROWS, feat_table, 1000 * dim + world, out_rows, **kw)


def ring_case(dim, world=64, out_rows=0):
    """cap = 7 items + 1: cps = 8, so world 64 has exactly 512 work items (ring) and world 63 has 504 (classic).  The world 63 inbox is the first
    63 blocks of the world 64 one."""
    I = ring_item(dim)
    cap = 7 * I + 1
    menu = [0, 1, I - 1, I, I + 1, 3 * I + 5, cap, cap + 9, 2 * I]
    counts = [_spread(menu[s % 9], [0, 2], 3, 77 * dim + s) for s in range(64)]
    full = make_inbox(64, cap, counts, TABLE_ROWS, [1, 0, 1], 5000 + dim, out_rows)
    if world == 64:
        return full
    return SimpleNamespace(**{**vars(full), "world": world, "recv2d": full.recv2d[:world], "rows": full.rows[:world * cap], "pos": full.pos[:world * cap]})


def wrap_case(dim, out_rows=0):
    """World 64, cps 25: 1600 work items on 1536 blocks.  Live sources 0 (clipped: all 25 items), 23 (one item and a slot), 62 (one item exactly) and
    63 (three items and five slots, the first four of them past the wrap)."""
    I = ring_item(dim)
    cap = (WRAP_CPS - 1) * I + 1
    counts = np.zeros((64, 2), np.int64)
    counts[0], counts[23], counts[62], counts[63] = [cap - I, I + 3], [I - 1, 2], [1, I - 1], [2 * I, I + 5]
    return make_inbox(64, cap, counts, TABLE_ROWS, [1, 0], 9000 + dim, out_rows)


def place_cases(dim):
    """name -> (world, cap, counts, feat_table, out_rows, feat_col, out_ld).  One work item, two, and more items than one source has (3 sources of 2
    items: cps + 1 and beyond); columns in no order, a stride wider than the features."""
    I = ring_item(dim)
    cols, ld = [2 * dim + 4, 0, dim + 4], 3 * dim + 12
    return {
        "one-item": (1, I, [[I - 3, 0, 2]], [0, 1, 0], I, cols, ld),
        "two-items": (1, I + 1, [[5, I - 10, 9]], [1, 0, 1], I, cols, ld),
        "w3": (3, I + 1, [[I, 1, 7], [0, 0, 0], [3, I + 1, 0]], [1, 0, 1], I + 1, cols, ld),
    }


def place_case(dim, name):
    world, cap, counts, feat_table, out_rows, cols, ld = place_cases(dim)[name]
    ib = make_inbox(world, cap, counts, TABLE_ROWS, feat_table, 3000 + dim + world, out_rows)
    ib.feat_col, ib.out_ld = cols, ld
    return ib


INBOX_REFUSALS = ["world 0", "world 65", "cap 0", "n_feats 0", "n_feats 65", "feat_table out of range", "null table", "misaligned table",
                  "null recv2d", "null inbox"]
PLACE_REFUSALS = ["dim 8", "dim 18", "dim 260", "out_ld % 4", "feat_col % 4", "feat_col + dim > out_ld", "misaligned peer_out", "null peer_out"]
