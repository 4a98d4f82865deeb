"""Case lists, seeded operands and exact references for the kernels of csrc/nrx_intutil.hip that the sharded path and the data pipeline call:
nrx_gather_rows_segmented, nrx_scatter_add_rows_segmented, nrx_csr_to_padded, nrx_mask_lengths.  tests/test_intutil_cases.py (CPU) asserts that
the lists reach every launch-shape edge; tests/test_intutil_kernels_gpu.py drives the C entry points with them.

The launch shapes restated from the source: gather / scatter give a row Q = 2^ql lanes of 4 columns, ql = min(6, ceil_log2(ceil(dim / 4))), so a
block of 256 threads holds tb = 256 >> ql rows and past dim = 256 a lane loops again; the gather copies float4 only when dim % 4 == 0 and the output
and every table are 16-byte aligned.  csr_to_padded launches min(ceil(batch * bag_len / 256), 4096) blocks, mask_lengths min(ceil(batch / 256), 2048):
beyond that a stride loop runs."""
from collections import namedtuple

import numpy as np

SEED = 20240612
BLOCK = 256
MAX_SEG = 4096
MAX_TABLES = 64
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 260, 1000)
ALIGNS = ("aligned", "table-one-float-in", "rows-one-float-in")      # "rows" = the gather's output / the scatter's g_rows
G_MAX, INIT_MAX = 4, 8          # |g_rows| <= 4, |initial gradient| in 1..8: small integers, float32 atomics are exact in any order

SegCase = namedtuple("SegCase", "index name dim table_rows seg_table seg_len align bad one_row")


def ql_of(dim):
    q, l = (dim + 3) // 4, 0
    while (1 << l) < q:
        l += 1
    return min(l, 6)


def tb_of(dim):
    return BLOCK >> ql_of(dim)


def _layout(rng, n_rows, n_seg, n_tables, empty=()):
    """Segment lengths that sum to n_rows with the segments listed in `empty` (and no others by intent) of length 0."""
    live = [s for s in range(n_seg) if s not in set(empty)]
    seg_len = np.zeros(n_seg, np.int64)
    if n_rows:
        assert live
        cuts = np.sort(rng.integers(0, n_rows + 1, len(live) - 1))
        seg_len[live] = np.diff(np.concatenate([[0], cuts, [n_rows]]))
    seg_table = rng.integers(0, n_tables, n_seg).astype(np.int32)
    return seg_table, seg_len


def seg_cases():
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, dim, table_rows, seg_table, seg_len, align="aligned", bad=(), one_row=False):
        out.append(SegCase(len(out), name, dim, tuple(int(r) for r in table_rows), tuple(int(t) for t in seg_table), tuple(int(l) for l in seg_len),
                           align, tuple(bad), one_row))

    # every width at tb - 1, tb, tb + 1 rows: 5 segments over 3 tables, the second one empty
    for dim in WIDTHS:
        tb = tb_of(dim)
        for n_rows, tag in ((tb - 1, "tb-1"), (tb, "tb"), (tb + 1, "tb+1")):
            seg_table, seg_len = _layout(rng, n_rows, 5, 3, empty=(1,))
            add(f"dim{dim}-rows-{tag}={n_rows}", dim, (11, 1, 7), seg_table, seg_len)
    # the scalar path by alignment (dim % 4 == 0, so only the pointer decides), several blocks
    for dim in (4, 16, 64, 256, 260):
        for align in ALIGNS[1:]:
            seg_table, seg_len = _layout(rng, 3 * tb_of(dim) + 1, 4, 2)
            add(f"dim{dim}-{align}", dim, (9, 5), seg_table, seg_len, align=align)
    # segment counts
    seg_table, seg_len = _layout(rng, 700, 1, 1)
    add("n_seg-1", 8, (13,), seg_table, seg_len)
    first, middle, last = range(0, 5), range(2000, 2101), range(MAX_SEG - 7, MAX_SEG)
    seg_table, seg_len = _layout(rng, 9000, MAX_SEG, 3, empty=[*first, *middle, *last])
    add("n_seg-4096-empty-first-middle-run-last", 8, (17, 3, 40), seg_table, seg_len)
    seg_table, seg_len = _layout(rng, 5000, MAX_SEG, MAX_TABLES, empty=[*first, *middle, *last])
    add("n_seg-4096-64-tables-dim5", 5, tuple(rng.integers(1, 9, MAX_TABLES)), seg_table, seg_len)
    # rows that no table has: negative, == rows, far out, INT64 extremes; (position, value) pairs, positions spread over the blocks
    seg_table, seg_len = _layout(rng, 600, 6, 3, empty=(3,))
    bad = ((0, -1), (17, 1 << 40), (130, -(1 << 62)), (311, (1 << 63) - 1), (599, None))       # None: exactly the table's row count
    add("out-of-range-and-negative-rows-dim16", 16, (21, 4, 9), seg_table, seg_len, bad=bad)
    seg_table, seg_len = _layout(rng, 150, 3, 2)
    add("out-of-range-and-negative-rows-dim3", 3, (6, 2), seg_table, seg_len, bad=((5, -7), (77, None), (149, 1 << 31)))
    # every lookup on one row (the scatter's worst contention), and nothing at all
    seg_table, seg_len = _layout(rng, 5000, 3, 1)
    add("every-lookup-hits-one-row-dim8", 8, (6,), seg_table, seg_len, one_row=True)
    seg_table, seg_len = _layout(rng, 3000, 2, 1)
    add("every-lookup-hits-one-row-dim33", 33, (4,), seg_table, seg_len, one_row=True)
    add("n_rows-0", 16, (5, 5), (0, 1), (0, 0))
    # few lookups into large tables: most rows must come back untouched
    seg_table, seg_len = _layout(rng, 150, 4, 2)
    add("sparse-lookups-leave-rows-untouched-dim16", 16, (400, 250), seg_table, seg_len, bad=((3, -2), (90, None)))
    seg_table, seg_len = _layout(rng, 90, 3, 2)
    add("sparse-lookups-leave-rows-untouched-dim7", 7, (300, 120), seg_table, seg_len)
    return out


def seg_operands(case):
    """tables (float32, arbitrary bit patterns are not needed: normal floats), local_rows, seg_start; the bad rows put in."""
    rng = np.random.default_rng([SEED, case.index])
    tables = [rng.standard_normal((r, case.dim)).astype(np.float32) for r in case.table_rows]
    seg_start = np.concatenate([[0], np.cumsum(case.seg_len)]).astype(np.int64)
    n = int(seg_start[-1])
    table_of = np.repeat(np.asarray(case.seg_table, np.int64), case.seg_len)
    rows_of = np.asarray(case.table_rows, np.int64)[table_of] if n else np.zeros(0, np.int64)
    local_rows = (rng.integers(0, 1 << 30, n) % rows_of).astype(np.int64) if n else np.zeros(0, np.int64)
    if case.one_row:
        local_rows[:] = rows_of - 1          # (one table: one row)
    for pos, val in case.bad:
        local_rows[pos] = rows_of[pos] if val is None else val
    return tables, local_rows, seg_start, table_of


def gather_reference(case, tables, local_rows, table_of):
    """out[p] = tables[t][row]; a row the table does not have reads row 0 and counts in the status."""
    out = np.empty((local_rows.size, case.dim), np.float32)
    bad = []
    for p, (t, r) in enumerate(zip(table_of.tolist(), local_rows.tolist())):
        if not 0 <= r < case.table_rows[t]:
            bad.append((t, p, r))
            r = 0
        out[p] = tables[t][r]
    return out, bad


def scatter_operands(case):
    """Initial gradient tables (non-zero small integers) and g_rows (small integers), float32."""
    rng = np.random.default_rng([SEED, case.index, 1])
    init = [(rng.integers(1, INIT_MAX + 1, (r, case.dim)) * rng.choice([-1, 1], (r, case.dim))).astype(np.float32) for r in case.table_rows]
    g_rows = rng.integers(-G_MAX, G_MAX + 1, (int(sum(case.seg_len)), case.dim)).astype(np.float32)
    return init, g_rows


def scatter_reference(case, init, g_rows, local_rows, table_of, skip_row0):
    """int64 scatter-add: rows the table does not have are dropped, row 0 too when skip_row0.  Returns (tables int64, largest sum of magnitudes
    that any float32 accumulator can pass through)."""
    acc = [t.astype(np.int64) for t in init]
    mag = [np.abs(t).astype(np.int64) for t in init]
    g = g_rows.astype(np.int64)
    for t in range(len(acc)):
        sel = (table_of == t) & (local_rows >= 0) & (local_rows < case.table_rows[t])
        if skip_row0:
            sel &= local_rows != 0
        np.add.at(acc[t], local_rows[sel], g[sel])
        np.add.at(mag[t], local_rows[sel], np.abs(g[sel]))
    return acc, max(int(m.max()) for m in mag)


# ------------------------------------------------------------------------------------------------ csr_to_padded
CsrCase = namedtuple("CsrCase", "index name bits n_dataset bag_len rows_kind batch")


def csr_cases():
    out = []

    def add(name, bits, n_dataset, bag_len, rows_kind=None, batch=None):
        out.append(CsrCase(len(out), f"{name}-int{bits}", bits, n_dataset, bag_len, rows_kind, n_dataset if batch is None else batch))

    for bits in (32, 64):
        add("empty-exact-and-longer-rows-L5", bits, 300, 5)
        add("bag_len-1", bits, 300, 1)
        add("batch-0", bits, 0, 4)
        add("rows-with-repeats", bits, 90, 6, "repeats", 700)
        add("rows-permutation", bits, 257, 6, "permutation", 257)
        add("rows-batch-0", bits, 40, 3, "repeats", 0)
        add("grid-cap-4100x257", bits, 4100, 257)
    add("grid-cap-rows-4100x257", 64, 300, 257, "repeats", 4100)
    return out


def csr_operands(case):
    """values, offsets (of the whole dataset), rows or None.  Row lengths: 0, bag_len exactly, bag_len + 1, 3 * bag_len and everything between."""
    rng = np.random.default_rng([SEED, 2, case.index])
    L = case.bag_len
    lens = rng.integers(0, 2 * L + 2, case.n_dataset)
    for i, v in enumerate((0, L, L + 1, 3 * L, 0, 0, L - 1 if L > 1 else 0)):
        if i < case.n_dataset:
            lens[(i * 7) % case.n_dataset] = v
    if case.n_dataset:
        lens[-1] = 0 if case.index % 2 else 2 * L          # the last row: empty / longer than bag_len (the end of `values`)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dt = np.int32 if case.bits == 32 else np.int64
    hi = (1 << 31) - 1 if case.bits == 32 else (1 << 62)
    values = rng.integers(1, hi, int(offsets[-1])).astype(dt)
    rows = None
    if case.rows_kind == "repeats":
        rows = rng.integers(0, case.n_dataset, case.batch).astype(np.int64)
        if case.batch >= 4:
            rows[1] = rows[0]
            rows[-1] = case.n_dataset - 1
    elif case.rows_kind == "permutation":
        rows = rng.permutation(case.n_dataset).astype(np.int64)
    return values, offsets, rows


def csr_reference(values, offsets, rows, batch, bag_len):
    """The padded form as plain numpy: row b of the batch is CSR row rows[b] (or b); its first bag_len values, then zeros; mask 1 on the values.
    A row longer than bag_len keeps its FIRST bag_len values -- what the reference's DataReader does with a long history
    (data_reader.py:102-105: `indices = indices[:max_len]`, mask all ones): truncation at the tail, not a window of the most recent."""
    ids = np.zeros((batch, bag_len), values.dtype)
    mask = np.zeros((batch, bag_len), np.float32)
    for b in range(batch):
        src = b if rows is None else int(rows[b])
        row = values[offsets[src]:offsets[src + 1]][:bag_len]
        ids[b, :row.size] = row
        mask[b, :row.size] = 1.0
    return ids, mask


# ------------------------------------------------------------------------------------------------ mask_lengths
MaskCase = namedtuple("MaskCase", "index name batch bag_len")
MASK_VALUES = np.array([0.0, 1.0, 0.5, -2.0, -0.0, np.nan], np.float32)      # counted: 1, 0.5, -2, NaN (as != 0); not counted: 0, -0.0


def mask_cases():
    return [MaskCase(0, "L1", 1000, 1), MaskCase(1, "L50", 777, 50), MaskCase(2, "L3-batch-past-the-grid-cap", 2048 * BLOCK + 37, 3),
            MaskCase(3, "L50-batch-1", 1, 50)]


def mask_operands(case):
    rng = np.random.default_rng([SEED, 3, case.index])
    mask = MASK_VALUES[rng.integers(0, MASK_VALUES.size, (case.batch, case.bag_len))]
    mask[0, :] = MASK_VALUES[np.arange(case.bag_len) % MASK_VALUES.size]
    return mask


def mask_reference(mask):
    return (mask != 0).sum(axis=1).astype(np.int64)
