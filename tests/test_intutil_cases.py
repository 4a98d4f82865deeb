"""CPU checks of tests/intutil_cases.py: the case lists reach every launch-shape edge of the gather / scatter / csr_to_padded / mask_lengths kernels
(a condition, so a list that stops reaching an edge fails here), the scatter's integer operands keep every float32 accumulator exact, the references
agree with independent restatements, and the generator is deterministic."""
import numpy as np

from oracle import ref_np as R
from tests import intutil_cases as ic

SEG = ic.seg_cases()
CSR = ic.csr_cases()
MASK = ic.mask_cases()


def _n_rows(c):
    return sum(c.seg_len)


def test_launch_shape_restatement():
    assert [ic.ql_of(d) for d in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1000)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6]
    assert [ic.tb_of(d) for d in (4, 5, 16, 17, 128, 129, 1000)] == [256, 128, 64, 32, 8, 4, 4]


def test_seg_cases_cover_every_edge():
    assert len({c.name for c in SEG}) == len(SEG) and [c.index for c in SEG] == list(range(len(SEG)))
    # each side of every lanes-per-row switch, the widths where a lane loops again, the narrow ones
    assert {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 260, 1000} == set(ic.WIDTHS) <= {c.dim for c in SEG}
    assert {ic.ql_of(c.dim) for c in SEG} == set(range(7))
    for dim in ic.WIDTHS:
        tb = ic.tb_of(dim)
        assert {tb - 1, tb, tb + 1} <= {_n_rows(c) for c in SEG if c.dim == dim and c.align == "aligned"}, dim
    # the scalar path by pointer only: dim % 4 == 0 with a table / the row buffer one float into its allocation
    for align in ic.ALIGNS[1:]:
        mine = [c for c in SEG if c.align == align]
        assert mine and all(c.dim % 4 == 0 for c in mine) and {4, 256, 260} <= {c.dim for c in mine}
        assert all(_n_rows(c) > 2 * ic.tb_of(c.dim) for c in mine)          # more than one block
    # segment counts and where the empty segments sit
    assert any(len(c.seg_len) == 1 for c in SEG)
    full = [c for c in SEG if len(c.seg_len) == ic.MAX_SEG]
    assert full
    for c in full:
        ln = np.array(c.seg_len)
        assert (ln[:5] == 0).all()
        assert (ln[2000:2101] == 0).all() and (ln[-7:] == 0).all() and ln[:2000].sum() > 0 and ln[2101:].sum() > 0
    assert any(len(c.table_rows) == ic.MAX_TABLES for c in SEG)
    assert any(0 in c.seg_len[1:-1] for c in SEG if len(c.seg_len) == 5)
    # bad rows: negative and too large, on both the float4 and the scalar path; first / last position of the launch among them
    bad = [c for c in SEG if c.bad]
    assert {c.dim % 4 == 0 for c in bad} == {True, False}
    for c in bad:
        _, rows, _, table_of = ic.seg_operands(c)
        lim = np.asarray(c.table_rows)[table_of]
        assert (rows < 0).any() and (rows >= lim).any() and (rows == lim).any()
        assert ((rows < 0) | (rows >= lim)).sum() == len(c.bad)
    assert any(p == 0 for c in bad for p, _ in c.bad) and any(p == _n_rows(c) - 1 for c in bad for p, _ in c.bad)
    assert any(c.one_row for c in SEG) and any(_n_rows(c) == 0 for c in SEG)
    assert {c.dim % 4 == 0 for c in SEG if c.name.startswith("sparse-lookups-leave-rows-untouched")} == {True, False}
    for c in SEG:
        if c.one_row:
            _, rows, _, _ = ic.seg_operands(c)
            assert len(set(rows.tolist())) == 1 and rows.size >= 3000
    # row 0 is looked up wherever skip_row0 is to matter
    assert sum((ic.seg_operands(c)[1] == 0).any() for c in SEG) > len(SEG) // 2
    assert all(len(c.seg_len) + 1 <= 8192 and _n_rows(c) * c.dim * 4 <= 8 << 20 for c in SEG)          # operands stay small


def test_scatter_sums_stay_exact_in_float32():
    """Every accumulator passes only through integers of magnitude <= sum of the magnitudes added: below 2^24 float32 adds are exact in any order."""
    worst = 0
    for c in SEG:
        tables, rows, seg_start, table_of = ic.seg_operands(c)
        init, g = ic.scatter_operands(c)
        for arr in init + [g]:
            assert arr.dtype == np.float32 and np.array_equal(arr, np.rint(arr))
        assert all((np.abs(t) >= 1).all() and np.abs(t).max() <= ic.INIT_MAX for t in init) and (g.size == 0 or np.abs(g).max() <= ic.G_MAX)
        for skip in (0, 1):
            acc, mag = ic.scatter_reference(c, init, g, rows, table_of, skip)
            worst = max(worst, mag)
            assert all(np.array_equal(a.astype(np.float32).astype(np.int64), a) for a in acc)
    assert 5000 < worst < 1 << 24          # (the one-row cases pile thousands of lookups on one accumulator)


def test_references_equal_independent_restatements():
    c = next(c for c in SEG if c.name == "sparse-lookups-leave-rows-untouched-dim16")
    tables, rows, seg_start, table_of = ic.seg_operands(c)
    want, bad = ic.gather_reference(c, tables, rows, table_of)
    assert len(bad) == len(c.bad) and {p for _, p, _ in bad} == {p for p, _ in c.bad}
    ok = np.ones(rows.size, bool)
    ok[[p for _, p, _ in bad]] = False
    for s, t in enumerate(c.seg_table):                       # segment by segment, with the oracle's row gather
        lo, hi = seg_start[s], seg_start[s + 1]
        r = np.where(ok[lo:hi], rows[lo:hi], 0)
        assert np.array_equal(want[lo:hi].view(np.int32), R.gather_rows(tables[t], r).view(np.int32))
    init, g = ic.scatter_operands(c)
    for skip in (0, 1):
        acc, _ = ic.scatter_reference(c, init, g, rows, table_of, skip)
        naive = [t.astype(np.int64) for t in init]
        for p in range(rows.size):
            t, r = int(table_of[p]), int(rows[p])
            if 0 <= r < c.table_rows[t] and not (skip and r == 0):
                naive[t][r] += g[p].astype(np.int64)
        assert all(np.array_equal(a, b) for a, b in zip(acc, naive))
        touched = [np.zeros(n, bool) for n in c.table_rows]
        for p in range(rows.size):
            t, r = int(table_of[p]), int(rows[p])
            if 0 <= r < c.table_rows[t] and not (skip and r == 0):
                touched[t][r] = True
        assert all((~m).sum() > m.size // 2 for m in touched)          # the case leaves rows untouched: they must come back bit-unchanged
    for cc in CSR:
        if cc.rows_kind is None and cc.n_dataset and cc.n_dataset * cc.bag_len < 5000:
            values, offsets, _ = ic.csr_operands(cc)
            ids, mask = ic.csr_reference(values, offsets, None, cc.batch, cc.bag_len)
            rid, rmask = R.csr_bag_to_padded(values, offsets, cc.bag_len)
            assert np.array_equal(ids, rid) and np.array_equal(mask, rmask)


def test_csr_cases_cover_every_edge():
    assert len({c.name for c in CSR}) == len(CSR) and [c.index for c in CSR] == list(range(len(CSR)))
    for bits in (32, 64):
        mine = [c for c in CSR if c.bits == bits]
        assert any(c.bag_len == 1 for c in mine) and any(c.batch == 0 for c in mine)
        assert {c.rows_kind for c in mine} == {None, "repeats", "permutation"}
        assert any(c.batch * c.bag_len > 4096 * ic.BLOCK for c in mine)                     # past the grid cap
        assert any(0 < c.batch * c.bag_len <= 4096 * ic.BLOCK for c in mine)
        for c in mine:
            values, offsets, rows = ic.csr_operands(c)
            lens = np.diff(offsets)
            assert values.dtype == (np.int32 if bits == 32 else np.int64) and (values != 0).all()
            if c.n_dataset >= 30:
                assert (lens == 0).any() and (lens == c.bag_len).any() and (lens > c.bag_len).any()
            if c.rows_kind == "repeats" and c.batch:
                assert len(set(rows.tolist())) < rows.size and rows.max() == c.n_dataset - 1
            if c.rows_kind == "permutation":
                assert sorted(rows.tolist()) == list(range(c.n_dataset)) and not np.array_equal(rows, np.arange(c.n_dataset))
    assert any(c.rows_kind and c.batch * c.bag_len > 4096 * ic.BLOCK for c in CSR)
    # a long row keeps its first bag_len values
    ids, mask = ic.csr_reference(np.arange(1, 8), np.array([0, 7]), None, 1, 3)
    assert ids.tolist() == [[1, 2, 3]] and mask.tolist() == [[1, 1, 1]]


def test_mask_cases_cover_every_edge():
    assert {1, 50, 3} <= {c.bag_len for c in MASK}
    assert any(c.batch > 2048 * ic.BLOCK and c.bag_len == 3 for c in MASK)
    v = ic.MASK_VALUES
    assert 0.5 in v and -2.0 in v and np.isnan(v).any() and ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
    assert ic.mask_reference(v[None, :]).tolist() == [4]                       # 1, 0.5, -2 and NaN count; 0 and -0.0 do not
    for c in MASK:
        m = ic.mask_operands(c)
        assert m.shape == (c.batch, c.bag_len) and m.dtype == np.float32
        if c.batch * c.bag_len >= 1000:
            assert np.isnan(m).any() and ((m == 0) & np.signbit(m)).any() and (m == 0.5).any() and (m == -2).any()
        ref = ic.mask_reference(m)
        assert ref.min() >= 0 and ref.max() <= c.bag_len
        off, _ = R.csr_from_mask(m)
        assert np.array_equal(np.diff(off), ref)


def test_the_generator_is_deterministic():
    assert ic.seg_cases() == SEG and ic.csr_cases() == CSR and ic.mask_cases() == MASK
    c = SEG[7]
    a, b = ic.seg_operands(c), ic.seg_operands(c)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert not np.array_equal(ic.scatter_operands(SEG[7])[1], ic.scatter_operands(SEG[8])[1][: ic.scatter_operands(SEG[7])[1].shape[0]])
