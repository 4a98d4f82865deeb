"""The row-utility kernels of csrc/nrx_intutil.hip alone: the C entry points nrx_gather_rows_segmented, nrx_scatter_add_rows_segmented, nrx_csr_to_padded
and nrx_mask_lengths at their launch-shape edges (tests/intutil_cases.py; tests/test_intutil_cases.py asserts what the lists reach), every result
bit for bit against a plain numpy definition.  Every buffer a kernel writes sits inside a larger allocation whose margins are poisoned and checked
afterwards; inputs are checked to come back unchanged."""
import ctypes as C

import numpy as np
import pytest

from tests import intutil_cases as ic

pytestmark = pytest.mark.gpu

PRE, POST = 8, 8                      # margin elements in front (a multiple of 16 bytes for every dtype used) and behind
POISON = {np.dtype(np.float32): -77777.0, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}


class Guarded:
    """A device array inside a poisoned allocation: `off` extra elements in front move it off the 16-byte boundary."""

    def __init__(self, array=None, shape=None, dtype=None, off=0):
        import torch
        if array is not None:
            array = np.ascontiguousarray(array)
            shape, dtype = array.shape, array.dtype
        self.shape, self.n, self.lo = tuple(shape), int(np.prod(shape)), PRE + off
        self.poison = POISON[np.dtype(dtype)]
        self.buf = torch.full((self.lo + self.n + POST,), self.poison, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + self.n]
        if array is not None and self.n:
            self.view.copy_(torch.from_numpy(array.reshape(-1)))
        self.ptr = self.view.data_ptr() if self.n else self.buf.data_ptr() + self.lo * self.buf.element_size()
        assert (self.ptr % 16 == 0) == (self.buf.element_size() * off % 16 == 0)

    def get(self):
        """The array back on the host, after checking both margins."""
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == self.poison).all(), "the margin in front of the buffer changed"
        assert (host[self.lo + self.n:] == self.poison).all(), "the margin behind the buffer changed"
        return host[self.lo:self.lo + self.n].reshape(self.shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _lib():
    from news_recsys_amd import _lib
    return _lib, _lib.load()


def _sync():
    import torch
    torch.cuda.synchronize()


SEG = ic.seg_cases()


def _seg_device(case, tables_np):
    """Tables (the LAST one off the boundary for 'table-one-float-in'), segment arrays, the host pointer arrays of the C call."""
    tables, local_rows, seg_start, table_of = ic.seg_operands(case)
    if tables_np is None:
        tables_np = tables
    n_t = len(tables_np)
    g_tables = [Guarded(t, off=1 if case.align == "table-one-float-in" and i == n_t - 1 else 0) for i, t in enumerate(tables_np)]
    tp = (C.c_void_p * n_t)(*[g.ptr for g in g_tables])
    tr = (C.c_int64 * n_t)(*case.table_rows)
    d_start, d_table, d_rows = Guarded(seg_start), Guarded(np.asarray(case.seg_table, np.int32)), Guarded(local_rows)
    return tables_np, local_rows, seg_start, table_of, g_tables, tp, tr, d_start, d_table, d_rows


@pytest.mark.parametrize("case", SEG, ids=lambda c: c.name)
def test_gather_rows_segmented(case):
    mod, lib = _lib()
    tables, local_rows, seg_start, table_of, g_tables, tp, tr, d_start, d_table, d_rows = _seg_device(case, None)
    n = int(seg_start[-1])
    out = Guarded(shape=(n, case.dim), dtype=np.float32, off=1 if case.align == "rows-one-float-in" else 0)
    status = Guarded(np.zeros(4, np.int32))
    vec = case.dim % 4 == 0 and out.ptr % 16 == 0 and all(g.ptr % 16 == 0 for g in g_tables)
    assert vec == (case.dim % 4 == 0 and case.align == "aligned")
    mod.check(lib.nrx_gather_rows_segmented(tp, tr, len(tables), d_start.ptr, d_table.ptr, len(case.seg_table), n, case.dim, d_rows.ptr, out.ptr,
                                            status.ptr, None), "nrx_gather_rows_segmented")
    _sync()
    want, bad = ic.gather_reference(case, tables, local_rows, table_of)
    assert len(bad) == len(case.bad)
    assert np.array_equal(bits(out.get()), bits(want))
    st = status.get().tolist()
    assert st[0] == len(bad)
    if bad:           # the first report is one of the bad lookups: (table, position, row), the row as the int32 word the status holds
        wrap = lambda v: int(np.array(v, np.int64).astype(np.int32))
        assert tuple(st[1:]) in {(t, p, wrap(r)) for t, p, r in bad}
    else:
        assert st[1:] == [0, 0, 0]
    # nothing else moved
    for g, t in zip(g_tables, tables):
        assert np.array_equal(bits(g.get()), bits(t))
    assert np.array_equal(d_rows.get(), local_rows) and np.array_equal(d_start.get(), seg_start)
    assert np.array_equal(d_table.get(), np.asarray(case.seg_table, np.int32))


def test_gather_without_a_status_buffer_still_reads_row_0():
    mod, lib = _lib()
    case = next(c for c in SEG if c.name == "out-of-range-and-negative-rows-dim3")
    tables, local_rows, seg_start, table_of, g_tables, tp, tr, d_start, d_table, d_rows = _seg_device(case, None)
    n = int(seg_start[-1])
    out = Guarded(shape=(n, case.dim), dtype=np.float32)
    mod.check(lib.nrx_gather_rows_segmented(tp, tr, len(tables), d_start.ptr, d_table.ptr, len(case.seg_table), n, case.dim, d_rows.ptr, out.ptr,
                                            None, None), "nrx_gather_rows_segmented")
    _sync()
    assert np.array_equal(bits(out.get()), bits(ic.gather_reference(case, tables, local_rows, table_of)[0]))


@pytest.mark.parametrize("skip_row0", [0, 1], ids=["skip_row0-0", "skip_row0-1"])
@pytest.mark.parametrize("case", SEG, ids=lambda c: c.name)
def test_scatter_add_rows_segmented(case, skip_row0):
    """Small-integer operands: float32 atomics are exact in any order (the bound: tests/test_intutil_cases.py), so the tables must equal an int64
    scatter bit for bit -- rows no lookup reaches included, which start non-zero."""
    mod, lib = _lib()
    init, g_rows = ic.scatter_operands(case)
    _, local_rows, seg_start, table_of, g_tables, tp, tr, d_start, d_table, d_rows = _seg_device(case, init)
    n = int(seg_start[-1])
    d_g = Guarded(g_rows, off=1 if case.align == "rows-one-float-in" else 0)
    mod.check(lib.nrx_scatter_add_rows_segmented(tp, tr, len(init), d_start.ptr, d_table.ptr, len(case.seg_table), n, case.dim, d_rows.ptr, d_g.ptr,
                                                 skip_row0, None), "nrx_scatter_add_rows_segmented")
    _sync()
    acc, mag = ic.scatter_reference(case, init, g_rows, local_rows, table_of, skip_row0)
    assert mag < 1 << 24
    for t, (g, a) in enumerate(zip(g_tables, acc)):
        got = g.get()
        assert np.array_equal(bits(got), bits(a.astype(np.float32))), f"table {t}"
        if skip_row0:
            assert np.array_equal(bits(got[0]), bits(init[t][0])), f"table {t}: the padding row received a gradient"
    assert np.array_equal(bits(d_g.get()), bits(g_rows)) and np.array_equal(d_rows.get(), local_rows)


# ------------------------------------------------------------------------------------------------ csr_to_padded
@pytest.mark.parametrize("case", ic.csr_cases(), ids=lambda c: c.name)
def test_csr_to_padded(case):
    mod, lib = _lib()
    values, offsets, rows = ic.csr_operands(case)
    d_values, d_offsets = Guarded(values), Guarded(offsets)
    d_rows = Guarded(rows) if rows is not None else None
    dt = values.dtype
    ids = Guarded(shape=(case.batch, case.bag_len), dtype=dt)
    mask = Guarded(shape=(case.batch, case.bag_len), dtype=np.float32)
    mod.check(lib.nrx_csr_to_padded(d_values.ptr if values.size else None, case.bits, d_offsets.ptr, d_rows.ptr if d_rows else None, case.batch,
                                    case.bag_len, ids.ptr, mask.ptr, None), "nrx_csr_to_padded")
    _sync()
    want_ids, want_mask = ic.csr_reference(values, offsets, rows, case.batch, case.bag_len)
    assert np.array_equal(ids.get(), want_ids)
    assert np.array_equal(bits(mask.get()), bits(want_mask))
    assert np.array_equal(d_values.get(), values) and np.array_equal(d_offsets.get(), offsets)


# ------------------------------------------------------------------------------------------------ mask_lengths
@pytest.mark.parametrize("case", ic.mask_cases(), ids=lambda c: c.name)
def test_mask_lengths_counts_half_minus_two_and_nan_but_not_negative_zero(case):
    """0.5, -2 and NaN count (the kernel's test is != 0), 0 and -0.0 do not."""
    mod, lib = _lib()
    m = ic.mask_operands(case)
    d_m = Guarded(m)
    lens = Guarded(shape=(case.batch,), dtype=np.int64)
    mod.check(lib.nrx_mask_lengths(d_m.ptr, case.batch, case.bag_len, lens.ptr, None), "nrx_mask_lengths")
    _sync()
    assert np.array_equal(lens.get(), ic.mask_reference(m))
    assert np.array_equal(bits(d_m.get()), bits(m))


def test_mask_lengths_and_csr_of_an_empty_batch_touch_nothing():
    mod, lib = _lib()
    lens = Guarded(shape=(0,), dtype=np.int64)
    mod.check(lib.nrx_mask_lengths(None, 0, 3, lens.ptr, None), "nrx_mask_lengths")
    assert lib.nrx_csr_to_padded(None, 64, None, None, 0, 3, None, None, None) == 0
    _sync()
    assert lens.get().size == 0
