"""The pooled-bag inbox kernels of csrc/nrx_route.hip alone, through the C ABI, at the edges of their launch arithmetic: every lane-group width
QLOG2 = 0..6, one, two and four passes over the columns, the Q == 1 load path and the exchange at 8 / 4 / 2 / 1 entries per lane with lanes that
load nothing, runs of 0 / 1 / 2 / 15 / 16 / 17 / 31 / 32 / 33 / 50 entries, 1 / TB - 1 / TB / TB + 1 / 3 TB + 5 / 3 TB + 6 tags, worlds 1-3 with an
empty block and a block clipped at cap, three features on two tables, rows and tags out of range, a row hit 200 times, the vector and the scalar
path of the expansion, narrow and wide norm weights, and every grid-stride wrap.  Against tests/pool_inbox_ref.py (held to oracle/ref_np.py by
tests/test_pool_inbox_ref.py):
  * bit for bit where the arithmetic is fixed: both forms of the forward (entry order, product then add, contraction off), the bf16 forward
    against the fp32 call on the widened tables, the expansion's rows fp32(w g), a table row that one entry names, norm weights of 0 / 1 masks,
    the upstream rows, every integer word;
  * inside gamma(k) sum |terms| elsewhere, k counted from the source: the dense backward (atomics in any order: n + 1), norm weights of
    weighted masks (L + 2).
Every device buffer is the body of a larger allocation whose every byte is 0xFF (NaN as a float, -1 as an integer); outputs start that way too.
After a call the margins are still 0xFF and every input holds what it held.

Each test prints its worst error / bound (pytest -s shows them); those figures are for the record, the asserts are the bounds themselves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib
from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM, NRX_ERR_BAD_ARG, NRX_OK
from tests import pool_inbox_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
KIND = {"masked_mean": NRX_BAG_MASKED_MEAN, "mean": NRX_BAG_MEAN, "sum": NRX_BAG_SUM}
MARGIN = 64                               # elements either side of a body: 128 bytes and more, so a body stays 16-byte aligned


class Buf:
    """A body of `shape` elements inside a device allocation of 0xFF bytes (MARGIN + off elements in front, MARGIN + 3 behind).  data=None:
    an output, 0xFF throughout.  read() returns the body and asserts that the margins are still 0xFF; unchanged() asserts that nothing
    at all was written."""

    def __init__(self, data=None, shape=None, dtype=None, off=0):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape))
        self.front = MARGIN + off
        host = np.full((self.front + self.n + MARGIN + 3) * self.dtype.itemsize, 0xFF, np.uint8)
        if data is not None:
            host[self.front * self.dtype.itemsize:(self.front + self.n) * self.dtype.itemsize] = data.reshape(-1).view(np.uint8)
        self.host0 = host
        self.t = torch.from_numpy(host.copy()).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front * self.dtype.itemsize

    def _now(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def read(self):
        host = self._now()
        lo, hi = self.front * self.dtype.itemsize, (self.front + self.n) * self.dtype.itemsize
        assert (host[:lo] == 0xFF).all() and (host[hi:] == 0xFF).all(), "a byte outside the result was written"
        return host[lo:hi].view(self.dtype).reshape(self.shape).copy()

    def unchanged(self):
        assert np.array_equal(self._now(), self.host0), "an input or an unused output was written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == NRX_OK, (what, rc, _lib.load().nrx_last_error())
    torch.cuda.synchronize()


def _ratio(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    assert not np.isnan(err).any()
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0


def _note(key, r):
    print(f"pool_inbox gpu worst error / bound: {key} {r:.4f}")


def _parr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


def _i32(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def _untouched(b):
    """An output no launch wrote: 0xFF throughout."""
    assert (b._now() == 0xFF).all(), "a refused or empty call wrote something"


class DevInbox:
    def __init__(self, ib):
        self.ib = ib
        self.rows, self.tag, self.w = Buf(ib.rows), Buf(ib.tag), Buf(ib.w)
        self.recv, self.run = Buf(ib.recv2d), Buf(ib.run)

    def head(self):
        ib = self.ib
        return (ib.n_feats, ib.batch, ib.world, ib.cap, self.recv.ptr)

    def unchanged(self):
        for b in (self.rows, self.tag, self.w, self.recv, self.run):
            b.unchanged()


def _tables(ib, bufs):
    return _parr([b.ptr for b in bufs]), _i64(ib.table_rows), len(bufs), _i32(ib.feat_table)


def _status():
    return Buf(np.zeros(4, np.int32))


def pool_fwd(d, tbufs, form, bf16=False):
    """One forward launch: (partial, status[4]).  The mark form's workspace must hold pool_mark_kernel's run bounds afterwards."""
    lib, ib = _lib.load(), d.ib
    part, st = Buf(shape=(ib.world, ib.ntag, ib.dim), dtype=F32), _status()
    if form == "mark":
        ws = Buf(shape=(ib.world, ib.ntag, 2), dtype=np.int32)
        assert lib.nrx_pool_inbox_workspace(ib.n_feats, ib.batch, ib.world) == ws.n * 4
        fn = lib.nrx_pool_inbox_fwd_bf16 if bf16 else lib.nrx_pool_inbox_fwd
        _ok(fn(*_tables(ib, tbufs), *d.head(), d.rows.ptr, d.tag.ptr, d.w.ptr, ib.dim, part.ptr, ws.ptr, st.ptr, _stream()), "forward, mark form")
        assert np.array_equal(ws.read(), ib.run), "the marking pass's run bounds"
    else:
        fn = lib.nrx_pool_inbox_fwd_runs_bf16 if bf16 else lib.nrx_pool_inbox_fwd_runs
        _ok(fn(*_tables(ib, tbufs), *d.head(), d.rows.ptr, d.w.ptr, d.run.ptr, ib.dim, part.ptr, st.ptr, _stream()), "forward, runs form")
    d.unchanged()
    for b in tbufs:
        b.unchanged()
    return part.read(), st.read()


def _check_status(st, ib, what):
    reports = P.oob_reports(ib)
    if not reports:
        assert st.tolist() == [0, 0, 0, 0], (what, st)                  # untouched: every row with a weight is inside its table
    else:                                                                # one count per entry; the first to arrive leaves (table, slot, row)
        assert st[0] == len(reports) and tuple(int(x) for x in st[1:]) in reports, (what, st, len(reports))


@functools.lru_cache(maxsize=None)
def _fwd_ref(dim, key):
    ib, tables = P.case_inbox(dim, key), P.case_tables(dim)
    ref, scale, n = P.pool_fwd64(ib, tables)
    dead = np.ones((ib.world, ib.ntag), bool)                           # tags none of whose entries reaches a row
    e = P.entries(ib)
    hit = e.tag_ok & e.row_ok
    dead[e.s[hit], e.tag[hit]] = False
    return P.pool_fwd32(ib, tables), ref, P.gamma(n)[..., None] * scale, n, dead


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("dim", P.DIMS)
def test_forward_mark_and_runs_form_bit_for_bit(dim):
    worst = 0.0
    tbufs = [Buf(t) for t in P.case_tables(dim)]
    for key, *_ in P.inbox_cases(dim):
        ib = P.case_inbox(dim, key)
        want, ref, bound, n, dead = _fwd_ref(dim, key)
        d = DevInbox(ib)
        got, st = pool_fwd(d, tbufs, "mark")
        assert not np.isnan(got).any(), key                              # every element of [world, ntag, dim] is written
        assert P.same_bits(got, want), (key, int((got != want).sum()))
        assert not got[dead].view(np.int32).any(), key                   # +0.f: empty runs, an empty block, runs of rows out of range only
        assert (n[dead] > 0).any() or key != "main"
        r = _ratio(got, ref, bound)
        assert r <= 1.0, (key, r)
        worst = max(worst, _ratio(got[n >= 2], ref[n >= 2], bound[n >= 2]))      # (a run of one entry: ONE rounding under gamma(1), ~1 by construction)
        _check_status(st, ib, (key, "mark"))
        got_runs, st = pool_fwd(d, tbufs, "runs")
        assert P.same_bits(got_runs, got), key
        _check_status(st, ib, (key, "runs"))
    _note(f"forward against float64, runs of two entries and more dim={dim}", worst)


def test_forward_status_is_silent_for_a_weightless_row_out_of_range_and_optional():
    dim = 16
    ib0 = P.case_inbox(dim, "main")
    e = P.entries(ib0)
    w = ib0.w.copy()
    w[e.counted & ~e.row_ok] = 0
    ib = P.inbox_from_arrays(ib0.world, ib0.n_feats, ib0.batch, ib0.cap, dim, ib0.table_rows, ib0.feat_table, ib0.rows, ib0.tag, w, ib0.recv2d)
    assert not P.oob_reports(ib) and P.inbox_facts(ib)["row out of range without weight"]
    tbufs, d = [Buf(t) for t in P.case_tables(dim)], DevInbox(ib)
    want = P.pool_fwd32(ib, P.case_tables(dim))
    for form in ("mark", "runs"):
        got, st = pool_fwd(d, tbufs, form)
        assert P.same_bits(got, want) and st.tolist() == [0, 0, 0, 0], form
    lib, d0 = _lib.load(), DevInbox(ib0)                                 # status = NULL: the same partial sums, nothing reported
    part, ws = Buf(shape=(ib0.world, ib0.ntag, dim), dtype=F32), Buf(shape=(ib0.world, ib0.ntag, 2), dtype=np.int32)
    _ok(lib.nrx_pool_inbox_fwd(*_tables(ib0, tbufs), *d0.head(), d0.rows.ptr, d0.tag.ptr, d0.w.ptr, dim, part.ptr, ws.ptr, None, _stream()), "fwd")
    assert P.same_bits(part.read(), _fwd_ref(dim, "main")[0])


@pytest.mark.parametrize("dim", P.BF16_DIMS)
def test_forward_bf16_tables_give_the_bits_of_the_widened_fp32_call(dim):
    bits, wide = P.bf16_tables(dim)
    b16, b32 = [Buf(t) for t in bits], [Buf(t) for t in wide]
    for key, *_ in P.inbox_cases(dim):
        d = DevInbox(P.case_inbox(dim, key))
        for form in ("mark", "runs"):
            got, st = pool_fwd(d, b16, form, bf16=True)
            want, st32 = pool_fwd(d, b32, form)
            assert P.same_bits(got, want), (key, form)
            assert st[0] == st32[0], (key, form)
            _check_status(st, d.ib, (key, form))


# ------------------------------------------------------------------------------------------------- dense backward
@pytest.mark.parametrize("dim", P.DIMS)
def test_dense_backward_in_bound_and_single_entries_bit_for_bit(dim):
    lib, worst, hot = _lib.load(), 0.0, 0
    for key, *_ in P.inbox_cases(dim):
        ib = P.case_inbox(dim, key)
        g = P.case_g_partial(ib)
        d, gb = DevInbox(ib), Buf(g)
        for skip_row0 in (0, 1):
            grads = [Buf(np.zeros((r, dim), F32)) for r in ib.table_rows]
            _ok(lib.nrx_pool_inbox_bwd(*_tables(ib, grads), *d.head(), d.rows.ptr, d.tag.ptr, d.w.ptr, dim, gb.ptr, skip_row0, _stream()),
                "nrx_pool_inbox_bwd")
            d.unchanged()
            gb.unchanged()
            for x, (ref, n, scale, single) in enumerate(P.pool_bwd64(ib, g, skip_row0)):
                got = grads[x].read()
                r = _ratio(got, ref, P.gamma(n + 1)[:, None] * scale)
                assert r <= 1.0, (key, skip_row0, x, r)
                worst = max(worst, _ratio(got[n >= 2], ref[n >= 2], (P.gamma(n + 1)[:, None] * scale)[n >= 2]))      # (n = 1: 1/2 by construction)
                assert not got[n == 0].view(np.int32).any(), (key, skip_row0, x)             # rows no entry names: +0.f still
                assert P.same_bits(got[n == 1], single[n == 1]), (key, skip_row0, x)
                if skip_row0:
                    assert n[0] == 0
                if key == "main" and x == P.HOT[0]:
                    hot = max(hot, int(n[P.HOT[1]]))
    assert hot >= 200, hot
    _note(f"dense backward against float64, rows of two entries and more dim={dim} (hot row: {hot} entries)", worst)


# ------------------------------------------------------------------------------------------------- expansion
@pytest.mark.parametrize("dim", P.DIMS)
def test_expansion_ids_and_rows_bit_for_bit(dim):
    lib = _lib.load()
    for key, *_ in P.inbox_cases(dim):
        ib = P.case_inbox(dim, key)
        g = P.case_g_partial(ib)
        d, gb = DevInbox(ib), Buf(g)
        for table_rows, skip_row0 in ((P.TABLE_ROWS[1], 0), (150, 1)):
            ids, live, g_rows = P.pool_expand(ib, table_rows, skip_row0, g)
            oid, rows = Buf(shape=(ib.world * ib.cap,), dtype=np.int32), Buf(shape=(ib.world * ib.cap, dim), dtype=F32)
            _ok(lib.nrx_pool_inbox_expand(table_rows, *d.head(), d.rows.ptr, d.tag.ptr, d.w.ptr, dim, gb.ptr, skip_row0, oid.ptr, rows.ptr,
                                          _stream()), "nrx_pool_inbox_expand")
            d.unchanged()
            gb.unchanged()
            assert np.array_equal(oid.read(), ids), (key, table_rows)
            got = rows.read()
            assert P.same_bits(got[live], g_rows[live]), (key, table_rows)
            assert (got[~live].view(np.uint8) == 0xFF).all(), (key, table_rows)               # written for the live entries only
            oid = Buf(shape=(ib.world * ib.cap,), dtype=np.int32)
            _ok(lib.nrx_pool_inbox_expand(table_rows, *d.head(), d.rows.ptr, d.tag.ptr, d.w.ptr, dim, None, skip_row0, oid.ptr, None, _stream()),
                "nrx_pool_inbox_expand, ids alone")
            assert np.array_equal(oid.read(), ids), (key, table_rows)


# ------------------------------------------------------------------------------------------------- owner words and the remap
def _owner_words(ib, table_rows, skip_row0):
    """nrx_pool_inbox_owner_ids and nrx_pool_inbox_runs_words on one inbox against the expansion's ids and the definitions."""
    lib, d = _lib.load(), DevInbox(ib)
    n = ib.world * ib.cap
    ids = P.pool_expand(ib, table_rows, skip_row0)[0]
    pay = P.pool_payload(ib, table_rows, skip_row0)
    for with_payload in (True, False):
        oid, pv = Buf(shape=(n,), dtype=np.int32), Buf(shape=(n,), dtype=np.uint32)
        _ok(lib.nrx_pool_inbox_owner_ids(table_rows, *d.head(), d.rows.ptr, d.tag.ptr, skip_row0, oid.ptr, pv.ptr if with_payload else None,
                                         _stream()), "nrx_pool_inbox_owner_ids")
        assert np.array_equal(oid.read(), ids)
        if with_payload:
            assert np.array_equal(pv.read(), pay)
        else:
            pv.unchanged()
    tag_want, oid_want, pay_want = P.runs_words(ib, table_rows, skip_row0)
    inside = oid_want != -1
    assert np.array_equal(oid_want[inside], ids[inside]) and np.array_equal(pay_want[inside], pay[inside])
    for use in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 1, 1)):
        outs = [Buf(shape=(n,), dtype=dt) for dt in (np.int32, np.int32, np.uint32)]
        _ok(lib.nrx_pool_inbox_runs_words(table_rows, *d.head(), d.rows.ptr, d.run.ptr, skip_row0, *[b.ptr if u else None for b, u in zip(outs, use)],
                                          _stream()), "nrx_pool_inbox_runs_words")
        for b, u, want in zip(outs, use, (tag_want, oid_want, pay_want)):
            if u:
                assert np.array_equal(b.read(), want), use                # (-1 where the launch writes nothing: tag_out outside the runs)
            else:
                b.unchanged()
    d.unchanged()


@pytest.mark.parametrize("dim", [1, 16, 1024])
def test_owner_ids_and_runs_words_equal_the_expansions_ids_and_the_payload(dim):
    for key, *_ in P.inbox_cases(dim):
        for table_rows, skip_row0 in ((P.TABLE_ROWS[1], 0), (150, 1)):
            _owner_words(P.case_inbox(dim, key), table_rows, skip_row0)


def _flat_inbox(rng, cap, ntag, total, per_tag, table_rows, must=()):
    """One source, one feature: about `total` entries whose tags rise (per_tag entries on every tag drawn and on the tags of `must`), rows from -2
    to table_rows + 1."""
    tags = np.unique(np.r_[rng.choice(ntag, total // per_tag, replace=False), np.asarray(must, np.int64)]).repeat(per_tag)
    assert tags.size <= cap
    tag = np.full(cap, P.GARBAGE_TAG, np.int64)
    tag[:tags.size] = tags
    rows = rng.integers(-2, table_rows + 2, cap)
    rows[tags.size:] = P.GARBAGE_ROW
    return P.inbox_from_arrays(1, 1, ntag, cap, 4, [table_rows], [0], rows, tag, np.ones(cap, F32), [[tags.size]])


def test_owner_words_past_their_grid_caps():
    rng = np.random.default_rng(41)
    cap = P.OWNER_IDS_GRID_CAP * P.NRX_BLOCK + P.NRX_BLOCK + 37          # 2048 blocks of 256 slots, and a second trip for 293 of them
    _owner_words(_flat_inbox(rng, cap, 1000, cap - 101, 600, 300), 300, 1)
    ntag = P.RUNS_WORDS_GRID_CAP * 16 + 16 + 3                           # 8192 blocks of 16 tags, and a second trip for 19 tags
    ib = _flat_inbox(rng, 40001, ntag, 39000, 2, 300, must=(ntag - 17, ntag - 1))
    assert ib.run[0, P.RUNS_WORDS_GRID_CAP * 16:, 1].any()               # a run among the tags of the second trip
    _owner_words(ib, 300, 0)


def _remap(order, n, tag, cap, n_tags, world):
    ob, tb_ = Buf(np.asarray(order, np.int64)), Buf(np.asarray(tag, np.int32))
    _ok(_lib.load().nrx_pool_order_remap(ob.ptr, n, tb_.ptr, cap, n_tags, world, _stream()), "nrx_pool_order_remap")
    tb_.unchanged()
    assert np.array_equal(ob.read(), P.order_remap(order, n, tag, cap, n_tags, world))


def test_order_remap_equals_its_definition_and_wraps():
    rng = np.random.default_rng(42)
    ib = P.case_inbox(16, "main")
    n = ib.world * ib.cap
    order = rng.permutation(np.r_[rng.permutation(n)[:n - 306], [-1, -n, n, n + 1, 1 << 40, -(1 << 40)], rng.integers(-5, n + 5, 300)])
    assert order.size == n
    _remap(order, n, ib.tag, ib.cap, ib.ntag, ib.world)
    _remap(order[:n - 3], n - 3, ib.tag, ib.cap, ib.ntag, ib.world)      # fewer entries than slots: the last three names are past the end
    cap, world, n_tags = (P.REMAP_GRID_CAP * P.NRX_BLOCK) // 2 + 151, 2, 77
    n = world * cap                                                      # 8192 blocks of 256 entries and 302 more
    assert n > P.REMAP_GRID_CAP * P.NRX_BLOCK
    _remap(rng.integers(-5, n + 5, n), n, rng.integers(-3, n_tags + 3, n), cap, n_tags, world)


# ------------------------------------------------------------------------------------------------- norm weights
def _norm(mask, B, L, kind, with_inv):
    lib = _lib.load()
    mb = Buf(mask) if mask is not None else None
    out, inv = Buf(shape=(B, L), dtype=F32), Buf(shape=(B,), dtype=F32)
    mp = mb.ptr if mb else None
    if with_inv:
        _ok(lib.nrx_bag_norm_weights_inv(mp, B, L, KIND[kind], out.ptr, inv.ptr, _stream()), "nrx_bag_norm_weights_inv")
    else:
        _ok(lib.nrx_bag_norm_weights(mp, B, L, KIND[kind], out.ptr, _stream()), "nrx_bag_norm_weights")
        inv.unchanged()
    if mb:
        mb.unchanged()
    return out.read(), inv.read() if with_inv else None


@pytest.mark.parametrize("L", P.NORM_LS)
def test_norm_weights_bit_for_bit_on_binary_masks_and_in_bound_on_weighted_ones(L):
    worst = 0.0
    for B in P.norm_batches(L):
        binary, weighted = P.norm_masks(B, L)
        for kind in P.NORM_KINDS:
            want, want_inv = P.norm_weights32(binary, B, L, kind)
            out, inv = _norm(binary, B, L, kind, True)
            assert P.same_bits(out, want) and P.same_bits(inv, want_inv), (B, kind)
            assert P.same_bits(_norm(binary, B, L, kind, False)[0], want), (B, kind)
            if kind != "masked_mean":                                    # no mask where it is allowed: every weight 1
                want, want_inv = P.norm_weights32(None, B, L, kind)
                out, inv = _norm(None, B, L, kind, True)
                assert P.same_bits(out, want) and P.same_bits(inv, want_inv), (B, kind)
                assert P.same_bits(_norm(None, B, L, kind, False)[0], want), (B, kind)
        out, inv = _norm(binary, B, L, "masked_mean", True)
        empty = ~binary.any(1)
        assert empty[0] and not out[empty].view(np.int32).any() and not inv[empty].view(np.int32).any()      # an empty bag: +0.f
        assert P.same_bits(_norm(weighted, B, L, "mean", True)[0], np.full((B, L), F32(1) / F32(L), F32)), B  # 1 / L exactly
        assert P.same_bits(_norm(weighted, B, L, "sum", True)[0], weighted), B
        out, inv = _norm(weighted, B, L, "masked_mean", True)
        ref, rinv = P.norm_weights64(weighted, B, L)
        r = _ratio(out, ref, P.gamma(L + 2) * np.abs(ref))
        ri = _ratio(inv[~empty], rinv[~empty], P.gamma(L + 2) * np.abs(rinv[~empty]))
        assert r <= 1.0 and ri <= 1.0 and not inv[empty].view(np.int32).any(), (B, r, ri)
        assert P.same_bits(_norm(weighted, B, L, "masked_mean", False)[0], out), B
        worst = max(worst, r, ri)
    _note(f"norm weights of weighted masks against float64 L={L}", worst)


# ------------------------------------------------------------------------------------------------- the element-wise launches
def _upstream(dim, batch, col, pad, copies, gap, with_scale):
    g_out, scale = P.upstream_inputs(dim, batch, col, pad)
    stride = batch * dim + gap
    gb, sb = Buf(g_out), Buf(scale)
    dst = Buf(shape=((copies - 1) * stride + batch * dim,), dtype=F32)
    _ok(_lib.load().nrx_bag_upstream_rows(gb.ptr, g_out.shape[1], col, dim, batch, sb.ptr if with_scale else None, copies, stride, dst.ptr,
                                          _stream()), "nrx_bag_upstream_rows")
    gb.unchanged()
    sb.unchanged()
    got = dst.read()
    want = P.upstream_rows(g_out, col, dim, scale if with_scale else None, copies)
    for c in range(copies):
        assert P.same_bits(got[c * stride:c * stride + batch * dim].reshape(batch, dim), want[c]), c
        if c:
            assert (got[c * stride - gap:c * stride].view(np.uint8) == 0xFF).all(), c                # the gap between two copies
    if not with_scale:
        assert P.same_bits(got[:batch * dim].reshape(batch, dim), g_out[:, col:col + dim])


@pytest.mark.parametrize("case", P.UPSTREAM_CASES + [P.UPSTREAM_WRAP], ids=lambda c: "-".join(str(int(x)) for x in c))
def test_upstream_rows_bit_for_bit(case):
    _upstream(*case)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("lens", [P.KEYS_LENS_SMALL, P.KEYS_LENS_WRAP], ids=["small", "wrap"])
def test_make_table_keys_equals_its_definition(bits, lens):
    ids = P.keys_inputs(bits, lens)
    bufs = [Buf(x) if x.size else None for x in ids]
    keys = Buf(shape=(sum(lens),), dtype=np.int64)
    _ok(_lib.load().nrx_make_table_keys(_parr([b.ptr if b else None for b in bufs]), _i64(lens), _i32(P.KEYS_TABLE_OF), len(lens), bits, keys.ptr,
                                        _stream()), "nrx_make_table_keys")
    for b in bufs:
        if b:
            b.unchanged()
    assert np.array_equal(keys.read(), P.table_keys(ids, P.KEYS_TABLE_OF))


# ------------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_and_write_nothing():
    lib = _lib.load()
    dim = 16
    ib = P.case_inbox(dim, "main")
    d, g = DevInbox(ib), Buf(P.case_g_partial(ib))
    tables = [Buf(t) for t in P.case_tables(dim)]
    tables16 = [Buf(t) for t in P.bf16_tables(dim)[0]]
    n = ib.world * ib.cap
    o = dict(partial=Buf(shape=(ib.world, ib.ntag, dim), dtype=F32), ws=Buf(shape=(ib.world, ib.ntag, 2), dtype=np.int32),
             grad0=Buf(shape=(ib.table_rows[0], dim), dtype=F32), grad1=Buf(shape=(ib.table_rows[1], dim), dtype=F32),
             oid=Buf(shape=(n,), dtype=np.int32), g_rows=Buf(shape=(n, dim), dtype=F32), pay=Buf(shape=(n,), dtype=np.uint32),
             tag_out=Buf(shape=(n,), dtype=np.int32), out_w=Buf(shape=(5, 6), dtype=F32), inv=Buf(shape=(5,), dtype=F32),
             dst=Buf(shape=(3 * 5 * 4,), dtype=F32), keys=Buf(shape=(10,), dtype=np.int64), order=Buf(shape=(n,), dtype=np.int64))
    mask, ids = Buf(np.ones((5, 6), F32)), Buf(np.arange(10, dtype=np.int32))
    base = dict(tables=[b.ptr for b in tables], tables16=[b.ptr for b in tables16], grads=[o["grad0"].ptr, o["grad1"].ptr], table_rows=ib.table_rows,
                n_tables=2, feat_table=ib.feat_table, n_feats=ib.n_feats, batch=ib.batch, world=ib.world, cap=ib.cap, recv=d.recv.ptr,
                rows=d.rows.ptr, tag=d.tag.ptr, w=d.w.ptr, run=d.run.ptr, dim=dim, partial=o["partial"].ptr, ws=o["ws"].ptr, g=g.ptr,
                oid=o["oid"].ptr, g_rows=o["g_rows"].ptr, pay=o["pay"].ptr, tag_out=o["tag_out"].ptr, one_rows=150)

    def common(a, tables="tables"):
        return (_parr(a[tables]), _i64(a["table_rows"]), a["n_tables"], _i32(a["feat_table"]), a["n_feats"], a["batch"], a["world"], a["cap"],
                a["recv"], a["rows"])

    def single(a):
        return (a["one_rows"], a["n_feats"], a["batch"], a["world"], a["cap"], a["recv"], a["rows"])

    calls = {
        "nrx_pool_inbox_fwd": lambda a: lib.nrx_pool_inbox_fwd(*common(a), a["tag"], a["w"], a["dim"], a["partial"], a["ws"], None, _stream()),
        "nrx_pool_inbox_fwd_bf16": lambda a: lib.nrx_pool_inbox_fwd_bf16(*common(a, "tables16"), a["tag"], a["w"], a["dim"], a["partial"], a["ws"],
                                                                         None, _stream()),
        "nrx_pool_inbox_fwd_runs": lambda a: lib.nrx_pool_inbox_fwd_runs(*common(a), a["w"], a["run"], a["dim"], a["partial"], None, _stream()),
        "nrx_pool_inbox_fwd_runs_bf16": lambda a: lib.nrx_pool_inbox_fwd_runs_bf16(*common(a, "tables16"), a["w"], a["run"], a["dim"], a["partial"],
                                                                                   None, _stream()),
        "nrx_pool_inbox_bwd": lambda a: lib.nrx_pool_inbox_bwd(*common(a, "grads"), a["tag"], a["w"], a["dim"], a["g"], 0, _stream()),
        "nrx_pool_inbox_expand": lambda a: lib.nrx_pool_inbox_expand(*single(a), a["tag"], a["w"], a["dim"], a["g"], 0, a["oid"], a["g_rows"],
                                                                     _stream()),
        "nrx_pool_inbox_owner_ids": lambda a: lib.nrx_pool_inbox_owner_ids(*single(a), a["tag"], 0, a["oid"], a["pay"], _stream()),
        "nrx_pool_inbox_runs_words": lambda a: lib.nrx_pool_inbox_runs_words(*single(a), a["run"], 0, a["tag_out"], a["oid"], a["pay"], _stream()),
    }
    every = list(calls)
    with_dim = every[:6]
    with_tables = every[:5]
    bad = [(nm, dict(batch=0)) for nm in every] + [(nm, dict(world=65)) for nm in every] + [(nm, dict(world=0)) for nm in every]
    bad += [(nm, dict(cap=0)) for nm in every] + [(nm, dict(n_feats=0)) for nm in every]
    bad += [(nm, dict(dim=0)) for nm in with_dim] + [(nm, dict(dim=1025)) for nm in with_dim]
    bad += [(nm, {k: None}) for nm in every for k in ("recv", "rows")]
    bad += [(nm, dict(tag=None)) for nm in ("nrx_pool_inbox_fwd", "nrx_pool_inbox_fwd_bf16", "nrx_pool_inbox_bwd", "nrx_pool_inbox_expand",
                                            "nrx_pool_inbox_owner_ids")]
    bad += [(nm, dict(w=None)) for nm in with_dim]
    bad += [(nm, dict(run=None)) for nm in ("nrx_pool_inbox_fwd_runs", "nrx_pool_inbox_fwd_runs_bf16", "nrx_pool_inbox_runs_words")]
    bad += [(nm, dict(partial=None)) for nm in every[:4]] + [(nm, dict(ws=None)) for nm in every[:2]]
    bad += [(nm, dict(feat_table=[1, 2, 0])) for nm in with_tables] + [(nm, dict(feat_table=[0, -1, 0])) for nm in with_tables]
    bad += [(nm, dict(n_tables=0)) for nm in with_tables] + [(nm, dict(n_tables=65)) for nm in with_tables]
    bad += [(nm, dict(tables=[base["tables"][0], None], grads=[base["grads"][0], None], tables16=[base["tables16"][0], None])) for nm in with_tables]
    bad += [(nm, dict(tables=[base["tables"][0] + 4, base["tables"][1]])) for nm in ("nrx_pool_inbox_fwd", "nrx_pool_inbox_fwd_runs")]
    bad += [(nm, dict(tables16=[base["tables16"][0], base["tables16"][1] + 2])) for nm in ("nrx_pool_inbox_fwd_bf16", "nrx_pool_inbox_fwd_runs_bf16")]
    bad += [("nrx_pool_inbox_bwd", dict(grads=[base["grads"][0] + 4, base["grads"][1]])), ("nrx_pool_inbox_bwd", dict(g=None)),
            ("nrx_pool_inbox_expand", dict(g=None)), ("nrx_pool_inbox_expand", dict(oid=None)), ("nrx_pool_inbox_expand", dict(g=base["g"] + 4)),
            ("nrx_pool_inbox_expand", dict(g_rows=base["g_rows"] + 4)), ("nrx_pool_inbox_owner_ids", dict(oid=None)),
            ("nrx_pool_inbox_runs_words", dict(tag_out=None, oid=None, pay=None)), ("nrx_pool_inbox_runs_words", dict(oid=None))]
    for nm, over in bad:
        assert calls[nm](dict(base, **over)) == NRX_ERR_BAD_ARG, (nm, over)
        assert nm.encode() in lib.nrx_last_error(), (nm, over, lib.nrx_last_error())

    m, s = mask.ptr, _stream()
    small = [
        ("nrx_bag_norm_weights", lambda: lib.nrx_bag_norm_weights(m, 5, 6, NRX_BAG_MASKED_MEAN, None, s)),
        ("nrx_bag_norm_weights", lambda: lib.nrx_bag_norm_weights(None, 5, 6, NRX_BAG_MASKED_MEAN, o["out_w"].ptr, s)),
        ("nrx_bag_norm_weights", lambda: lib.nrx_bag_norm_weights(m, 5, 0, NRX_BAG_MEAN, o["out_w"].ptr, s)),
        ("nrx_bag_norm_weights", lambda: lib.nrx_bag_norm_weights(m, -1, 6, NRX_BAG_MEAN, o["out_w"].ptr, s)),
        ("nrx_bag_norm_weights", lambda: lib.nrx_bag_norm_weights(m, 5, 6, 1, o["out_w"].ptr, s)),
        ("nrx_bag_norm_weights_inv", lambda: lib.nrx_bag_norm_weights_inv(m, 5, 6, NRX_BAG_SUM, o["out_w"].ptr, None, s)),
        ("nrx_bag_norm_weights_inv", lambda: lib.nrx_bag_norm_weights_inv(m, 5, 6, NRX_BAG_SUM, None, o["inv"].ptr, s)),
        ("nrx_bag_norm_weights_inv", lambda: lib.nrx_bag_norm_weights_inv(None, 5, 6, NRX_BAG_MASKED_MEAN, o["out_w"].ptr, o["inv"].ptr, s)),
        ("nrx_bag_norm_weights_inv", lambda: lib.nrx_bag_norm_weights_inv(m, 5, 6, 0, o["out_w"].ptr, o["inv"].ptr, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(None, 6, 1, 4, 5, None, 1, 0, o["dst"].ptr, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, 1, 4, 5, None, 1, 0, None, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, 1, 0, 5, None, 1, 0, o["dst"].ptr, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, -1, 4, 5, None, 1, 0, o["dst"].ptr, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, 3, 4, 5, None, 1, 0, o["dst"].ptr, s)),           # ld < col + dim
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, 1, 4, 5, None, 0, 20, o["dst"].ptr, s)),
        ("nrx_bag_upstream_rows", lambda: lib.nrx_bag_upstream_rows(m, 6, 1, 4, 5, None, 3, 19, o["dst"].ptr, s)),          # copies > 1, stride < batch dim
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([ids.ptr]), _i64([10]), _i32([0]), 0, 32, o["keys"].ptr, s)),
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([ids.ptr]), _i64([10]), _i32([0]), 1, 16, o["keys"].ptr, s)),
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([ids.ptr]), _i64([-1]), _i32([0]), 1, 32, o["keys"].ptr, s)),
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([None]), _i64([10]), _i32([0]), 1, 32, o["keys"].ptr, s)),
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([ids.ptr]), _i64([10]), _i32([1 << 20]), 1, 32, o["keys"].ptr, s)),
        ("nrx_make_table_keys", lambda: lib.nrx_make_table_keys(_parr([ids.ptr]), _i64([10]), _i32([0]), 1, 32, None, s)),
        ("nrx_pool_order_remap", lambda: lib.nrx_pool_order_remap(None, n, d.tag.ptr, ib.cap, ib.ntag, ib.world, s)),
        ("nrx_pool_order_remap", lambda: lib.nrx_pool_order_remap(o["order"].ptr, n, None, ib.cap, ib.ntag, ib.world, s)),
        ("nrx_pool_order_remap", lambda: lib.nrx_pool_order_remap(o["order"].ptr, n, d.tag.ptr, 0, ib.ntag, ib.world, s)),
        ("nrx_pool_order_remap", lambda: lib.nrx_pool_order_remap(o["order"].ptr, -1, d.tag.ptr, ib.cap, ib.ntag, ib.world, s)),
    ]
    for nm, call in small:
        assert call() == NRX_ERR_BAD_ARG, nm
        assert nm.encode() in lib.nrx_last_error(), (nm, lib.nrx_last_error())
    # batch == 0 / nothing to do: NRX_OK and nothing written
    assert lib.nrx_bag_norm_weights(m, 0, 6, NRX_BAG_MASKED_MEAN, o["out_w"].ptr, s) == NRX_OK
    assert lib.nrx_bag_norm_weights_inv(m, 0, 6, NRX_BAG_MASKED_MEAN, o["out_w"].ptr, o["inv"].ptr, s) == NRX_OK
    assert lib.nrx_bag_upstream_rows(m, 6, 1, 4, 0, None, 1, 0, o["dst"].ptr, s) == NRX_OK
    assert lib.nrx_make_table_keys(_parr([None]), _i64([0]), _i32([0]), 1, 32, o["keys"].ptr, s) == NRX_OK
    assert lib.nrx_pool_order_remap(o["order"].ptr, 0, d.tag.ptr, ib.cap, ib.ntag, ib.world, s) == NRX_OK
    for b in o.values():
        _untouched(b)
    d.unchanged()
    # the same buffers with good arguments: every call goes through
    for b in (o["grad0"], o["grad1"]):
        b.t.zero_()
    for nm, call in calls.items():
        _ok(call(base), nm)
    _ok(calls["nrx_pool_inbox_fwd"](base), "nrx_pool_inbox_fwd")
    assert P.same_bits(o["partial"].read(), _fwd_ref(dim, "main")[0])
