"""The fixed-capacity exchange kernels of csrc/nrx_route.hip alone, through the C ABI (nrx_route_ids, nrx_route_ids_pos, nrx_gather_inbox,
nrx_gather_inbox_place, nrx_scatter_add_inbox), at the edges of their launch arithmetic: one, two and three steps of route_scan, owners on a
later wavefront trip, features of 0 / 1 / 2047 / 2048 / 2049 ids, 64 features, a block that overflows by one, ids that are no rows; the classic
inbox kernel at every lane-group width with float4 and scalar rows and a second trip over the columns; the ring gather at every width with
busy and idle lanes, at exactly 512 work items beside its classic neighbour of 504, and past the wrap of its persistent grid; the placing
gather into per-source buffers.  Against the definitions of tests/route_inbox_ref.py (held to oracle/ref_np.py by tests/test_route_inbox_ref.py).

Everything is exact: integer words equal the definition, gathered rows are the table rows bit for bit, and the scatter-add works on small
integers whose every sum of |terms| stays below 2^24, so the float atomics are exact in any order and owe the int64 result bit for bit.
Every device buffer is the body of a larger allocation of fill bytes (0xFF for floats: NaN; 0x7F for integers: 0x7f7f7f7f, which is neither
-1 nor a slot); outputs start as fill throughout.  After a call the margins and every word the definition leaves alone still hold the fill."""
import ctypes as C

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib
from news_recsys_amd._lib import NRX_ERR_BAD_ARG, NRX_ERR_UNSUPPORTED, NRX_OK
from tests import route_inbox_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1024                             # bytes in front of a body (it stays 16-byte aligned) and at least as many behind
IFILL = 0x7F7F7F7F
TORCH = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}


class Dev:
    """A body of `shape` elements inside a device allocation of fill bytes (0xFF for float32, 0x7F for integers); `off` elements more in front
    (a body that is only element-aligned); `tail` bytes more behind.  data=None: an output, fill throughout."""

    def __init__(self, data=None, shape=None, dtype=None, off=0, tail=0):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        self.shape, self.dtype = tuple(int(x) for x in shape), np.dtype(dtype)
        self.fill = 0xFF if self.dtype == np.float32 else 0x7F
        n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.lo = MARGIN + off * self.dtype.itemsize
        self.hi = self.lo + n
        self.t = torch.full((self.hi + MARGIN + tail + (-self.hi) % 8,), self.fill, dtype=torch.uint8, device=DEV)
        self.body = self.t[self.lo:self.hi].view(TORCH[self.dtype]).view(self.shape)
        self.t0 = None
        if data is not None:
            self.body.copy_(torch.from_numpy(data))
            self.t0 = self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lo

    def bits(self):
        return self.body.view(torch.int32) if self.dtype == np.float32 else self.body

    def margins_ok(self):
        torch.cuda.synchronize()
        assert bool((self.t[:self.lo] == self.fill).all()) and bool((self.t[self.hi:] == self.fill).all()), "a byte outside the body was written"

    def read(self):
        self.margins_ok()
        return self.body.cpu().numpy()

    def unchanged(self):
        torch.cuda.synchronize()
        ref = self.t0 if self.t0 is not None else torch.full_like(self.t, self.fill)
        assert torch.equal(self.t, ref), "an input, or an output of a refused call, was written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == NRX_OK, (what, rc, _lib.load().nrx_last_error())
    torch.cuda.synchronize()


def _parr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


def _i32(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


# ------------------------------------------------------------------------------------------------- routing
def route(ids, world, cap, view=0, pos=True, overflow=None):
    """One call of nrx_route_ids_pos (pos) or nrx_route_ids on fresh fill-initialised outputs.  The id arrays are untouched afterwards."""
    lib = _lib.load()
    n = sum(a.size for a in ids)
    bufs = [Dev(a, off=view) if a.size else None for a in ids]
    o = dict(send_rows=Dev(shape=(world * cap,), dtype=np.int32), send_pos=Dev(shape=(world * cap,), dtype=np.int32),
             slot=Dev(shape=(n,), dtype=np.int32), counts2d=Dev(shape=(world, len(ids)), dtype=np.int64),
             ws=Dev(shape=(lib.nrx_route_workspace(n, world),), dtype=np.int64))
    o["overflow"] = overflow if overflow is not None else Dev(np.zeros(1, np.int64))
    head = (_parr([b.ptr if b else None for b in bufs]), _i64([a.size for a in ids]), len(ids), ids[0].dtype.itemsize * 8, world, cap)
    if pos:
        _ok(lib.nrx_route_ids_pos(*head, o["send_rows"].ptr, o["send_pos"].ptr, o["slot"].ptr, o["counts2d"].ptr, o["overflow"].ptr, o["ws"].ptr,
                                  _stream()), "nrx_route_ids_pos")
    else:
        _ok(lib.nrx_route_ids(*head, o["send_rows"].ptr, o["slot"].ptr, o["counts2d"].ptr, o["overflow"].ptr, o["ws"].ptr, _stream()), "nrx_route_ids")
    for b in bufs:
        if b:
            b.unchanged()
    o["ws"].margins_ok()
    return o


@pytest.mark.parametrize("name", sorted(P.route_cases()))
def test_route_every_word_equals_the_definition(name):
    ids, world, cap, view = P.route_case(name)
    want = P.route_def(ids, world, cap, IFILL)
    for pos in (True, False):
        o = route(ids, world, cap, view, pos)
        assert np.array_equal(o["counts2d"].read(), want.counts2d), (name, pos)
        assert o["overflow"].read()[0] == want.worst, (name, pos)
        assert np.array_equal(o["slot"].read(), want.slot), (name, pos)
        assert np.array_equal(o["send_rows"].read(), want.send_rows), (name, pos)       # (the slots past a block's count hold the fill still)
        if pos:
            assert np.array_equal(o["send_pos"].read(), want.send_pos), name
        else:
            o["send_pos"].unchanged()


def test_overflow_word_is_a_running_maximum():
    a, b = P.route_case("w2-view"), P.route_case("w5-over1")
    wa, wb = P.route_def(*a[:3], 0).worst, P.route_def(*b[:3], 0).worst
    assert wa > wb > 0
    word = Dev(np.zeros(1, np.int64))
    route(*b, overflow=word)
    assert word.read()[0] == wb
    route(*a, overflow=word)
    assert word.read()[0] == wa                                          # a larger block count raises it
    route(*b, overflow=word)
    assert word.read()[0] == wa                                          # a smaller one leaves it
    one = P.route_case("w1-over")                                        # route_single: the total, held against the same word
    route(*one, overflow=word)
    assert word.read()[0] == max(wa, sum(x.size for x in one[0]))
    word = Dev(np.full(1, 1 << 40, np.int64))
    route(*one, overflow=word)
    assert word.read()[0] == 1 << 40


# ------------------------------------------------------------------------------------------------- owner side: helpers
def make_tables(dim, off=0):
    """Two tables of P.TABLE_ROWS rows, each the head of a NaN allocation that reaches more than a row past its end."""
    gen = torch.Generator().manual_seed(dim)
    return [Dev(torch.randn((r, dim), generator=gen).numpy(), off=off, tail=4 * dim) for r in P.TABLE_ROWS]


class DevInbox:
    def __init__(self, ib):
        self.ib = ib
        self.rows, self.pos, self.recv = Dev(ib.rows), Dev(ib.pos), Dev(ib.recv2d)

    def head(self, tables):
        ib = self.ib
        return (_parr([t.ptr for t in tables]), _i64(ib.table_rows), len(tables), _i32(ib.feat_table), ib.n_feats, ib.world, ib.cap, self.recv.ptr,
                self.rows.ptr)

    def unchanged(self):
        for b in (self.rows, self.pos, self.recv):
            b.unchanged()


def _dev_idx(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(DEV)


def expected_rows(g, tables, n_slots, dim):
    """The definition's out_rows as bits, built on the device: 0xFF words but for slot flat[i] <- tables[tab[i]][row[i]]."""
    exp = torch.full((n_slots, dim), -1, dtype=torch.int32, device=DEV)
    for t, T in enumerate(tables):
        sel = g.tab == t
        exp[_dev_idx(g.flat[sel])] = T.bits()[_dev_idx(g.row[sel])]
    return exp


def check_status(st, n, reports, what):
    if n == 0:
        assert st.tolist() == [0, 0, 0, 0], (what, st)
    else:                                                                # one count per offender; the first to arrive leaves (table, slot, word)
        assert st[0] == n and tuple(int(x) for x in st[1:]) in reports, (what, st, n)


def gather(ib, tables, dim, off=0):
    """nrx_gather_inbox into a NaN buffer: (out Dev, DevInbox).  Asserts the status words, that inputs and tables are untouched."""
    d, out, st = DevInbox(ib), Dev(shape=(ib.world * ib.cap, dim), dtype=np.float32, off=off), Dev(np.zeros(4, np.int32))
    _ok(_lib.load().nrx_gather_inbox(*d.head(tables), dim, out.ptr, st.ptr, _stream()), "nrx_gather_inbox")
    d.unchanged()
    for t in tables:
        t.unchanged()
    g = P.gather_index(ib)
    check_status(st.read(), int(g.bad.sum()), g.reports, (dim, ib.world))
    return out, g


def check_gather(ib, tables, dim, off=0):
    out, g = gather(ib, tables, dim, off)
    assert torch.equal(out.bits(), expected_rows(g, tables, ib.world * ib.cap, dim)), (dim, ib.world, ib.cap)
    out.margins_ok()
    return out


# ------------------------------------------------------------------------------------------------- classic form
@pytest.mark.parametrize("dim", P.CLASSIC_DIMS)
def test_classic_gather_rows_bit_for_bit_and_nothing_else_written(dim):
    off = 1 if dim % 4 else 0                                            # odd widths: tables and rows only 4-byte aligned
    tables = make_tables(dim, off)
    for name in P.classic_cases(dim):
        ib = P.classic_case(dim, name)
        assert P.form(dim, ib.cap, ib.world) == "classic"
        check_gather(ib, tables, dim, off)
    ib = P.classic_case(dim, "w3-f3")                                    # status = NULL: the same rows, nothing reported
    d, out = DevInbox(ib), Dev(shape=(ib.world * ib.cap, dim), dtype=np.float32)
    if off == 0:
        _ok(_lib.load().nrx_gather_inbox(*d.head(tables), dim, out.ptr, None, _stream()), "nrx_gather_inbox without status")
        assert torch.equal(out.bits(), expected_rows(P.gather_index(ib), tables, ib.world * ib.cap, dim))


@pytest.mark.parametrize("dim", P.CLASSIC_DIMS)
def test_scatter_add_equals_the_int64_sum_bit_for_bit(dim):
    lib = _lib.load()
    rng = np.random.default_rng(dim)
    for name in P.classic_cases(dim):
        ib = P.classic_case(dim, name, garbage_row=1)                    # the slots past a count name a row that exists ...
        n = ib.world * ib.cap
        flat, _ = P.slot_features(ib)
        g_rows = np.full((n, dim), np.nan, np.float32)                   # ... and carry NaN: reading one poisons the table
        g_rows[flat] = rng.integers(-3, 4, (flat.size, dim))
        start = [rng.integers(-5, 6, (r, dim)).astype(np.float32) for r in ib.table_rows]
        d, gb = DevInbox(ib), Dev(g_rows)
        for skip_row0 in (0, 1):
            want, mag = P.scatter_def(ib, np.nan_to_num(g_rows), start, skip_row0)
            assert max(int(m.max()) for m in mag) < 1 << 24             # every partial sum is an integer below 2^24: exact in any order
            grads = [Dev(t) for t in start]
            _ok(lib.nrx_scatter_add_inbox(*d.head(grads), dim, gb.ptr, skip_row0, _stream()), "nrx_scatter_add_inbox")
            d.unchanged()
            gb.unchanged()
            for t in range(len(grads)):
                got = grads[t].read()
                assert not np.isnan(got).any() and np.array_equal(got.astype(np.int64), want[t]), (dim, name, skip_row0, t)
                assert np.array_equal(got, want[t].astype(np.float32)), (dim, name, skip_row0, t)
            if skip_row0:
                assert all(np.array_equal(grads[t].read()[0], start[t][0]) for t in range(len(grads))), (dim, name)


# ------------------------------------------------------------------------------------------------- ring form
@pytest.mark.parametrize("dim", P.RING_DIMS)
def test_ring_gather_at_512_items_and_its_classic_neighbour_give_the_definitions_bits(dim):
    tables = make_tables(dim)
    ring, classic = P.ring_case(dim, 64), P.ring_case(dim, 63)
    assert P.form(dim, ring.cap, 64) == "ring" and P.form(dim, classic.cap, 63) == "classic" and P.cps(dim, ring.cap) * 64 == P.RING_MIN_ITEMS
    a = check_gather(ring, tables, dim)
    b = check_gather(classic, tables, dim)
    assert torch.equal(a.bits()[:63 * ring.cap], b.bits())


@pytest.mark.parametrize("dim", P.WRAP_DIMS)
def test_ring_gather_past_the_wrap_of_its_persistent_grid(dim):
    ib = P.wrap_case(dim)
    assert P.cps(dim, ib.cap) * 64 == 1600 > P.ring_grid(dim, ib.cap, 64) and P.form(dim, ib.cap, 64) == "ring"
    check_gather(ib, make_tables(dim), dim)


# ------------------------------------------------------------------------------------------------- placing form
def place(ib, tables, dim, live_only=False):
    """nrx_gather_inbox_place: every source writes into its own NaN buffer [out_rows, out_ld] (live_only: the sources without an entry share one
    buffer, which must stay NaN).  Compares every buffer with the definition, bit for bit, fill included."""
    d, st = DevInbox(ib), Dev(np.zeros(4, np.int32))
    g = P.place_index(ib)
    live = set(np.unique(g.src).tolist())
    shared = Dev(shape=(4, ib.out_ld), dtype=np.float32)
    outs = [Dev(shape=(ib.out_rows, ib.out_ld), dtype=np.float32) if (s in live or not live_only) else shared for s in range(ib.world)]
    _ok(_lib.load().nrx_gather_inbox_place(*d.head(tables), d.pos.ptr, dim, _parr([o.ptr for o in outs]), ib.out_ld, ib.out_rows, _i32(ib.feat_col),
                                           st.ptr, _stream()), "nrx_gather_inbox_place")
    d.unchanged()
    for t in tables:
        t.unchanged()
    check_status(st.read(), g.n_reports, g.reports, (dim, ib.world, ib.cap))
    shared.unchanged()
    for s in range(ib.world):
        if outs[s] is shared:
            continue
        exp = torch.full((ib.out_rows, ib.out_ld), -1, dtype=torch.int32, device=DEV)
        for f in range(ib.n_feats):
            sel = (g.src == s) & (g.feat == f) & ~g.dropped
            c = ib.feat_col[f]
            exp[_dev_idx(g.at[sel]), c:c + dim] = tables[ib.feat_table[f]].bits()[_dev_idx(g.row[sel])]
        assert torch.equal(outs[s].bits(), exp), (dim, s)
        outs[s].margins_ok()


@pytest.mark.parametrize("dim", P.PLACE_DIMS)
def test_placing_gather_puts_every_row_where_the_definition_does(dim):
    tables = make_tables(dim)
    for name in P.place_cases(dim):
        place(P.place_case(dim, name), tables, dim)


@pytest.mark.parametrize("dim", P.WRAP_DIMS)
def test_placing_gather_past_the_wrap(dim):
    I = P.ring_item(dim)
    ib = P.wrap_case(dim, out_rows=(P.WRAP_CPS - 1) * I + 1)
    ib.feat_col, ib.out_ld = [dim + 4, 0], 2 * dim + 8
    place(ib, make_tables(dim), dim, live_only=True)


# ------------------------------------------------------------------------------------------------- refusals
def test_route_refusals_enqueue_and_write_nothing():
    lib = _lib.load()
    ids = [np.arange(10, dtype=np.int32), np.arange(5, dtype=np.int32)]
    bufs = [Dev(a) for a in ids]
    world, cap = 2, 16
    o = dict(send_rows=Dev(shape=(world * cap,), dtype=np.int32), send_pos=Dev(shape=(world * cap,), dtype=np.int32), slot=Dev(shape=(15,), dtype=np.int32),
             counts2d=Dev(shape=(world, 2), dtype=np.int64), overflow=Dev(shape=(1,), dtype=np.int64),
             ws=Dev(shape=(lib.nrx_route_workspace(15, 64),), dtype=np.int64))
    base = dict(ids=[b.ptr for b in bufs], lens=[10, 5], n_feats=2, bits=32, world=world, cap=cap, **{k: v.ptr for k, v in o.items()})

    def call(a, pos):
        head = (_parr(a["ids"]), _i64(a["lens"]), a["n_feats"], a["bits"], a["world"], a["cap"], a["send_rows"])
        tail = (a["slot"], a["counts2d"], a["overflow"], a["ws"], _stream())
        return lib.nrx_route_ids_pos(*head, a["send_pos"], *tail) if pos else lib.nrx_route_ids(*head, *tail)

    bad = {"world 0": dict(world=0), "world 65": dict(world=65), "cap 0": dict(cap=0), "cap * world = 2^31": dict(cap=1 << 30),
           "n_feats 0": dict(n_feats=0), "n_feats 65": dict(n_feats=65), "index_bits 16": dict(bits=16), "null send_rows": dict(send_rows=None),
           "null slot": dict(slot=None), "negative length": dict(lens=[10, -1]), "null ids with a length": dict(ids=[base["ids"][0], None]),
           "null counts2d": dict(counts2d=None), "null overflow": dict(overflow=None), "null workspace": dict(ws=None)}
    assert set(P.ROUTE_REFUSALS) - {"null send_pos"} <= set(bad)
    for what, over in bad.items():
        for pos in (False, True):
            assert call(dict(base, **over), pos) == NRX_ERR_BAD_ARG, (what, pos)
            assert b"nrx_route_ids" in lib.nrx_last_error(), (what, lib.nrx_last_error())
    assert call(dict(base, send_pos=None), True) == NRX_ERR_BAD_ARG and b"nrx_route_ids_pos" in lib.nrx_last_error()
    for b in list(o.values()) + bufs:
        b.unchanged()
    o["overflow"].body.zero_()                                           # the same buffers with good arguments go through
    _ok(call(base, True), "nrx_route_ids_pos")
    want = P.route_def(ids, world, cap, IFILL)
    assert np.array_equal(o["send_rows"].read(), want.send_rows) and np.array_equal(o["send_pos"].read(), want.send_pos)
    assert np.array_equal(o["slot"].read(), want.slot) and o["overflow"].read()[0] == want.worst


def test_inbox_refusals_enqueue_and_write_nothing():
    lib = _lib.load()
    dim = 16
    ib = P.place_case(dim, "w3")
    n = ib.world * ib.cap
    d, tables = DevInbox(ib), make_tables(dim)
    g_rows = Dev(np.ones((n, dim), np.float32))
    o = dict(out=Dev(shape=(n, dim), dtype=np.float32), st=Dev(shape=(4,), dtype=np.int32), grad0=Dev(shape=(P.TABLE_ROWS[0], dim), dtype=np.float32),
             grad1=Dev(shape=(P.TABLE_ROWS[1], dim), dtype=np.float32), wide=Dev(shape=(n, 264), dtype=np.float32),
             **{f"peer{s}": Dev(shape=(ib.out_rows, ib.out_ld), dtype=np.float32) for s in range(ib.world)})
    base = dict(tables=[t.ptr for t in tables], grads=[o["grad0"].ptr, o["grad1"].ptr], table_rows=ib.table_rows, n_tables=2, feat_table=ib.feat_table,
                n_feats=ib.n_feats, world=ib.world, cap=ib.cap, recv=d.recv.ptr, rows=d.rows.ptr, pos=d.pos.ptr, dim=dim, out=o["out"].ptr,
                st=o["st"].ptr, g_rows=g_rows.ptr, peers=[o[f"peer{s}"].ptr for s in range(ib.world)], out_ld=ib.out_ld, out_rows=ib.out_rows,
                feat_col=ib.feat_col)

    def head(a, tables="tables"):
        return (_parr(a[tables]), _i64(a["table_rows"]), a["n_tables"], _i32(a["feat_table"]), a["n_feats"], a["world"], a["cap"], a["recv"], a["rows"])

    calls = {
        "nrx_gather_inbox": lambda a: lib.nrx_gather_inbox(*head(a), a["dim"], a["out"], a["st"], _stream()),
        "nrx_scatter_add_inbox": lambda a: lib.nrx_scatter_add_inbox(*head(a, "grads"), a["dim"], a["g_rows"], 0, _stream()),
        "nrx_gather_inbox_place": lambda a: lib.nrx_gather_inbox_place(*head(a), a["pos"], a["dim"], _parr(a["peers"]), a["out_ld"], a["out_rows"],
                                                                     _i32(a["feat_col"]), a["st"], _stream()),
    }
    common = {"world 0": dict(world=0), "world 65": dict(world=65), "cap 0": dict(cap=0), "n_feats 0": dict(n_feats=0), "n_feats 65": dict(n_feats=65),
              "feat_table out of range": dict(feat_table=[1, 2, 0]), "feat_table negative": dict(feat_table=[0, -1, 0]),
              "null table": dict(tables=[base["tables"][0], None], grads=[base["grads"][0], None]),
              "misaligned table": dict(tables=[base["tables"][0] + 4, base["tables"][1]], grads=[base["grads"][0], base["grads"][1] + 8]),
              "null recv2d": dict(recv=None), "null inbox": dict(rows=None), "dim 0": dict(dim=0), "n_tables 0": dict(n_tables=0),
              "n_tables 65": dict(n_tables=65)}
    assert set(P.INBOX_REFUSALS) <= set(common)
    for nm, fn in calls.items():
        for what, over in common.items():
            assert fn(dict(base, **over)) == NRX_ERR_BAD_ARG, (nm, what)
            assert nm.encode() in lib.nrx_last_error(), (nm, what, lib.nrx_last_error())
    one = [("nrx_gather_inbox", dict(out=None)), ("nrx_gather_inbox", dict(out=base["out"] + 4)), ("nrx_scatter_add_inbox", dict(g_rows=None))]
    for nm, over in one:
        assert calls[nm](dict(base, **over)) == NRX_ERR_BAD_ARG and nm.encode() in lib.nrx_last_error(), (nm, over)
    peers = base["peers"]
    placing = {"dim 8": (dict(dim=8), NRX_ERR_UNSUPPORTED), "dim 18": (dict(dim=18), NRX_ERR_UNSUPPORTED),
               "dim 260": (dict(dim=260, out_ld=264, feat_col=[0, 0, 0], peers=[o["wide"].ptr] * 3), NRX_ERR_UNSUPPORTED),
               "out_ld % 4": (dict(out_ld=ib.out_ld + 2), NRX_ERR_UNSUPPORTED), "out_ld < dim": (dict(out_ld=12), NRX_ERR_BAD_ARG),
               "feat_col % 4": (dict(feat_col=[0, 18, 36]), NRX_ERR_BAD_ARG), "feat_col negative": (dict(feat_col=[0, -4, 36]), NRX_ERR_BAD_ARG),
               "feat_col + dim > out_ld": (dict(feat_col=[0, 16, ib.out_ld - dim + 4]), NRX_ERR_BAD_ARG),
               "misaligned peer_out": (dict(peers=[peers[0], peers[1] + 4, peers[2]]), NRX_ERR_BAD_ARG),
               "null peer_out": (dict(peers=[peers[0], peers[1], None]), NRX_ERR_BAD_ARG), "null inbox_pos": (dict(pos=None), NRX_ERR_BAD_ARG),
               "out_rows negative": (dict(out_rows=-1), NRX_ERR_BAD_ARG)}
    assert set(P.PLACE_REFUSALS) <= set(placing)
    for what, (over, code) in placing.items():
        assert calls["nrx_gather_inbox_place"](dict(base, **over)) == code, what
        assert b"nrx_gather_inbox_place" in lib.nrx_last_error(), (what, lib.nrx_last_error())
    for b in o.values():
        b.unchanged()
    d.unchanged()
    o["st"].body.zero_()                                                 # the same buffers with good arguments go through
    _ok(calls["nrx_gather_inbox"](base), "nrx_gather_inbox")
    assert torch.equal(o["out"].bits(), expected_rows(P.gather_index(ib), tables, n, dim))
    _ok(calls["nrx_gather_inbox_place"](base), "nrx_gather_inbox_place")
    for k in ("grad0", "grad1"):
        o[k].body.zero_()
    _ok(calls["nrx_scatter_add_inbox"](base), "nrx_scatter_add_inbox")
    want, _ = P.scatter_def(ib, np.ones((n, dim)), [np.zeros((r, dim)) for r in P.TABLE_ROWS], 0)
    assert all(np.array_equal(o[k].read().astype(np.int64), w) for k, w in zip(("grad0", "grad1"), want))
