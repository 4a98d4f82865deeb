"""The per-feature channel of the sharded step (csrc/nrx_route_feat.hip: nrx_route_feat, nrx_inbox_transpose, nrx_gather_place_feat(_bf16),
nrx_shard_dest_combine) and the direct-gradient backward's entry points (csrc/nrx_embed.hip: nrx_embed_bwd_scatter_multi, nrx_embed_bwd_walk)
alone, through the C ABI, at the edges of their launch arithmetic: every lane-group width of the placing gather (dim 16 .. 256), 1 / 8 / 9 / 16 /
17 / 24 / 25 / 64 features (one chunk of GP_R = 8, two, the first refill of the first register set, the refill after it, NRX_MAX_FEATURES),
an arena of the dummy row alone, permuted columns, worlds 1 and 3, every capped grid with a second trip, the packed destination word at bit 30,
1 / 2 / 8 / 64 destination bases, batches around a block of 64 / 256 / 4096.  Against tests/shard_feat_ref.py (held to hand-written cases and to
oracle/ref_np.py by tests/test_shard_feat_ref.py) and oracle/ref_np.py's route_feat / owner_ids_from_inbox.

Every comparison is BIT FOR BIT: the work is integers, row copies, and one reduction whose two call paths the header promises equal.
Every device buffer is the body of a larger allocation whose every byte is 0xFF (NaN as a float, -1 as an integer); outputs start that way too
and carry guard rows / padding columns.  After a call the margins and everything the definition does not write are still 0xFF, and every input
holds what it held."""
import ctypes as C

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd._lib import NRX_ERR_BAD_ARG, NRX_ERR_UNSUPPORTED, NRX_OK, NRX_SPARSE, NrxFeature, NrxFmGrad
from oracle import ref_np
from tests import shard_feat_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32, I64, U32 = np.float32, np.int32, np.int64, np.uint32
I32MAX = S.I32MAX
MARGIN = 64                               # elements either side of a body: 64 bytes and more, so a body stays 16-byte aligned
NRX_BLOCK = 256
GUARD_ROWS = 2                            # rows behind every requester's buffer that nothing may write


class Buf:
    """A body of `shape` elements inside a device allocation of 0xFF bytes (MARGIN elements in front, MARGIN + 3 behind).  data=None: an
    output, 0xFF throughout.  read() returns the body and asserts that the margins are still 0xFF; unchanged() asserts that nothing at all
    was written."""

    def __init__(self, data=None, shape=None, dtype=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape))
        self.front = MARGIN
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


def _pack(arrays):
    """Several arrays in ONE 0xFF allocation, each at a 64-byte aligned offset with 64 bytes and more of 0xFF between them: (Buf, addresses)."""
    offs, size = [], 0
    for a in arrays:
        offs.append(size)
        size += (a.nbytes + 63) // 64 * 64 + 64
    host = np.full(max(size, 64), 0xFF, np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    b = Buf(host)
    return b, [b.ptr + o for o in offs]


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


# ================================================================================================= nrx_gather_place_feat(_bf16)
GATHER_DIMS = (16, 32, 64, 128, 256)
GATHER_FEATS = (1, 8, 9, 16, 17, 24, 25, 64)
BF16_NAN = 0x7FC1                                                       # a quiet NaN with a payload bit, as bf16


def _gather_case(seed, dim, n, world, capf, out_rows, nan_unused=False):
    """One launch's inputs.  Every (feature, source) block names each position at most once (what nrx_route_feat produces); its live slots are
    scattered among empty ones (position -1, whatever the id).  Planted on distinct live entries: ids -1, INT32 MIN, rows[f], rows[f] + 1 and
    INT32_MAX; a padding lookup (id 0 with a position); positions out_rows, out_rows + 3 and INT32_MAX.  Arenas of 2 .. 40 rows of bf16 bit
    patterns (the fp32 launches get them widened), row 0 zero; with more than one feature one arena is its dummy row alone.  nan_unused: every
    row the definition does not read -- row 0 among them -- holds a NaN."""
    rng = np.random.default_rng(seed)
    rows = [int(r) for r in rng.integers(2, 41, n)]
    if n > 1:
        rows[n // 2] = 1
    bits16 = [(rng.standard_normal((r, dim)).astype(F32).view(U32) >> 16).astype(np.uint16) for r in rows]
    for t in bits16:
        t[0] = 0
    cols = [int(c) * dim for c in rng.permutation(n)]                    # not in feature order
    bp = world * capf
    oid = rng.integers(-5, 100, (n, bp)).astype(I32)                     # (what an empty slot holds is ignored)
    opos = np.full((n, bp), -1, I32)
    for f in range(n):
        for s in range(world):
            k = int(rng.integers(3 * capf // 4, min(capf, out_rows) + 1))
            where = s * capf + np.sort(rng.choice(capf, k, replace=False))
            opos[f, where] = rng.permutation(out_rows)[:k]
            oid[f, where] = rng.integers(0, rows[f], k)
    live = np.argwhere(opos >= 0)
    pick = live[rng.choice(len(live), 9, replace=False)]
    for (f, b), what in zip(pick, ("neg", "min", "rows", "rows1", "max", "pad", "pos", "pos3", "posmax")):
        if what in ("neg", "min", "rows", "rows1", "max", "pad"):
            oid[f, b] = dict(neg=-1, min=-(1 << 31), rows=rows[f], rows1=rows[f] + 1, max=I32MAX, pad=0)[what]
        else:
            opos[f, b] = dict(pos=out_rows, pos3=out_rows + 3, posmax=I32MAX)[what]
    if nan_unused:
        for f in range(n):
            ok = (opos[f] >= 0) & (oid[f] > 0) & (oid[f] < rows[f])
            unread = np.setdiff1d(np.arange(rows[f]), oid[f][ok])
            bits16[f][unread] = BF16_NAN
            assert 0 in unread
    return dict(dim=dim, n=n, world=world, capf=capf, out_rows=out_rows, rows=rows, cols=cols, bits16=bits16, oid=oid, opos=opos,
                ld=n * dim + 4)


def _gather_want(c):
    outs = [np.full((c["out_rows"] + GUARD_ROWS, c["ld"]), S.SENTINEL, U32) for _ in range(c["world"])]
    count, reports = S.gather_place_feat(c["bits16"], c["rows"], c["cols"], c["oid"], c["opos"], c["world"], c["capf"], c["dim"], outs,
                                         c["out_rows"])
    return outs, count, reports


def _gather_run(c, form, with_status=True, **over):
    """One launch of the fp32 or the bf16 entry point on case c: (rc, the requesters' buffers as bit patterns, status or None).  over: arguments
    to replace (the refused calls)."""
    lib = _lib.load()
    arenas = c["bits16"] if form == "bf16" else [S.widen_bf16(t) for t in c["bits16"]]
    tabs, tab_ptrs = _pack(arenas)
    oid, opos = Buf(c["oid"]), Buf(c["opos"])
    outs = [Buf(shape=(c["out_rows"] + GUARD_ROWS, c["ld"]), dtype=U32) for _ in range(c["world"])]
    st = Buf(np.zeros(4, I32)) if with_status else None
    a = dict(tables=tab_ptrs, rows=c["rows"], cols=c["cols"], n=c["n"], world=c["world"], capf=c["capf"], dim=c["dim"],
             peers=[o.ptr for o in outs], ld=c["ld"], out_rows=c["out_rows"])
    a.update(over)
    fn = lib.nrx_gather_place_feat_bf16 if form == "bf16" else lib.nrx_gather_place_feat
    rc = fn(_parr(a["tables"]), _i64(a["rows"]), _i32(a["cols"]), a["n"], a["world"], a["capf"], oid.ptr, opos.ptr, a["dim"], _parr(a["peers"]),
            a["ld"], a["out_rows"], st.ptr if st else None, _stream())
    torch.cuda.synchronize()
    for b in (tabs, oid, opos):
        b.unchanged()
    return rc, [o.read() for o in outs], st.read() if st else None


def _gather_check(c, form, what):
    want, count, reports = _gather_want(c)
    rc, got, st = _gather_run(c, form)
    assert rc == NRX_OK, (what, form, _lib.load().nrx_last_error())
    for s, (g, w) in enumerate(zip(got, want)):                          # (the 4 padding columns and the guard rows are part of the comparison)
        assert np.array_equal(g, w), (what, form, "peer", s, "first difference at", np.argwhere(g != w)[:1].tolist())
    assert count == len(reports) and count >= 4                          # (distinct entries: one triple per report)
    assert int(st[0]) == count and tuple(int(x) for x in st[1:]) in reports, (what, form, st.tolist(), count)
    return got, st


@pytest.mark.parametrize("dim", GATHER_DIMS)
def test_gather_place_feat_both_forms_equal_the_definition(dim):
    for n in GATHER_FEATS:
        for world in (1, 3):
            capf = 16 if n <= 17 else 8
            c = _gather_case(1000 * dim + 10 * n + world, dim, n, world, capf, capf + 1)
            assert sorted(c["cols"]) != c["cols"] or n == 1
            a, sa = _gather_check(c, "fp32", (dim, n, world))
            b, sb = _gather_check(c, "bf16", (dim, n, world))
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and sa[0] == sb[0]


def test_gather_place_feat_without_a_status_word():
    """status = NULL (the header allows it): the same bad entries, the same buffers, NRX_OK."""
    c = _gather_case(7, 32, 9, 3, 16, 17)
    want, count, _ = _gather_want(c)
    assert count >= 8
    for form in ("fp32", "bf16"):
        rc, got, st = _gather_run(c, form, with_status=False)
        assert rc == NRX_OK and st is None
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), form


def test_gather_place_feat_reports_nothing_on_a_clean_launch():
    """Every id inside its arena and every position inside the batch: the status word is left as it was."""
    c = _gather_case(8, 64, 17, 3, 16, 17)
    for f in range(c["n"]):
        c["oid"][f][(c["oid"][f] < 0) | (c["oid"][f] >= c["rows"][f])] = 0
    c["opos"][c["opos"] >= c["out_rows"]] = -1
    want, count, reports = _gather_want(c)
    assert count == 0 and not reports
    for form in ("fp32", "bf16"):
        rc, got, st = _gather_run(c, form)
        assert rc == NRX_OK and st.tolist() == [0, 0, 0, 0]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), form


@pytest.mark.parametrize("dim,world,capf,n", [(256, 3, 10925, 2), (16, 2, 262144 + 19, 1)], ids=["dim256", "dim16"])
def test_gather_place_feat_past_its_grid_cap(dim, world, capf, n):
    """The launch is capped at 8192 blocks of 256 >> log2(dim / 4) pseudo-samples (4 at dim 256, 64 at dim 16) and strides beyond: world * capf
    just above 32 768 / 524 288 gives the first blocks a second trip.  Almost every slot is empty; a few hundred live ones lie in the first trip,
    in its last block and in the second trip, and what ONLY the second trip writes is compared on its own."""
    rng = np.random.default_rng(dim)
    tb = NRX_BLOCK // (dim // 4)
    first, bp, out_rows = 8192 * tb, world * capf, 400
    assert first < bp <= first + 2 * tb
    c = _gather_case(dim, dim, n, world, 16, out_rows)                   # (for its arenas and columns)
    oid, opos = np.zeros((n, bp), I32), np.full((n, bp), -1, I32)
    for f in range(n):
        where = np.unique(np.r_[rng.choice(first - tb, 300, replace=False), np.arange(first - tb, bp)])
        for s in range(world):
            w = where[where // capf == s]
            assert w.size <= out_rows
            opos[f, w] = rng.permutation(out_rows)[:w.size]
            oid[f, w] = rng.integers(0, c["rows"][f], w.size)
        bad = rng.choice(where, 4, replace=False)
        oid[f, bad[:2]] = (c["rows"][f], -3)
        opos[f, bad[2:]] = (out_rows, out_rows + 1)
    c.update(world=world, capf=capf, oid=oid, opos=opos)
    assert (opos[:, first:] >= 0).any() and (opos[:, first - tb:first] >= 0).any()
    only = dict(c, opos=np.where(np.arange(bp)[None, :] >= first, opos, -1).astype(I32))
    second = _gather_want(only)[0]
    for form in ("fp32", "bf16"):
        got, _ = _gather_check(c, form, ("grid cap", dim))
        written = 0
        for g, w in zip(got, second):
            m = w != S.SENTINEL
            written += int(m.sum())
            assert np.array_equal(g[m], w[m]), form
        assert written >= dim                                            # at least one whole row came from the second trip


@pytest.mark.parametrize("nan_unused", [False, True], ids=["plain", "nan_in_unread_rows"])
@pytest.mark.parametrize("dim", [16, 256])
def test_gather_place_feat_bf16_equals_fp32_on_the_widened_arenas(dim, nan_unused):
    """The header's promise, bit for bit.  The bf16 form loads unconditionally (row 0 for a slot that reads nothing) and then SELECTS: with a NaN
    in row 0 and in every other row that is not to be read, a load that is multiplied by 0 instead of dropped shows up as a NaN."""
    for n, world in ((9, 3), (25, 1)):
        c = _gather_case(dim + n, dim, n, world, 16, 17, nan_unused=nan_unused)
        a, sa = _gather_check(c, "fp32", ("fp32", dim, n))
        b, sb = _gather_check(c, "bf16", ("bf16", dim, n))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and sa[0] == sb[0]
        for x in b:
            body = x[:c["out_rows"], :c["ld"] - 4]
            assert not np.isnan(body[body != S.SENTINEL].view(F32)).any()


def test_gather_place_feat_refuses_bad_arguments_and_writes_nothing():
    c = _gather_case(3, 16, 3, 2, 16, 17)
    tabs = c["bits16"]
    for form, mis in (("fp32", 4), ("bf16", 2)):
        def call(**over):
            rc, outs, st = _gather_run(c, form, **over)
            assert all((o == S.SENTINEL).all() for o in outs) and st.tolist() == [0, 0, 0, 0], (form, over)
            return rc
        assert call(dim=24) == NRX_ERR_UNSUPPORTED
        assert call(ld=c["ld"] + 2) == NRX_ERR_UNSUPPORTED
        assert call(cols=[c["cols"][0] + 2] + c["cols"][1:]) == NRX_ERR_BAD_ARG
        good, ptrs = _pack(tabs if form == "bf16" else [S.widen_bf16(t) for t in tabs])
        assert call(tables=[ptrs[0] + mis] + ptrs[1:]) == NRX_ERR_BAD_ARG      # a misaligned arena
        assert call(tables=[ptrs[0], None, ptrs[2]]) == NRX_ERR_BAD_ARG
        peers = [Buf(shape=(c["out_rows"] + GUARD_ROWS, c["ld"]), dtype=U32) for _ in range(2)]
        assert call(peers=[peers[0].ptr, None]) == NRX_ERR_BAD_ARG
        assert call(peers=[peers[0].ptr, peers[1].ptr + 4]) == NRX_ERR_BAD_ARG
        for p in peers:
            p.unchanged()
        assert call(n=65) == NRX_ERR_BAD_ARG and call(world=0) == NRX_ERR_BAD_ARG and call(capf=0) == NRX_ERR_BAD_ARG
        if form == "bf16":                                               # (the bf16 form reads row 0 for the slots that read nothing: it must exist)
            assert call(rows=[c["rows"][0], 0, c["rows"][2]]) == NRX_ERR_BAD_ARG
    rc, got, _ = _gather_run(c, "fp32")                                  # the same case with good arguments goes through
    assert rc == NRX_OK and all(np.array_equal(g, w) for g, w in zip(got, _gather_want(c)[0]))


# ================================================================================================= nrx_route_feat
def _route(ids_np, world, capf, dtype=I64, with_pos=True, batch=None):
    """One nrx_route_feat launch on a zeroed state block: (rc, send_ids, send_pos or None, slot, counts, overflow), outputs 0xFF before."""
    lib = _lib.load()
    n = len(ids_np)
    B = len(ids_np[0]) if batch is None else batch
    ids = [Buf(np.asarray(x).astype(dtype)) for x in ids_np]
    send, pos = Buf(shape=(world, n, capf), dtype=I32), Buf(shape=(world, n, capf), dtype=I32)
    slot, counts, over = Buf(shape=(n, max(B, 1)), dtype=I32), Buf(shape=(world, n), dtype=I64), Buf(np.zeros(1, I64))
    state = torch.zeros(lib.nrx_route_feat_state_bytes(n, B, world), dtype=torch.uint8, device=DEV)
    rc = lib.nrx_route_feat(_parr([x.ptr for x in ids]), n, B, np.dtype(dtype).itemsize * 8, world, capf, send.ptr, pos.ptr if with_pos else None,
                            slot.ptr, counts.ptr, over.ptr, state.data_ptr(), _stream())
    torch.cuda.synchronize()
    for x in ids:
        x.unchanged()
    if not with_pos:
        pos.unchanged()
    return rc, send, pos if with_pos else None, slot, counts, over


def _route_check(ids_np, world, capf, dtype=I64, with_pos=True):
    rc, send, pos, slot, counts, over = _route(ids_np, world, capf, dtype, with_pos)
    assert rc == NRX_OK, _lib.load().nrx_last_error()
    w_send, w_pos, w_slot, w_counts, w_max = ref_np.route_feat(ids_np, world, capf)
    got = (send.read(), slot.read(), counts.read(), over.read(), pos.read() if with_pos else None)
    assert np.array_equal(got[0], w_send) and np.array_equal(got[1], w_slot) and np.array_equal(got[2], w_counts) and int(got[3][0]) == w_max
    if with_pos:
        assert np.array_equal(got[4], w_pos)
    return got


@pytest.mark.parametrize("world", [1, 3])
def test_route_feat_without_positions(world):
    """send_pos = NULL: the other four outputs are what the launch with positions leaves."""
    rng = np.random.default_rng(world)
    ids = [rng.integers(0, 5000, 4500) for _ in range(3)]
    capf = 4500 if world == 1 else 1600
    a = _route_check(ids, world, capf, with_pos=True)
    b = _route_check(ids, world, capf, with_pos=False)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and b[4] is None


def test_route_feat_world_1_with_a_capacity_that_is_not_the_batch():
    """The one-rank branch has its own overflow and tail code: capf < B drops the samples from capf on (slot -1) and reports counts = overflow = B;
    capf > B fills [B, capf) with 0 / -1."""
    rng = np.random.default_rng(5)
    for B, capf in ((4500, 4000), (4500, 100), (4500, 4500 + 700), (300, 4097 + 300), (1, 4)):
        ids = [rng.integers(0, 900, B) for _ in range(2)]
        for dt in (I64, I32):
            send, slot, counts, over, pos = _route_check(ids, 1, capf, dt)
            if capf < B:
                assert (slot[:, capf:] == -1).all() and (slot[:, :capf] >= 0).all() and (counts == B).all() and over[0] == B
            else:
                assert (send[0, :, B:] == 0).all() and (pos[0, :, B:] == -1).all() and (slot >= 0).all()


@pytest.mark.parametrize("B", [4095, 4097, 8192, 8193])
def test_route_feat_around_its_tile_of_4096_ids(B):
    rng = np.random.default_rng(B)
    ids = [rng.integers(0, 100_000, B) for _ in range(2)]
    ids[1][:4] = (0, -9, I32MAX, 1 << 40)
    _route_check(ids, 3, B // 3 + 40)
    _route_check(ids, 3, B // 3 - 40)                                    # every block overflows a little


def test_route_feat_every_id_on_one_rank_and_half_the_room():
    """Every id is owned by rank 2 (id % 3 == 2) and capf is half the count: the surplus is dropped from the middle of the first tile on."""
    rng = np.random.default_rng(8)
    ids = [3 * rng.integers(0, 1000, 6000) + 2]
    send, slot, counts, over, _ = _route_check(ids, 3, 3000)
    assert counts.tolist() == [[0], [0], [6000]] and over[0] == 6000
    assert (slot[0, 3000:] == -1).all() and np.array_equal(slot[0, :3000], 2 * 3000 + np.arange(3000))
    assert not send[:2].any()


@pytest.mark.parametrize("world", [1, 3])
def test_route_feat_the_largest_id_that_is_a_row(world):
    """int64 id 2^31 - 2: the last id that can still be a row (2^31 - 1 and beyond go to rank 0 as INT32_MAX).  The header's send_ids text decides:
    owner id = id / world + 1 on rank id % world -- at world 1 that IS INT32_MAX, the value the marker shares."""
    big = (1 << 31) - 2
    ids = [np.array([5, big, 0, big - 1, big + 1, 7, big], I64)]
    send = _route_check(ids, world, 8)[0]
    if world == 1:                                                       # everything stays, in sample order
        assert send[0, 0, :7].tolist() == [6, I32MAX, 0, big, I32MAX, 8, I32MAX]
    else:                                                                # big % 3 == 0: rank 0 gets big, the padding id, the id that is no row, big
        assert big % 3 == 0 and send[0, 0, :5].tolist() == [big // 3 + 1, 0, I32MAX, big // 3 + 1, 0]


def test_route_feat_with_an_empty_batch():
    rc, send, pos, slot, counts, over = _route([np.zeros(0, I64)], 3, 8)
    assert rc == NRX_OK
    for b in (send, pos, slot, counts):
        b.unchanged()
    assert over.read()[0] == 0


# ================================================================================================= nrx_inbox_transpose
def _transpose(a, b, world, n, capf, over=()):
    lib = _lib.load()
    ia, ib = Buf(a), Buf(b) if b is not None else None
    oa, ob = Buf(shape=(n, world * capf), dtype=I32), Buf(shape=(n, world * capf), dtype=I32)
    arg = dict(ia=ia.ptr, oa=oa.ptr, ib=ib.ptr if ib else None, ob=ob.ptr if ib else None, world=world, n=n, capf=capf)
    arg.update(dict(over))
    rc = lib.nrx_inbox_transpose(arg["ia"], arg["oa"], arg["ib"], arg["ob"], arg["world"], arg["n"], arg["capf"], _stream())
    torch.cuda.synchronize()
    ia.unchanged()
    if ib:
        ib.unchanged()
    return rc, oa, ob


@pytest.mark.parametrize("world,n,capf", [(1, 1, 4), (2, 3, 4), (5, 64, 8), (64, 2, 12)])
def test_inbox_transpose_equals_its_definition(world, n, capf):
    rng = np.random.default_rng(world * n)
    a = rng.integers(-5, 1 << 30, (world, n, capf)).astype(I32)
    b = rng.integers(-1, 1 << 20, (world, n, capf)).astype(I32)
    rc, oa, ob = _transpose(a, b, world, n, capf)
    assert rc == NRX_OK
    assert np.array_equal(oa.read(), ref_np.owner_ids_from_inbox(a)) and np.array_equal(ob.read(), ref_np.owner_ids_from_inbox(b))
    rc, oa, ob = _transpose(a, None, world, n, capf)
    assert rc == NRX_OK and np.array_equal(oa.read(), ref_np.owner_ids_from_inbox(a))
    ob.unchanged()
    # the backward's call with the roles of the outer dimensions swapped: [f][s][k] -> [s][f][k]
    per_feature = ref_np.owner_ids_from_inbox(a).reshape(n, world, capf)
    rc, back, _ = _transpose(per_feature, None, n, world, capf)
    assert rc == NRX_OK
    got = back.read().reshape(world, n, capf)
    assert np.array_equal(got, np.transpose(per_feature, (1, 0, 2))) and np.array_equal(got, a)


def test_inbox_transpose_past_its_grid_cap():
    """The launch is capped at 4096 blocks of 256 lanes x 16 bytes = 4 194 304 ints and strides beyond: world 2, n 5, capf 419 432 is 16 ints
    more, four 16-byte pieces that only the second trip moves -- the last of them asserted by itself, in both arrays."""
    world, n, capf = 2, 5, 419_432
    total = world * n * capf
    assert 4096 * NRX_BLOCK * 4 < total <= 4096 * NRX_BLOCK * 4 + 64
    rng = np.random.default_rng(2)
    a = rng.integers(-5, 1 << 30, (world, n, capf)).astype(I32)
    b = rng.integers(-1, 1 << 20, (world, n, capf)).astype(I32)
    rc, oa, ob = _transpose(a, b, world, n, capf)
    assert rc == NRX_OK
    ga, gb = oa.read(), ob.read()
    # the input's last piece is (source 1, feature 4, k = capf - 4 ..): the end of feature 4's row of the output
    assert np.array_equal(ga[4, -4:], a[1, 4, -4:]) and np.array_equal(gb[4, -4:], b[1, 4, -4:])
    assert np.array_equal(ga[4, -16:], a[1, 4, -16:]) and np.array_equal(gb[4, -16:], b[1, 4, -16:])
    assert np.array_equal(ga, ref_np.owner_ids_from_inbox(a)) and np.array_equal(gb, ref_np.owner_ids_from_inbox(b))


def test_inbox_transpose_refuses_bad_arguments_and_writes_nothing():
    a = np.arange(2 * 3 * 8, dtype=I32).reshape(2, 3, 8)
    good = Buf(a)
    for over in (dict(capf=6), dict(capf=0), dict(ia=good.ptr + 4), dict(oa=None), dict(ia=None), dict(world=0), dict(n=0)):
        rc, oa, ob = _transpose(a, a, 2, 3, 8, over)
        assert rc == NRX_ERR_BAD_ARG, over
        oa.unchanged()
        ob.unchanged()
    rc, oa, ob = _transpose(a, None, 2, 3, 8, dict(ib=good.ptr))                # inbox_b without out_b
    assert rc == NRX_ERR_BAD_ARG
    oa.unchanged()
    rc, oa, ob = _transpose(a, None, 2, 3, 8, dict(ob=good.ptr))                # ... and out_b without inbox_b
    assert rc == NRX_ERR_BAD_ARG
    oa.unchanged()
    good.unchanged()
    rc, oa, _ = _transpose(a, None, 2, 3, 8)
    assert rc == NRX_OK and np.array_equal(oa.read(), ref_np.owner_ids_from_inbox(a))


# ================================================================================================= nrx_shard_dest_combine
def _combine(slot, dest_req, n, batch, capf, recv_row0, rank, world, shift, want_rc=NRX_OK):
    lib = _lib.load()
    sb, db = Buf(np.asarray(slot, I32)), Buf(np.asarray(dest_req, I32))
    out = Buf(shape=(n, max(batch, 1)), dtype=I32)
    rc = lib.nrx_shard_dest_combine(sb.ptr, db.ptr, n, batch, capf, recv_row0, rank, world, shift, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, want_rc, lib.nrx_last_error())
    sb.unchanged()
    db.unchanged()
    if rc != NRX_OK or batch == 0:
        out.unchanged()
        return None
    return out.read()


@pytest.mark.parametrize("n", [1, 3, 26, 64])
def test_shard_dest_combine_on_route_feats_own_slots(n):
    """slot comes from a real nrx_route_feat launch with a capacity tight enough to drop lookups; dest_req is random with a share of -1."""
    rng = np.random.default_rng(n)
    dropped = 0
    for batch in (1, 255, 256, 257):
        for world in (1, 2, 5, 8):
            ids = [rng.integers(0, 1000, batch) for _ in range(n)]
            capf = max(1, int(batch / world * 0.8))
            rc, _, _, slot_b, _, _ = _route(ids, world, capf)
            assert rc == NRX_OK
            slot = slot_b.read()
            assert np.array_equal(slot, ref_np.route_feat(ids, world, capf)[2])
            dropped += int((slot == -1).sum())
            shift, recv_row0 = 20, 1 << 19
            dest_req = np.where(rng.random((world, n, capf)) < 0.3, -1, rng.integers(0, recv_row0, (world, n, capf))).astype(I32)
            for rank in sorted({0, world - 1}):
                got = _combine(slot, dest_req, n, batch, capf, recv_row0, rank, world, shift)
                want = S.shard_dest_combine(slot, dest_req, n, batch, capf, recv_row0, rank, shift)
                assert np.array_equal(got, want), (batch, world, rank, np.argwhere(got != want)[:1].tolist())
    assert dropped > 0


def test_shard_dest_combine_packs_up_to_bit_30():
    """shift 30, world 2, capf 2^20, the receive buffer ending exactly at row 2^30: the largest words are 2^31 - 1 and must stay positive int32."""
    n, world, shift, capf = 1, 2, 30, 1 << 20
    recv_row0 = (1 << 30) - (1 << 21)
    rng = np.random.default_rng(30)
    batch = 999
    o, k = rng.integers(0, 2, batch), rng.integers(0, capf, batch)
    o[:4], k[:4] = (1, 1, 0, 0), (capf - 1, 0, capf - 1, 0)
    slot = ((o * capf + k) * n).astype(I32)[None, :]
    slot[0, 10] = -1
    dest_req = np.full((world, n, capf), -1, I32)
    dest_req[1, 0, 0] = (1 << 30) - 1                                    # a placed row at the top of owner 1's arena
    dest_req[0, 0, rng.integers(1, capf - 1, 5000)] = rng.integers(0, recv_row0, 5000)
    got = _combine(slot, dest_req, n, batch, capf, recv_row0, 1, world, shift)
    want = S.shard_dest_combine(slot, dest_req, n, batch, capf, recv_row0, 1, shift)
    assert want[0, 0] == I32MAX and want[0, 1] == I32MAX and want[0, 10] == -1 and (np.delete(want[0], 10) >= 0).all()
    assert np.array_equal(got, want)


def test_shard_dest_combine_past_its_grid_cap():
    """grid.x is capped at 1024 blocks of 256 lookups per feature and strides beyond: batch 262 144 + 300 gives 300 lookups of each feature to the
    second trip, asserted present (routed, not dropped) and correct by themselves."""
    n, world, batch, capf, shift, recv_row0 = 2, 2, 262_144 + 300, 140_000, 24, 1 << 23
    rng = np.random.default_rng(1024)
    o, k = rng.integers(0, world, (n, batch)), rng.integers(0, capf, (n, batch))
    slot = ((o * capf + k) * n + np.arange(n)[:, None]).astype(I32)
    slot[rng.random((n, batch)) < 0.05] = -1
    slot[:, -5:] = ((1 * capf + capf - 1) * n + np.arange(n)[:, None])
    dest_req = np.where(rng.random((world, n, capf)) < 0.5, -1, rng.integers(0, recv_row0, (world, n, capf))).astype(I32)
    got = _combine(slot, dest_req, n, batch, capf, recv_row0, 1, world, shift)
    want = S.shard_dest_combine(slot, dest_req, n, batch, capf, recv_row0, 1, shift)
    tail = slice(1024 * NRX_BLOCK, batch)
    assert (want[:, tail] >= 0).sum() > 500 and np.array_equal(got[:, tail], want[:, tail])
    assert np.array_equal(got, want)


def test_shard_dest_combine_refuses_bad_arguments_and_an_empty_batch_writes_nothing():
    n, batch, capf, world = 2, 10, 4, 2
    slot = np.arange(n * batch, dtype=I32).reshape(n, batch) % (world * capf * n)
    dest_req = np.full((world, n, capf), -1, I32)
    bad = [dict(rank=2), dict(rank=-1), dict(shift=0), dict(shift=31), dict(world=3, shift=30), dict(world=5, shift=29),
           dict(recv_row0=(1 << 20) - world * capf * n + 1), dict(capf=0)]
    base = dict(n=n, batch=batch, capf=capf, recv_row0=100, rank=0, world=world, shift=20)
    for over in bad:
        _combine(slot, dest_req, want_rc=NRX_ERR_BAD_ARG, **dict(base, **over))
    _combine(np.zeros((65, batch), I32), np.full((world, 65, capf), -1, I32), want_rc=NRX_ERR_BAD_ARG, **dict(base, n=65))
    assert _combine(slot, dest_req, **dict(base, batch=0)) is None       # NRX_OK, nothing written
    assert _combine(slot, dest_req, **dict(base, recv_row0=(1 << 20) - world * capf * n)) is not None      # exactly full: accepted


# ================================================================================================= the direct-gradient backward
def _features(n, D, index_ptrs, bits, fm, rows=None, wide=None):
    arr = (NrxFeature * n)()
    for i in range(n):
        f = arr[i]
        f.table, f.weight, f.index, f.index_bits = None, None, index_ptrs[i], bits
        f.rows = 0 if rows is None else rows[i]
        f.dim, f.bag_len, f.kind, f.out_col, f.wide_col, f.fm_field, f.flags = D, 0, NRX_SPARSE, i * D, -1 if wide is None else wide[i], int(fm), 0
    return arr


class Upstream:
    """g_out [B, n D] and, with the FM term, g_fm [B], the field sums [B, D] and the forward concat [B, n D]: the fixtures of
    test_embed_bwd_scatter_places_every_upstream_row."""

    def __init__(self, rng, B, n, D, fm):
        self.ld = n * D
        self.g = Buf(rng.standard_normal((B, self.ld)).astype(F32))
        self.fmg, self.keep = None, [self.g]
        if fm:
            feat, sums, g_fm = (Buf(rng.standard_normal(s).astype(F32)) for s in ((B, self.ld), (B, D), (B,)))
            self.fmg = NrxFmGrad(g_fm.ptr, sums.ptr, D, feat.ptr, self.ld)
            self.keep += [feat, sums, g_fm]

    def unchanged(self):
        for b in self.keep:
            b.unchanged()


MULTI_COMBOS = [(1, 30), (1, 12), (2, 30), (2, 12), (8, 28), (8, 12), (64, 25), (64, 12)]      # (bases, shift): the largest shift the count allows, and 12


def _multi_case(rng, lib, D, n, B, fm, n_bases, shift):
    """nrx_embed_bwd_scatter_multi into n_bases buffers against nrx_embed_bwd_scatter into each of them with scatter_multi_split's dest."""
    total = n * B
    base_of = rng.integers(0, n_bases, total)
    empty = n_bases - 1 if n_bases > 1 else None                         # one base receives nothing
    if empty is not None:
        base_of[base_of == empty] = 0
    dest = np.full(total, -1, I64)
    sizes = []
    for x in range(n_bases):
        m = np.flatnonzero(base_of == x)
        sizes.append(m.size + 7)
        assert sizes[-1] <= 1 << shift
        dest[m] = (x << shift) | rng.permutation(sizes[-1])[:m.size]      # a partial permutation of the base's rows
    dest[rng.random(total) < 0.01] = -1
    dest = dest.astype(I32)
    up, db = Upstream(rng, B, n, D, fm), Buf(dest)
    arr = _features(n, D, [db.ptr + 4 * i * B for i in range(n)], 32, fm)
    multi = [Buf(shape=(r, D), dtype=U32) for r in sizes]
    _ok(lib.nrx_embed_bwd_scatter_multi(arr, n, B, D, up.g.ptr, up.ld, up.fmg, db.ptr, _parr([b.ptr for b in multi]), n_bases, shift, _stream()),
        "nrx_embed_bwd_scatter_multi")
    db.unchanged()
    up.unchanged()
    what = (D, n, B, fm, n_bases, shift)
    for x, d in enumerate(S.scatter_multi_split(dest, shift, n_bases)):
        got = multi[x].read()
        named = np.zeros(sizes[x], bool)
        named[d[d >= 0]] = True
        assert (got[~named] == S.SENTINEL).all(), what                   # rows no lookup names keep their sentinel
        if not named.any():
            continue
        one, sd = Buf(shape=(sizes[x], D), dtype=U32), Buf(d)
        _ok(lib.nrx_embed_bwd_scatter(arr, n, B, D, up.g.ptr, up.ld, None, 0, up.fmg, sd.ptr, one.ptr, _stream()), "nrx_embed_bwd_scatter")
        want = one.read()
        assert np.array_equal(got, want), (what, "base", x, np.argwhere(got != want)[:1].tolist())
        assert not np.isnan(got[named].view(F32)).any()
    if empty is not None:
        multi[empty].unchanged()


@pytest.mark.parametrize("fm", [False, True], ids=["plain", "fm"])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_embed_bwd_scatter_multi_equals_the_single_buffer_scatter_per_base(D, fm):
    """Per base the buffer holds, bit for bit, what nrx_embed_bwd_scatter writes with that base's share of dest (that entry point has its own
    value-exact test), unnamed rows and a base that receives nothing stay 0xFF.  The several-buffer launch of embed_bwd_sorted_impl
    (sorted_bwd_launch_place, multi_bases) has ONE form and no grid cap -- ceil(batch / (256 >> log2(D / 4))) blocks, one lane group per sample
    -- so the batches are those around a block of 64 samples (D 16), and 3001."""
    lib = _lib.load()
    rng = np.random.default_rng(D + fm)
    seen, j = set(), D // 16 + fm
    for n in (1, 5, 26):
        for B in (1, 63, 64, 65, 3001):
            n_bases, shift = MULTI_COMBOS[j % 8]
            j += 1
            if (n * B + 7) > (1 << shift):                               # shift 12 names 4096 rows per base
                shift = max(s for b, s in MULTI_COMBOS if b == n_bases)
            seen.add((n_bases, shift))
            _multi_case(rng, lib, D, n, B, fm, n_bases, shift)
    for n_bases, shift in MULTI_COMBOS:
        if (n_bases, shift) not in seen:
            _multi_case(rng, lib, D, 5, 65, fm, n_bases, shift)


def test_embed_bwd_scatter_multi_refuses_bad_arguments_and_writes_nothing():
    lib = _lib.load()
    rng = np.random.default_rng(4)
    n, B, D = 3, 50, 16
    up = Upstream(rng, B, n, D, False)
    db = Buf(rng.permutation(n * B).astype(I32))
    out = Buf(shape=(n * B, D), dtype=U32)
    arr = _features(n, D, [db.ptr] * n, 32, False)
    many = _parr([out.ptr] * 65)

    def call(arr=arr, D=D, bases=many, n_bases=1, shift=20):
        return lib.nrx_embed_bwd_scatter_multi(arr, n, B, D, up.g.ptr, up.ld, None, db.ptr, bases, n_bases, shift, _stream())

    assert call(arr=_features(n, 24, [db.ptr] * n, 32, False), D=24) == NRX_ERR_UNSUPPORTED
    assert call(n_bases=65) == NRX_ERR_BAD_ARG and call(n_bases=0) == NRX_ERR_BAD_ARG
    assert call(shift=31) == NRX_ERR_BAD_ARG and call(shift=0) == NRX_ERR_BAD_ARG
    assert call(n_bases=3, shift=30) == NRX_ERR_BAD_ARG                   # base numbers past bit 30
    assert call(bases=_parr([out.ptr + 4])) == NRX_ERR_BAD_ARG and call(bases=_parr([out.ptr, None]), n_bases=2) == NRX_ERR_BAD_ARG
    assert call(arr=_features(n, D, [db.ptr] * n, 32, False, wide=[-1, 0, -1])) == NRX_ERR_BAD_ARG
    out.unchanged()
    _ok(call(), "nrx_embed_bwd_scatter_multi")
    assert not (out.read() == S.SENTINEL).any()


WALK_B = 1500


def _walk_id_sets(rng):
    """name -> (ids per feature, table of each feature, rows per table, place mask)."""
    B = WALK_B
    five, full = [0, 1, 2, 3, 4], (1 << 5) - 1
    rows = [4000, 2000, 9000, 1700, 3000]
    distinct = [rng.permutation(np.arange(1, r))[:B] for r in rows]
    with_pad = [x.copy() for x in distinct]
    for x in with_pad:
        x[rng.integers(0, B, 3)] = 0
    zipf = [np.minimum(rng.zipf(1.2, B) - 1, r - 1) for r in rows]
    uniform = [rng.integers(0, r, B) for r in rows]
    shared = [rng.integers(0, 2500, B), rng.integers(0, 2500, B), rng.integers(0, 50_000, B)]
    return {
        "all_distinct": (distinct, five, rows, full),                    # nothing is walked
        "distinct_and_padding": (with_pad, five, rows, full),            # the walk list holds the padding rows only
        "all_equal": ([np.full(B, 7) for _ in rows], five, rows, full),  # everything walked, through the work lists of the long rows
        "padding_40_percent": ([np.where(rng.random(B) < 0.4, 0, x) for x in uniform], five, rows, full),
        "zipf": (zipf, five, rows, full),
        "partial_mask": (uniform, five, rows, 0b10101),
        "shared_table": (shared, [0, 0, 1], [2500, 50_000], 0b111),
    }


def _walk_case(lib, rng, D, fm, ids_np, table_of, rows, mask, dev_count, policy):
    n, B = len(ids_np), len(ids_np[0])
    total = n * B
    ids = [torch.from_numpy(np.asarray(x, I64)).to(DEV) for x in ids_np]
    pl = ops.sparse_plan(ids, table_of, [rows[t] for t in table_of], len(rows), place_feats=mask, policy=policy)
    torch.cuda.synchronize()
    pairs = len(pl) == 8
    assert pairs == (policy is not None)
    order, uniq, seg, counts, dest, walk, n_walk = pl[:7]
    nu = int(counts[0])
    up = Upstream(rng, B, n, D, fm)
    arr = _features(n, D, [x.data_ptr() for x in ids], 64, fm, rows=[rows[t] for t in table_of])
    lws = torch.empty(lib.nrx_embed_bwd_workspace_for(arr, n, B, D), dtype=torch.uint8, device=DEV)
    n_unique, n_dev = (total, counts.data_ptr()) if dev_count else (nu, None)
    plan = (order.data_ptr(), seg.data_ptr(), uniq.data_ptr(), n_unique, n_dev, up.fmg)
    tail = (mask, dest.data_ptr(), walk.data_ptr(), n_walk.data_ptr())
    rec = (pl[7].data_ptr(), n_walk.data_ptr() + 8) if pairs else (None, None)
    a, b = Buf(shape=(total, D), dtype=U32), Buf(shape=(total, D), dtype=U32)
    if pairs:
        _ok(lib.nrx_embed_bwd_placed_pairs(arr, n, B, D, up.g.ptr, up.ld, None, 0, *plan, a.ptr, None, 0, 0, *tail, *rec, lws.data_ptr(), lws.numel(),
                                           None, _stream()), "nrx_embed_bwd_placed_pairs")
    else:
        _ok(lib.nrx_embed_bwd_placed(arr, n, B, D, up.g.ptr, up.ld, None, 0, *plan, a.ptr, *tail, lws.data_ptr(), lws.numel(), _stream()),
            "nrx_embed_bwd_placed")
    # what the requesters place: the plan's dest for the lookups of the features in place_feats -- the planner leaves the other words untouched
    # (include/nrx_embed.h, nrx_sparse_plan_place), so they are no destinations
    placeable = np.repeat([(mask >> i) & 1 == 1 for i in range(n)], B)
    req = np.where(placeable, dest.cpu().numpy()[:total], -1).astype(I32)
    assert req.max() < nu and np.unique(req[req >= 0]).size == (req >= 0).sum()
    rb = Buf(req)
    _ok(lib.nrx_embed_bwd_scatter(arr, n, B, D, up.g.ptr, up.ld, None, 0, up.fmg, rb.ptr, b.ptr, _stream()), "nrx_embed_bwd_scatter")
    _ok(lib.nrx_embed_bwd_walk(arr, n, B, D, up.g.ptr, up.ld, *plan, b.ptr, *tail, *rec, lws.data_ptr(), lws.numel(), _stream()), "nrx_embed_bwd_walk")
    up.unchanged()
    va, vb = a.read(), b.read()
    assert 0 < nu <= total
    assert np.array_equal(va[:nu], vb[:nu]), ("first difference at", np.argwhere(va[:nu] != vb[:nu])[:1].tolist())
    assert not np.isnan(vb[:nu].view(F32)).any()                         # every unique row was written: placed, walked or paired
    assert (vb[nu:] == S.SENTINEL).all()
    return nu, int(n_walk[0]), pairs


@pytest.mark.parametrize("fm", [False, True], ids=["plain", "fm"])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_embed_bwd_scatter_then_walk_gives_the_bits_of_the_placed_backward(D, fm, monkeypatch):
    """The header's identity: nrx_embed_bwd_scatter with the plan's dest followed by nrx_embed_bwd_walk leaves in values[:n_unique] the bits of
    nrx_embed_bwd_placed (sorted plan) / nrx_embed_bwd_placed_pairs (one-kernel plan with pair records), and nothing behind them.  n_unique on
    the host and as the plan's device count; pair-record plans wherever nrx_sparse_plan_lds_ok accepts the shape.  With a partial place_feats
    mask the scatter places the masked features' lookups only, as the placement pass it stands in for does: the planner writes no dest word for
    the others."""
    lib = _lib.load()
    rng = np.random.default_rng(10 * D + fm)
    monkeypatch.setattr(ops, "PLAN_LDS", "1")                            # (a PlanPolicy then always picks the one-kernel planner where it is eligible)
    lds_runs = 0
    for name, (ids_np, table_of, rows, mask) in _walk_id_sets(rng).items():
        n = len(ids_np)
        for dev_count in (False, True):
            nu, nw, _ = _walk_case(lib, rng, D, fm, ids_np, table_of, rows, mask, dev_count, None)
            if name == "all_distinct":                                   # the walk list holds nothing, or the tables' padding rows
                assert nw <= n and nu == n * WALK_B
            if name == "distinct_and_padding":
                assert 1 <= nw <= n
            if name == "all_equal":
                assert nw == nu == n
        lens, tof, rws = _i64([WALK_B] * n), _i32(table_of), _i64([rows[t] for t in table_of])
        if mask == (1 << n) - 1 and lib.nrx_sparse_plan_lds_ok(lens, tof, rws, n, len(rows)):
            pol = ops.PlanPolicy(lens, tof, rws, n, len(rows), n * WALK_B)
            assert pol.eligible and pol.choose()
            for dev_count in (False, True):
                _walk_case(lib, rng, D, fm, ids_np, table_of, rows, mask, dev_count, pol)
                lds_runs += 1
    assert lds_runs > 0


def test_embed_bwd_walk_refuses_shapes_outside_the_placement_plan():
    lib = _lib.load()
    n, B, D = 2, 40, 24
    rng = np.random.default_rng(24)
    ids = [torch.from_numpy(rng.integers(0, 30, B)).to(DEV) for _ in range(n)]
    pl = ops.sparse_plan(ids, [0, 1], [30, 30], 2, place_feats=3)
    up = Upstream(rng, B, n, D, False)
    arr = _features(n, D, [x.data_ptr() for x in ids], 64, False, rows=[30, 30])
    vals, ws = Buf(shape=(n * B, D), dtype=U32), torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rc = lib.nrx_embed_bwd_walk(arr, n, B, D, up.g.ptr, up.ld, pl[0].data_ptr(), pl[2].data_ptr(), pl[1].data_ptr(), n * B, pl[3].data_ptr(), None,
                                vals.ptr, 3, pl[4].data_ptr(), pl[5].data_ptr(), pl[6].data_ptr(), None, None, ws.data_ptr(), ws.numel(), _stream())
    assert rc == NRX_ERR_UNSUPPORTED
    rc = lib.nrx_embed_bwd_walk(arr, n, B, D, up.g.ptr, up.ld, pl[0].data_ptr(), pl[2].data_ptr(), pl[1].data_ptr(), n * B, pl[3].data_ptr(), None,
                                vals.ptr, 3, None, pl[5].data_ptr(), pl[6].data_ptr(), None, None, ws.data_ptr(), ws.numel(), _stream())
    assert rc == NRX_ERR_BAD_ARG                                         # no dest: not a placement plan
    vals.unchanged()
