"""tests/shard_feat_ref.py against hand-written cases (every expected array written out) and against oracle/ref_np.py: the slot word that
shard_dest_combine takes apart is route_feat's, so every routed lookup must come back as the (owner, k) route_feat gave it.  No GPU."""
import numpy as np

from oracle import ref_np
from tests import shard_feat_ref as S


def _hand_gather(arenas, zero_row=True):
    # world 2, capf 2, two features of 2 columns placed in swapped column order, a requester batch of 2 rows (+ a guard row), ld 5
    oid = np.array([[1, 0, 2, 3],            # f0: row 1 | the padding id | an empty slot (its id is ignored) | id == rows[0]: zeros, reported
                    [1, -1, 1, 1]], np.int32)  # f1: position == out_rows: dropped, reported | id < 0: zeros, reported | row 1 | an empty slot
    opos = np.array([[0, 1, -1, 1],
                     [2, 0, 0, -1]], np.int32)
    outs = [np.full((3, 5), 9.0, np.float32) for _ in range(2)]
    count, reports = S.gather_place_feat(arenas, [3, 2], [2, 0], oid, opos, 2, 2, 2, outs, 2)
    return outs, count, reports


def test_gather_place_feat_definition_by_hand():
    a0 = np.array([[0, 0], [1, 2], [3, 4]], np.float32)
    a1 = np.array([[0, 0], [5, 6]], np.float32)
    outs, count, reports = _hand_gather([a0, a1])
    assert np.array_equal(outs[0], np.array([[0, 0, 1, 2, 9], [9, 9, 0, 0, 9], [9, 9, 9, 9, 9]], np.float32))
    assert np.array_equal(outs[1], np.array([[5, 6, 9, 9, 9], [9, 9, 0, 0, 9], [9, 9, 9, 9, 9]], np.float32))
    assert count == 3 and reports == {(0, 3, 3), (1, 0, 2), (1, 1, -1)}
    # the dummy row is never READ: a NaN there changes nothing
    a0[0], a1[0] = np.nan, np.nan
    again, count, reports = _hand_gather([a0, a1])
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(outs, again)) and count == 3


def test_gather_place_feat_definition_widens_bf16_exactly():
    # bf16 1.0 = 0x3F80, 2.0 = 0x4000, -3.0 = 0xC040, 0.5 = 0x3F00, 5.0 = 0x40A0, 6.0 = 0x40C0
    b0 = np.array([[0, 0], [0x3F80, 0x4000], [0xC040, 0x3F00]], np.uint16)
    b1 = np.array([[0, 0], [0x40A0, 0x40C0]], np.uint16)
    assert np.array_equal(S.widen_bf16(b0).view(np.float32), np.array([[0, 0], [1, 2], [-3, 0.5]], np.float32))
    outs, count, _ = _hand_gather([b0, b1])
    assert np.array_equal(outs[0], np.array([[0, 0, 1, 2, 9], [9, 9, 0, 0, 9], [9, 9, 9, 9, 9]], np.float32))
    assert np.array_equal(outs[1], np.array([[5, 6, 9, 9, 9], [9, 9, 0, 0, 9], [9, 9, 9, 9, 9]], np.float32))
    wide, _, _ = _hand_gather([S.widen_bf16(b0), S.widen_bf16(b1)])                     # the fp32 call on the widened arenas: the same bits
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(outs, wide)) and count == 3


HAND_SLOT = np.array([[0, 4, 2],              # f0: (o0, k0) | (o1, k0) | (o0, k1)                slot = (o * capf + k) * n + f, n = 2, capf = 2
                      [7, -1, 1]], np.int32)  # f1: (o1, k1) | dropped  | (o0, k0)
HAND_DEST_REQ = np.array([[[5, -1], [-1, 9]],       # owner 0: feature 0's two slots, feature 1's
                          [[-1, 3], [2, 7]]], np.int32)
HAND_DEST = np.array([[5, 256 + 104, 106],    # placed at values[5] of owner 0 | owner 1's receive row 100 + (1 * 2 + 0) * 2 + 0 | owner 0's 100 + (2 + 1) * 2 + 0
                      [256 + 7, -1, 105]], np.int32)  # values[7] of owner 1 | dropped | owner 0's 100 + (2 + 0) * 2 + 1


def test_shard_dest_combine_definition_by_hand():
    got = S.shard_dest_combine(HAND_SLOT, HAND_DEST_REQ, n=2, batch=3, capf=2, recv_row0=100, rank=1, shift=8)
    assert got.dtype == np.int32 and np.array_equal(got, HAND_DEST)
    assert np.array_equal(S.shard_dest_combine(HAND_SLOT.reshape(-1), HAND_DEST_REQ, 2, 3, 2, 100, 1, 8), HAND_DEST)       # flat, feature-major


def test_scatter_multi_split_definition_by_hand():
    per_base = S.scatter_multi_split(HAND_DEST.reshape(-1), shift=8, n_bases=3)
    assert [x.tolist() for x in per_base] == [[5, -1, 106, -1, -1, 105], [-1, 104, -1, 7, -1, -1], [-1] * 6]
    assert all(x.dtype == np.int32 for x in per_base)


def test_shard_dest_combine_decodes_route_feats_slot():
    rng = np.random.default_rng(11)
    for n, B, world in ((1, 40, 1), (3, 257, 2), (5, 300, 5), (26, 97, 8)):
        ids = [rng.integers(0, 500, B) for _ in range(n)]
        capf = max(1, int(B / world * 0.8))                              # tight: some lookups are dropped
        _, send_pos, slot, counts, _ = ref_np.route_feat(ids, world, capf)
        assert (slot == -1).any() and counts.max() > capf
        shift = 20
        for rank in (0, world - 1):
            # dest_req all -1: every routed lookup goes to its row of the receive buffer, (rank * capf + k) * n + f behind recv_row0
            got = S.shard_dest_combine(slot, np.full((world, n, capf), -1, np.int32), n, B, capf, 1000, rank, shift).astype(np.int64)
            assert np.array_equal(got == -1, slot == -1)
            for f in range(n):
                for b in np.flatnonzero(slot[f] >= 0):
                    o, row = got[f, b] >> shift, (got[f, b] & ((1 << shift) - 1)) - 1000
                    assert row % n == f
                    k = row // n - rank * capf
                    assert 0 <= k < capf and send_pos[o, f, k] == b       # the (o, k) route_feat gave this lookup
            # dest_req naming its own cell: the word comes back whatever the rank
            cell = np.arange(world * n * capf, dtype=np.int32).reshape(world, n, capf)
            got = S.shard_dest_combine(slot, cell, n, B, capf, 1 << 19, rank, shift).astype(np.int64)
            o, c = got >> shift, got & ((1 << shift) - 1)
            live = slot >= 0
            assert np.array_equal(o[live], c[live] // (n * capf))
            assert np.array_equal(send_pos.reshape(-1)[c[live]], np.broadcast_to(np.arange(B), (n, B))[live])


def test_scatter_multi_split_partitions_the_destinations():
    rng = np.random.default_rng(12)
    for shift, n_bases in ((12, 1), (12, 8), (25, 64), (30, 2)):
        rows = min(1 << shift, 5000)
        dest = (rng.integers(0, n_bases, 3000) << shift) | rng.integers(0, rows, 3000)
        dest[rng.random(3000) < 0.1] = -1
        per_base = S.scatter_multi_split(dest, shift, n_bases)
        named = np.stack([x >= 0 for x in per_base])
        assert np.array_equal(named.sum(0), (dest >= 0).astype(np.int64))            # every destination in exactly one base, -1 in none
        for x, d in enumerate(per_base):
            assert np.array_equal((np.int64(x) << shift) | d[named[x]], dest[named[x]])
