"""The per-feature shard kernels' definitions in numpy (csrc/nrx_route_feat.hip, and the destination word of the direct-gradient backward in
csrc/nrx_embed.hip), as include/nrx_embed.h states them: tests/test_shard_feat_kernels_gpu.py holds the kernels to these, bit for bit, and
tests/test_shard_feat_ref.py holds these to hand-written cases and to oracle/ref_np.py (route_feat, whose slot word shard_dest_combine decodes).
nrx_route_feat and nrx_inbox_transpose are defined by oracle/ref_np.py itself (route_feat, owner_ids_from_inbox).

Rows travel as BIT PATTERNS (uint32): a copy has no arithmetic, and a NaN planted in a row nobody may read compares like any other word."""
import numpy as np

I32MAX = (1 << 31) - 1
SENTINEL = np.uint32(0xFFFFFFFF)              # what every output buffer of the GPU tests holds before a launch


def widen_bf16(bits16) -> np.ndarray:
    """bf16 bit patterns -> the fp32 bit patterns of the same numbers (exact: the upper half of the word)."""
    return np.asarray(bits16, np.uint16).astype(np.uint32) << np.uint32(16)


def arena_bits(arena) -> np.ndarray:
    """An arena as fp32 bit patterns [rows, dim]: float32 (or uint32 words) as they are, uint16 = bf16 bit patterns widened exactly."""
    arena = np.asarray(arena)
    if arena.dtype == np.uint16:
        return widen_bf16(arena)
    assert arena.dtype in (np.float32, np.uint32), arena.dtype
    return np.ascontiguousarray(arena).view(np.uint32)


def gather_place_feat(arenas, rows, cols, oid, opos, world, capf, dim, outs, out_rows):
    """Definition of nrx_gather_place_feat(_bf16).  oid / opos: int32 [n, world * capf]; arenas[f]: [>= rows[f], dim] (arena_bits' types);
    outs[s]: the requester s's buffer, a 2-D float32 / uint32 array of at least out_rows rows, written IN PLACE as bit patterns.  For every
    (f, b') with 0 <= opos[f, b'] < out_rows:  outs[b' // capf][opos, cols[f] : cols[f] + dim] = arenas[f][oid] when 0 < oid < rows[f], else zeros
    (owner id 0 -- the padding id, the arena's dummy row -- always writes zeros, whatever row 0 holds).  Nothing else is written.
    Returns (count, reports): one report per id outside [0, rows[f]) at a live position (opos >= 0), and one per position >= out_rows -- an
    entry that is both is reported for both -- and the set of (feature, b', value) triples those reports carry: status[0] is the count, and
    status[1..3] is whichever triple arrived first."""
    oid, opos = np.asarray(oid, np.int64), np.asarray(opos, np.int64)
    n, bp = oid.shape
    assert opos.shape == (n, bp) and bp == world * capf and len(arenas) == len(rows) == len(cols) == n and len(outs) == world
    views = [o.view(np.uint32) for o in outs]
    for v, o in zip(views, outs):
        assert np.shares_memory(v, o) and o.ndim == 2 and o.shape[0] >= out_rows
    count, reports = 0, set()
    for f in range(n):
        tab = arena_bits(arenas[f])
        live = opos[f] >= 0
        bad_id = live & ((oid[f] < 0) | (oid[f] >= rows[f]))
        bad_pos = live & (opos[f] >= out_rows)
        for b in np.flatnonzero(bad_id):
            reports.add((f, int(b), int(oid[f, b])))
        for b in np.flatnonzero(bad_pos):
            reports.add((f, int(b), int(opos[f, b])))
        count += int(bad_id.sum()) + int(bad_pos.sum())
        b = np.flatnonzero(live & ~bad_pos)
        reads = ~bad_id[b] & (oid[f, b] != 0)
        vals = np.zeros((b.size, dim), np.uint32)
        vals[reads] = tab[oid[f, b[reads]], :dim]
        s = b // capf
        for peer in range(world):
            m = s == peer
            views[peer][opos[f, b[m]], cols[f]:cols[f] + dim] = vals[m]
    return count, reports


def shard_dest_combine(slot, dest_req, n, batch, capf, recv_row0, rank, shift) -> np.ndarray:
    """Definition of nrx_shard_dest_combine.  slot: int32 [n, batch] (nrx_route_feat's: (o * capf + k) * n + f, -1 = dropped); dest_req: int32
    [world, n, capf] (the owners' plan destinations in send_ids' layout).  slot < 0 -> -1; else ok = slot // n, o = ok // capf, k = ok % capf,
    d = dest_req[o, f, k], row = d if d >= 0 else recv_row0 + (rank * capf + k) * n + f, result (o << shift) | row.  int32 [n, batch]."""
    slot = np.asarray(slot, np.int64).reshape(n, batch)
    dest_req = np.asarray(dest_req, np.int64)
    assert dest_req.ndim == 3 and dest_req.shape[1:] == (n, capf)
    f = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], slot.shape)
    live = slot >= 0
    ok = np.where(live, slot, 0) // n
    o, k = ok // capf, ok % capf
    d = dest_req[o, f, k]
    row = np.where(d >= 0, d, recv_row0 + (rank * capf + k) * n + f)
    res = np.where(live, (o << shift) | row, -1)
    assert res.max(initial=-1) <= I32MAX and res.min(initial=0) >= -1
    return res.astype(np.int32)


def scatter_multi_split(dest, shift, n_bases):
    """nrx_embed_bwd_scatter_multi's dest word taken apart: per base the dest array of a single-buffer nrx_embed_bwd_scatter -- the row where
    dest >> shift == base, else -1 (a negative dest names no base)."""
    dest = np.asarray(dest, np.int64)
    base = np.where(dest >= 0, dest >> shift, -1)
    assert base.max(initial=-1) < n_bases
    row = dest & ((1 << shift) - 1)
    return [np.where(base == x, row, -1).astype(np.int32) for x in range(n_bases)]
