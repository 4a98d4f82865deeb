"""Definitions, kernel-order restatements, error bounds and case lists for the standalone FM and bag-pooling kernels of
csrc/nrx_interact.hip (nrx_fm_fwd, nrx_fm_fwd_train, nrx_fm_bwd, nrx_bag_pool_fwd, nrx_bag_pool_bwd).  numpy only: tests/test_fm_pool_ref.py holds
this file to oracle/ref_np.py and the committed goldens on the CPU, tests/test_fm_pool_kernels_gpu.py holds the kernels to this file.

Layout: the kernels take the FM concat flat, [B, F*D]; here it is [B, F, D].  Column 0 of a field is its first-order weight w_f, columns
1..D-1 its factor v_f (FM.get_inp_embedding, src/model/sort/fm/model.py:48-59).

Three kinds of function:
  *64   the definition in float64 (the formulas of oracle/ref_np.py: fm_logit, fm_logit_bwd, array_pool, array_pool_bwd);
  *32   the kernel's own float32 arithmetic in the kernel's own order, for the quantities where no multiply sits next to an add (nothing the
        compiler could fuse): the GPU test asks for these bit for bit;
  *_bound   a bound on |kernel - definition| for the rest, from counting the roundings in the source (u = 2^-24, unit roundoff of float32).
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
EPS32 = F32(1e-8)                       # the pooling denominator's epsilon as the kernels (and the reference, on float32 tensors) add it
NRX_BLOCK = 256


def gamma(n):
    """(1 + u)^n - 1 <= n u / (1 - n u): the exact form of 'n roundings'."""
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------- launch arithmetic (nrx_interact.hip)
def fm_qlog2(D):
    """Lanes per sample = 2^QLOG2 = the power of two >= the number of four-column chunks, at most 64 (then the kernel loops)."""
    chunks, ql = (D + 3) // 4, 0
    while (1 << ql) < chunks:
        ql += 1
    return min(ql, 6)


def fm_tb(D):
    """Samples per 256-thread block."""
    return NRX_BLOCK >> fm_qlog2(D)


def fm_passes(D):
    return -(-D // (4 << fm_qlog2(D)))


# (F, D): what it reaches
FM_PAIRS = [
    (1, 1), (2, 2), (7, 3), (8, 4),          # QLOG2 0: D = 1 (first-order only), odd widths, one full chunk
    (9, 5), (3, 8),                          # QLOG2 1
    (16, 12), (26, 16),                      # QLOG2 2: three of four lanes live; the production width
    (17, 17), (5, 20), (7, 32),              # QLOG2 3: odd, five of eight lanes live, full
    (3, 33), (9, 64),                        # QLOG2 4
    (8, 100), (4, 128),                      # QLOG2 5
    (3, 132), (2, 256),                      # QLOG2 6, one pass
    (3, 260), (2, 300), (2, 516),            # QLOG2 6, two / two / three passes: the last pass holds 1, 11 and 1 chunks
    (70, 16),                                # more than 64 fields (ops.embed_apply runs the FM on the concat)
]
FM_VARIANT_PAIRS = [(26, 16), (7, 32), (9, 64), (4, 128), (3, 260)]      # D % 4 == 0: the layout variants (vector against scalar loads / stores)
FM_MAX_ELEMS = 1 << 20


def fm_batches(F, D):
    """1, tb - 1, tb, tb + 1 and 3 tb + 5 samples: one partial block, a block short of one sample, a full block, a second block holding one sample,
    four blocks with a ragged last one -- the largest dropped while B F D is above about a million elements."""
    tb = fm_tb(D)
    bs = sorted({b for b in (1, tb - 1, tb, tb + 1, 3 * tb + 5) if b >= 1})
    while len(bs) > 1 and bs[-1] * F * D > FM_MAX_ELEMS:
        bs.pop()
    return bs


def fm_seed(F, D, B):
    return [20, F, D, B]


def fm_inputs(F, D, B):
    """feat [B, F, D] (v scaled by 0.7 as the goldens' generator does), the logit's upstream gradient gl [B], the concat's upstream gradient
    g_in [B, F, D]."""
    rng = np.random.default_rng(fm_seed(F, D, B))
    feat = rng.standard_normal((B, F, D)).astype(F32)
    feat[:, :, 1:] *= F32(0.7)
    gl = rng.standard_normal(B).astype(F32)
    g_in = rng.standard_normal((B, F, D)).astype(F32)
    return feat, gl, g_in


# (B, L, D): what it reaches
POOL_CASES = [
    (1, 1, 1), (5, 3, 3), (9, 6, 16),        # small shapes
    (5, 50, 17),                             # odd width (the scalar backward)
    (7, 64, 4),                              # L exactly one wavefront
    (7, 65, 8), (5, 130, 16),                # second and third trip of the backward's lane loop over the mask
    (5, 3, 100),                             # wide rows
    (8193, 3, 64),                           # both grid-stride loops repeat: the forward by 64 elements (B D = 2048 * 256 + 64), the backward by one sample
    (8193, 2, 3),                            # the scalar backward wraps (2048 * 4 wavefronts + 1)
]
POOL_MASKS = ["none", "bin", "w"]
POOL_GRID_CAP = 2048                          # stream_grid(): at most 8 blocks per CU x 256 CUs


def pool_inputs(B, L, D):
    """emb [B, L, D], the upstream gradient up [B, D], a binary mask [B, L] (row 0 all zero, row 1 full, every later row a random subset of
    1..L-1 positions when L >= 2) and a weighted mask rand * binary.  Masks are non-negative, as the reference's are."""
    rng = np.random.default_rng([21, B, L, D])
    emb = rng.standard_normal((B, L, D)).astype(F32)
    up = rng.standard_normal((B, D)).astype(F32)
    n = rng.integers(1, max(2, L), B)                     # L = 1: a row is empty or full, nothing between
    n[0] = 0
    if B > 1:
        n[1] = L
    rank = rng.random((B, L)).argsort(axis=1).argsort(axis=1)
    binary = (rank < n[:, None]).astype(F32)
    weighted = (rng.random((B, L)).astype(F32) * binary).astype(F32)
    return emb, up, {"none": None, "bin": binary, "w": weighted}


# ------------------------------------------------------------------------------------------------- float64 definitions
def fm_logit64(feat):
    """sum_f w_f + 1/2 sum_k [(sum_f v_fk)^2 - sum_f v_fk^2]   -> [B]"""
    x = feat.astype(np.float64)
    w, v = x[:, :, 0], x[:, :, 1:]
    return w.sum(1) + 0.5 * ((v.sum(1) ** 2) - (v ** 2).sum(1)).sum(1)


def fm_sums64(feat):
    """[B, D]: column 0 sum_f w_f, column k sum_f v_fk."""
    return feat.astype(np.float64).sum(1)


def fm_grad64(feat, gl, g_in=None):
    """[B, F, D]: g_w = gl, g_v = gl (S_k - v_fk), plus the upstream gradient of the concat when there is one."""
    x = feat.astype(np.float64)
    g = gl.astype(np.float64)[:, None, None] * (x.sum(1, keepdims=True) - x)
    g[:, :, 0] = gl.astype(np.float64)[:, None]
    return g if g_in is None else g + g_in.astype(np.float64)


def pool_den64(mask, B, L):
    if mask is None:
        return np.full(B, float(L))
    return mask.astype(np.float64).sum(1) + np.float64(EPS32)


def pool_fwd64(emb, mask):
    """mask: sum_l e m / (sum_l m + 1e-8); none: the mean over L.   -> [B, D]"""
    e = emb.astype(np.float64)
    B, L, _ = e.shape
    if mask is None:
        return e.sum(1) / float(L)
    return (e * mask.astype(np.float64)[:, :, None]).sum(1) / pool_den64(mask, B, L)[:, None]


def pool_bwd64(up, mask, L):
    """g m / den   -> [B, L, D]"""
    g = up.astype(np.float64)
    B = g.shape[0]
    m = np.ones((B, L)) if mask is None else mask.astype(np.float64)
    return (g / pool_den64(mask, B, L)[:, None])[:, None, :] * m[:, :, None]


# ------------------------------------------------------------------------------------------------- float32 restatements (bit for bit)
def fm_sums32(feat):
    """fm_fwd_kernel / fm_bwd_kernel: one lane owns a column and adds the fields in order f = 0..F-1, starting from 0.f."""
    s = np.zeros((feat.shape[0], feat.shape[2]), F32)
    for f in range(feat.shape[1]):
        s = s + feat[:, f, :]
    return s


def fm_grad32(feat, gl):
    """fm_bwd_kernel without g_in: 0.f + fp32(gl * fp32(S - v)), gl itself in column 0.  (The product is rounded once whether or not the compiler
    fuses it with the add of the zero upstream: fma(gl, d, 0) = fp32(gl d).)"""
    S = fm_sums32(feat)
    g = (gl[:, None, None] * (S[:, None, :] - feat).astype(F32)).astype(F32) + F32(0)
    g[:, :, 0] = gl[:, None] + F32(0)
    return g


def pool_fwd32(emb, mask):
    """bag_pool_fwd_kernel: one thread per (b, d), l in order.  With a mask acc += fp32(e w), den += w (contraction is switched off in that loop),
    out = acc / fp32(den + 1e-8f); without one acc += e, out = acc / float(L): one correctly rounded division."""
    B, L, D = emb.shape
    acc = np.zeros((B, D), F32)
    if mask is None:
        for l in range(L):
            acc = acc + emb[:, l, :]
        return (acc / F32(L)).astype(F32)
    den = np.zeros(B, F32)
    for l in range(L):
        w = mask[:, l]
        den = den + w
        acc = acc + (emb[:, l, :] * w[:, None]).astype(F32)
    return (acc / (den + EPS32).astype(F32)[:, None]).astype(F32)


def pool_bwd32(up, mask, L):
    """bag_pool_bwd_kernel with no mask or a BINARY mask -- den is then a small integer whatever the order of the wavefront's sum:
    fp32(fp32(g / den) * m), den = float(L) or fp32(count + 1e-8f)."""
    B, D = up.shape
    if mask is None:
        return np.broadcast_to((up / F32(L)).astype(F32)[:, None, :], (B, L, D)).copy()
    assert np.all((mask == 0) | (mask == 1)), "the restatement pins the bits for binary masks only"
    den = (mask.sum(1, dtype=np.float64).astype(F32) + EPS32).astype(F32)
    return ((up / den[:, None]).astype(F32)[:, None, :] * mask[:, :, None]).astype(F32)


def _fma(a, b, c):
    """fp32(a b + c) with one rounding (the product of two float32 is exact in float64; the second rounding float64 -> float32 differs from a
    true fused result in far fewer cases than matter to a bound check)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def fm_logit32(feat, fma):
    """fm_fwd_kernel's logit in its own order: lane q of a sample's 2^QLOG2 lanes owns columns kc + 4q .. +3 of every pass kc, chains s, sq (and
    `first` for column 0) over the fields, adds 0.5 ((sx sx - sqx) + (sy sy - sqy) + (sz sz - sqz) + (sw sw - sqw)) + first to its total,
    and the lanes' totals meet in a butterfly (total += total of lane ^ off, off = Q/2 .. 1).  fma: every multiply next to an add fused, as
    the compiler may; the bits the GPU gives lie somewhere between the two, which is why the logit has a bound and no bit equality."""
    B, F, D = feat.shape
    Q = 1 << fm_qlog2(D)
    P = fm_passes(D)
    x = np.zeros((B, F, P * Q * 4), F32)                  # (columns past D load as 0.f in the kernel too: they add exact zeros)
    x[:, :, :D] = feat
    x = x.reshape(B, F, P, Q, 4)
    total = np.zeros((B, Q), F32)
    half = F32(0.5)
    for p in range(P):
        v = x[:, :, p].copy()                             # [B, F, Q, 4]
        first = np.zeros((B, Q), F32)
        if p == 0:
            for f in range(F):
                first[:, 0] = first[:, 0] + v[:, f, 0, 0]
            v[:, :, 0, 0] = 0
        s = np.zeros((B, Q, 4), F32)
        sq = np.zeros((B, Q, 4), F32)
        for f in range(F):
            s = s + v[:, f]
            sq = _fma(v[:, f], v[:, f], sq) if fma else sq + (v[:, f] * v[:, f]).astype(F32)
        t = _fma(s, s, -sq) if fma else (s * s).astype(F32) - sq
        inner = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
        total = total + (_fma(np.broadcast_to(half, inner.shape), inner, first) if fma else (half * inner).astype(F32) + first)
    off = Q // 2
    lanes = np.arange(Q)
    while off > 0:
        total = total + total[:, lanes ^ off]
        off >>= 1
    return total[:, 0].copy()


def fm_grad32_up(feat, gl, g_in, fma):
    """fm_bwd_kernel with g_in: up + gl * (S - v), the product fused into the add or not."""
    S = fm_sums32(feat)
    d = (S[:, None, :] - feat).astype(F32)
    glb = np.broadcast_to(gl[:, None, None], d.shape)
    g = _fma(glb, d, g_in) if fma else g_in + (glb * d).astype(F32)
    g[:, :, 0] = g_in[:, :, 0] + gl[:, None]
    return g


def pool_bwd32_lanes(up, mask, L):
    """bag_pool_bwd_kernel with any mask, the wavefront's sum in the kernel's order: lane l adds m[l], m[l + 64], ...; lane ^ 1, lane ^ 2, the other
    quad of each 8, the other half of each 16, then (r0 + r1) + (r2 + r3) over the four rows of 16."""
    B, D = up.shape
    T = -(-L // 64)
    m = np.zeros((B, T * 64), F32)
    m[:, :L] = mask
    part = np.zeros((B, 64), F32)
    for t in range(T):
        part = part + m[:, t * 64:(t + 1) * 64]
    lanes = np.arange(64)
    for perm in (lanes ^ 1, lanes ^ 2, (lanes & ~7) | (7 - (lanes & 7)), (lanes & ~15) | (15 - (lanes & 15))):
        part = part + part[:, perm]
    den = ((part[:, 0] + part[:, 16]) + (part[:, 32] + part[:, 48]) + EPS32).astype(F32)
    return ((up / den[:, None]).astype(F32)[:, None, :] * mask[:, :, None]).astype(F32)


# ------------------------------------------------------------------------------------------------- derived bounds
def fm_logit_n(F, D):
    """Roundings on the longest path to the logit, counted in fm_fwd_kernel (P = passes = ceil(D / 256) once D > 256, else 1):
      the squared sum   2 (F - 1)  [the chain s, F - 1 roundings, counted twice: s s]  + 1 [the square] + 1 [minus sq] + 3 [the four columns added]
                        + 0 [times 0.5: exact] + 1 [plus first] + P [total +=] + 6 [the butterfly over at most 64 lanes]           = 2 F + P + 10
      the sum of squares  1 [v v] + F [the chain sq] + 1 + 3 + 0 + 1 + P + 6                                                       = F + P + 12
      the first order     F - 1 [the chain] + 1 + P + 6                                                                            = F + P + 6
    The issue's F + ceil(D/256) + 12 is the second line; the first is longer from F = 3 on, so the counted constant is their maximum,
    2 F + P + 12 (above both for every F >= 1)."""
    return 2 * F + fm_passes(D) + 12


def fm_logit_scale(feat):
    """M_i = sum_f |w_f| + sum_k [(sum_f |v_fk|)^2 + sum_f v_fk^2]: what the roundings are relative to."""
    x = np.abs(feat.astype(np.float64))
    w, v = x[:, :, 0], x[:, :, 1:]
    return w.sum(1) + ((v.sum(1) ** 2) + (v ** 2).sum(1)).sum(1)


def fm_logit_bound(feat):
    """|got - fm_logit64| <= gamma(n) M_i per sample."""
    _, F, D = feat.shape
    return gamma(fm_logit_n(F, D)) * fm_logit_scale(feat)


def fm_grad_up_bound(feat, gl, g_in):
    """|got - fm_grad64(feat, gl, g_in)| <= u (3 (|up| + |gl| (|S_k| + |v_fk|)) + F |gl| sum_f |v_fk|) per element: S carries F - 1 roundings of a
    sum bounded by sum_f |v_fk| (the F term), then S - v, gl *, up + are three more on magnitudes bounded by the first term (two when fused).
    Column 0 is up + gl, one rounding: u (|up| + |gl|)."""
    x = feat.astype(np.float64)
    F = x.shape[1]
    a = np.abs(gl.astype(np.float64))[:, None, None]
    S = x.sum(1, keepdims=True)
    b = U * (3 * (np.abs(g_in.astype(np.float64)) + a * (np.abs(S) + np.abs(x))) + F * a * np.abs(x).sum(1, keepdims=True))
    b[:, :, 0] = U * (np.abs(g_in[:, :, 0].astype(np.float64)) + a[:, :, 0])
    return b


def pool_bwd_weighted_rtol(L):
    """Relative error of g m / den with a non-negative weighted mask (no cancellation in den): ceil(L/64) - 1 roundings in a lane's chain, 6 in the
    wavefront's tree, 1 for + 1e-8f, the division, the multiply = ceil(L/64) + 8 counted; the issue's ceil(L/64) + 10 keeps two more for the
    second-order terms of the product of roundings."""
    return (-(-L // 64) + 10) * U


# ------------------------------------------------------------------------------------------------- structural mistakes the bounds must not hide
def mut_logit_field_dropped(feat):
    """The last field missing from S (its square still subtracted)."""
    x = feat.astype(np.float64)
    w, v = x[:, :, 0], x[:, :, 1:]
    return w.sum(1) + 0.5 * ((v[:, :-1].sum(1) ** 2) - (v ** 2).sum(1)).sum(1)


def mut_logit_squares_kept(feat):
    x = feat.astype(np.float64)
    return x[:, :, 0].sum(1) + 0.5 * (x[:, :, 1:].sum(1) ** 2).sum(1)


def mut_logit_no_half(feat):
    x = feat.astype(np.float64)
    w, v = x[:, :, 0], x[:, :, 1:]
    return w.sum(1) + ((v.sum(1) ** 2) - (v ** 2).sum(1)).sum(1)


def mut_logit_first_order_in_column_1(feat):
    x = feat.astype(np.float64)
    return fm_logit64(np.concatenate([x[:, :, 1:2], x[:, :, 0:1], x[:, :, 2:]], axis=2))


def mut_grad_sum_not_reduced(feat, gl, g_in=None):
    """S where S - v_f belongs."""
    x = feat.astype(np.float64)
    g = gl.astype(np.float64)[:, None, None] * np.broadcast_to(x.sum(1, keepdims=True), x.shape)
    g[:, :, 0] = gl.astype(np.float64)[:, None]
    return g if g_in is None else g + g_in.astype(np.float64)


def mut_pool_den_without_mask(emb, mask):
    e = emb.astype(np.float64)
    return (e * mask.astype(np.float64)[:, :, None]).sum(1) / float(e.shape[1])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
