"""Definitions, launch arithmetic, exactness condition, error bounds, mutants and case lists for the DCN-v1 kernels of csrc/nrx_interact.hip
(nrx_dcn_v1_fwd, nrx_dcn_v1_bwd, nrx_dcn_v1_bwd_ordered + dcn_v1_reduce_kernel, nrx_embed_dcn_v1_fwd).  numpy only: tests/test_dcn_v1_ref.py holds
this file to oracle/ref_np.py, the goldens and float64 autograd on the CPU, tests/test_dcn_v1_kernels_gpu.py holds the kernels to this file.

The operation: x_{l+1} = z (x_l . w_l) + b_l + x_l for l = 0 .. NL-1, where z is the layer-0 input: x itself, or a separate x0 (the stack then
starts from a later x_l).  The backward, top down from g = dL/dx_NL (the comment above dcn_v1_bwd_kernel):
    gs = g . z;   g_b[l] = sum_rows g;   g_w[l] = sum_rows gs x_l;   gx0 += g s_l;   g <- g + gs w_l
and at the end g_x = g + gx0 when z is x, else g_x = g and g_x0 = gx0.  NL = 0 is the identity and has no weight gradients.

Three ways of holding a kernel to that:
  * integer inputs under the exactness condition (int_exact_margin): every sum the kernel can form has a sum of |terms| below 2^24, so every
    float32 operation is exact in any order, fused or not, atomics included -- the kernel must give dcn()'s int64 result bit for bit;
  * real inputs: |kernel - float64| <= bounds(), a running recurrence over the layers evaluated next to the float64 values, from the roundings
    counted in the source (listed at bounds());
  * MUTANTS: structural mistakes that both of the above must expose."""
import numpy as np

from tests.fm_pool_ref import F32, U, gamma, same_bits      # noqa: F401  (U, same_bits: for the two test files)

MAX_LAYERS = 8                   # NRX_MAX_DCN_LAYERS
MAX_DIM = 2048
LDS_FWD = 64 * 1024              # nrx_dcn_v1_fwd / nrx_embed_dcn_v1_fwd: w, b staged in LDS
LDS_BWD = 128 * 1024             # nrx_dcn_v1_bwd: w, b, g_w, g_b (+ slabs)
STREAM_CAP = 2048                # stream_grid(): 8 blocks x 256 CUs
REDUCE_MAX_BLOCKS = 1024         # DCN_V1_MAX_BLOCKS: slots of the ordered mode's scratch
EXACT = 1 << 24


def dp(D):
    return (D + 3) & ~3


# ------------------------------------------------------------------------------------------------- launch arithmetic (nrx_interact.hip)
def lanes(D, vec):
    """(V, R, RR): floats per load, chunks per lane the row needs, chunks per lane of the instantiation NRX_RSWITCH picks."""
    assert 1 <= D <= MAX_DIM and (not vec or D % 4 == 0)
    V = 4 if vec else 1
    R = -(-D // (64 * V))
    RR = next(r for r in ((1, 2, 4, 8) if vec else (1, 2, 4, 8, 16, 32)) if R <= r)
    return V, R, RR


def dot_roundings(D, vec):
    """row_dot: a lane chains its R V products onto 0.f (a product, then R V - 1 adds that can round), then the wavefront's tree: four DPP steps
    and (r0 + r1) + (r2 + r3), 6 adds -- or r0 + r1 of the row's own half, 5 adds, with two rows per wavefront."""
    V, R, _ = lanes(D, vec)
    return R * V + (5 if vec and D <= 128 else 6)


def fwd_form(D, NL, vec):
    """nrx_dcn_v1_fwd: 256 threads; vector rows of <= 128 floats go two per wavefront (8 rows per block), every other row one per wavefront (4);
    stream_grid caps the grid at 2048 blocks."""
    V, R, RR = lanes(D, vec)
    half = vec and D <= 128
    smem = 2 * NL * dp(D) * 4
    rpb = 8 if half else 4
    return dict(ok=smem <= LDS_FWD, V=V, R=1 if half else RR, half=half, threads=256, rpb=rpb, cap=STREAM_CAP, pass_rows=STREAM_CAP * rpb, smem=smem)


def bwd_form(D, NL, vec, sep):
    """dcn_v1_bwd_impl.  body: 'reg' (g_w / g_b of a wavefront's rows in registers, 1..4 layers and <= 2 chunks per lane; with a separate x0 only
    for ONE layer), 'slab' (a per-wavefront LDS slab [NL][2][Dp]), 'atomic' (per-row LDS atomics, when the slabs do not fit 128 KB)."""
    V, R, RR = lanes(D, vec)
    half = vec and D <= 128
    rpw = 2 if half else 1
    nlr = NL if 1 <= NL <= 4 and R <= 2 else 0
    Dp = dp(D)
    smem = (4 * NL + (2 * (32 if half else 16) if nlr else 0)) * Dp * 4
    gen_smem = (4 * NL + (8 if half else 4) * NL * 2) * Dp * 4
    ok = smem <= LDS_BWD
    if sep and not (NL == 1 and R <= 2):
        nlr = 0
    if nlr:
        threads = 1024 if nlr <= 2 else 512
        body, cap, use = "reg", 256 * (1024 // threads), smem
        RR = min(RR, 2)
    elif half or gen_smem <= LDS_BWD:
        body, threads, cap, use = "slab", 256, 512, gen_smem
    else:
        body, threads, cap, use = "atomic", 512, 512, smem
    rpb = threads // 64 * rpw
    return dict(ok=ok, body=body, V=V, R=1 if half else RR, half=half, threads=threads, rpb=rpb, cap=cap, pass_rows=cap * rpb, smem=use)


def ordered_takes(D, NL):
    """nrx_dcn_v1_bwd_ordered refuses (NRX_ERR_UNSUPPORTED) what would run the atomic body -- decided from dim alone, before the pointers are
    looked at."""
    if NL == 0:
        return True
    vec = D % 4 == 0
    gen_smem = (4 * NL + (8 if vec and D <= 128 else 4) * NL * 2) * dp(D) * 4
    return gen_smem <= LDS_BWD or (NL <= 4 and -(-D // (64 * (4 if vec else 1))) <= 2)


def fused_form(dims, batch=None):
    """nrx_embed_dcn_v1_fwd.  Uniform rows of 32 / 64 floats, 2..8 features: the grouped persistent kernel (Q lanes per sample, TB samples per
    block, at most 256 x 16 resident blocks).  Everything else: one wavefront per S samples, R chunks per lane, grid = stream_grid(ceil(B/8), 4)."""
    W, D0 = sum(dims), dims[0]
    if D0 in (32, 64) and 2 <= len(dims) <= 8 and all(d == D0 for d in dims):
        Q = D0 // 4
        return dict(kernel="group_persist", Q=Q, TB=256 // Q, cap=4096, pass_rows=4096 * (256 // Q))
    R = -(-W // 256)
    RR, S = next((r, s) for r, s in ((1, 8), (2, 8), (4, 4), (8, 2)) if R <= r)
    form = dict(kernel="general", R=RR, S=S, cap=STREAM_CAP)
    if batch is not None:
        grid = min(STREAM_CAP, max(1, -(-(-(-batch // 8)) // 4)))
        form.update(grid=grid, pass_rows=grid * 4 * S)
    return form


def edge_batches(rpb):
    """One partial block, a block short of one row, a full block, a second block holding one row, four blocks with a ragged last one.  Odd
    batches leave the upper half of the last wavefront idle where two rows share one."""
    return sorted({b for b in (1, rpb - 1, rpb, rpb + 1, 3 * rpb + 5) if b >= 1})


# ------------------------------------------------------------------------------------------------- the definition (int64 or float64) and its mutants
MUTANTS = ("bias_dropped",              # layer 0's bias dropped
           "xl_in_hadamard",            # x_l where z belongs in z (x_l . w_l)
           "dot_short",                 # the last column left out of x_l . w_l
           "gw_last_row",               # the last row left out of g_w
           "gx0_term_missing",          # layer 0's term missing from gx0
           "w_next_in_g",               # w_{l+1} where w_l belongs in g <- g + gs w_l
           "pair_scalar")               # the second row of a pair given the first row's x_l . w_l
# the outputs a mutant must show up in, and what it needs to differ from the definition at all
MUTANT_SHOWS = {"bias_dropped": ("out",), "xl_in_hadamard": ("out",), "dot_short": ("out",), "gw_last_row": ("g_w",),
                "gx0_term_missing": ("g_x0", "g_x"), "w_next_in_g": ("g_x",), "pair_scalar": ("out",)}


def mutant_applies(mut, D, NL, B, sep):
    return {"bias_dropped": NL >= 1, "xl_in_hadamard": NL >= 2 or (sep and NL >= 1), "dot_short": NL >= 1 and D >= 2, "gw_last_row": NL >= 1 and B >= 2,
            "gx0_term_missing": NL >= 1, "w_next_in_g": NL >= 2, "pair_scalar": NL >= 1 and B >= 2}[mut]


def dcn(x, w, b, g=None, x0=None, mut=None):
    """The definition.  Integer arrays are evaluated in int64 (exact), everything else in float64.  Returns out, and with an upstream gradient g
    also g_x, g_x0 (None when z is x), g_w, g_b."""
    T = np.int64 if np.asarray(x).dtype.kind == "i" else np.float64
    x, w, b = np.asarray(x, T), np.asarray(w, T), np.asarray(b, T)
    sep = x0 is not None
    z = np.asarray(x0, T) if sep else x
    NL, D = w.shape[0], x.shape[1]
    xs, ss = [x], []
    for l in range(NL):
        xl = xs[-1]
        s = (xl[:, :-1] * w[l, :-1]).sum(1, keepdims=True) if mut == "dot_short" else (xl * w[l]).sum(1, keepdims=True)
        if mut == "pair_scalar":
            s = s.copy()
            s[1::2] = s[0::2][:s[1::2].shape[0]]
        bias = 0 if (mut == "bias_dropped" and l == 0) else b[l]
        xs.append((xl if mut == "xl_in_hadamard" else z) * s + bias + xl)
        ss.append(s)
    res = dict(out=xs[-1])
    if g is None:
        return res
    g = np.asarray(g, T)
    gx0 = np.zeros_like(x)
    gw, gb = np.zeros((NL, D), T), np.zeros((NL, D), T)
    for l in reversed(range(NL)):
        gs = (g * z).sum(1, keepdims=True)
        gb[l] = g.sum(0)
        t = gs * xs[l]
        gw[l] = (t[:-1] if mut == "gw_last_row" else t).sum(0)
        if not (mut == "gx0_term_missing" and l == 0):
            gx0 = gx0 + g * ss[l]
        g = g + gs * w[(l + 1) % NL if mut == "w_next_in_g" else l]
    res.update(g_x=g if sep else g + gx0, g_x0=gx0 if sep else None, g_w=gw, g_b=gb)
    return res


OUTPUTS = ("out", "g_x", "g_x0", "g_w", "g_b")


# ------------------------------------------------------------------------------------------------- integer-exact inputs
def int_inputs(D, NL, B, density):
    """x, x0, w, b, g with entries in {-1, 0, 1}, non-zero with probability `density` (int64)."""
    rng = np.random.default_rng([30, D, NL, B])

    def draw(*shape):
        return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < density)

    i = dict(x=draw(B, D), x0=draw(B, D), w=draw(NL, D), b=draw(NL, D), g=draw(B, D))
    # whatever the density: the last column of x and w is +-1, and in the last row g is the unit vector of column 0 with x = x0 = 1 there (so
    # g . z = 1 and g_w[NL - 1][0] gets that row's x) -- a kernel that leaves out the last column of a dot product or the last row of a batch
    # sum cannot agree by meeting zeros
    i["x"][:, -1], i["w"][:, -1] = rng.integers(0, 2, B) * 2 - 1, rng.integers(0, 2, NL) * 2 - 1
    i["g"][-1] = 0
    i["g"][-1, 0] = i["x"][-1, 0] = i["x0"][-1, 0] = 1
    return i


def int_exact_margin(x, w, b, g, x0=None):
    """The largest sum of |terms| over every sum the kernels form: the dot products x_l . w_l and g . z, the row update z s + b + x_l, the
    updates of g (g + gs w_l) and of gx0 (the running sum of g s_l, and g + gx0 at the end), and the batch sums g_w / g_b.  Below 2^24 every
    partial sum in any order is an integer below 2^24 -- exactly representable, so no float32 operation rounds (and every product is a term of
    one of these sums, so it is below 2^24 too)."""
    x, w, b, g = (np.asarray(a, np.int64) for a in (x, w, b, g))
    z = x if x0 is None else np.asarray(x0, np.int64)
    NL = w.shape[0]
    m = int(max(np.abs(x).max(initial=0), np.abs(g).max(initial=0)))
    xs, ss = [x], []
    for l in range(NL):
        xl = xs[-1]
        s = (xl * w[l]).sum(1, keepdims=True)
        m = max(m, int((np.abs(xl) * np.abs(w[l])).sum(1).max()), int((np.abs(z) * np.abs(s) + np.abs(b[l]) + np.abs(xl)).max()))
        xs.append(z * s + b[l] + xl)
        ss.append(s)
    k_abs = np.zeros_like(x)
    for l in reversed(range(NL)):
        gs = (g * z).sum(1, keepdims=True)
        k_abs = k_abs + np.abs(g) * np.abs(ss[l])
        m = max(m, int((np.abs(g) * np.abs(z)).sum(1).max()), int(np.abs(g).sum(0).max()), int((np.abs(gs) * np.abs(xs[l])).sum(0).max()),
                int((np.abs(g) + np.abs(gs) * np.abs(w[l])).max()))
        g = g + gs * w[l]
    return max(m, int((np.abs(g) + k_abs).max()))


# ------------------------------------------------------------------------------------------------- real-valued inputs and bounds
def real_inputs(D, NL, B):
    """The distribution of tests/test_hip_parity.py::test_dcn_v1_vs_oracle: rows and upstream gradient N(0, 1), w ~ N / sqrt(D), b ~ 0.1 N."""
    rng = np.random.default_rng([31, D, NL, B])
    n = rng.standard_normal
    return dict(x=n((B, D)).astype(F32), x0=n((B, D)).astype(F32), w=(n((NL, D)) / np.sqrt(D)).astype(F32), b=(n((NL, D)) * 0.1).astype(F32),
                g=n((B, D)).astype(F32))


def bounds(x, w, b, g=None, x0=None, n_dot=None):
    """(float64 results, bounds on |kernel - float64|), both keyed like dcn().  Roundings, counted in dcn_v1_fwd_kernel / dcn_v1_bwd_kernel
    (a fused multiply-add only removes some):
      s_l = x_l . w_l      n_dot = dot_roundings(): R V + 6 (R V + 5 with two rows per wavefront), relative to sum |x_l| |w_l|;
      x_{l+1}              3: the product z s, + b, + x_l -- each of the three terms passes at most 3;
      gs = g . z           n_dot;
      g <- g + gs w_l      2: the product, the add;
      gx0                  NL: a term's product, then at most NL - 1 adds that can round (the first lands on 0.f);  g + gx0: 1 more;
      g_w[l], g_b[l]       a sum over the batch in an order nobody fixes (registers, slabs, atomics or the block-order launch): a term passes
                           at most B - 1 adds of two non-empty partial sums (adds of 0.f are exact), plus g_w's product: gamma(B) and
                           gamma(B - 1) times the sum of |terms|, plus the error the terms carry.
    The carried error goes through the recurrences below, per row.  A row's error keeps the shape the arithmetic gives it, so that it is not
    multiplied by sum |z| |w| (tens of times |z . w| on wide rows) at every layer:
      x^_l - x_l = alpha z + r,  |alpha| <= a (one number per row), |r| <= rho elementwise: the update adds z (s^ - s) to it, so
          |s^_l - s_l| <= a |z . w_l| + sum rho |w_l| + gamma(n_dot) sum (|x_l| + e) |w_l| =: ds,   a <- a + ds,   rho <- rho + gamma(3) (...);
      g^ - g = sum_m beta_m w_m + q over the layers m already walked, |beta_m| <= bm_m per row, |q| <= qq elementwise: the update adds
          (gs^ - gs) w_l, so |gs^ - gs| <= sum_m bm_m |w_m . z| + sum qq |z| + gamma(n_dot) sum (|g| + h) |z| =: dgs,   bm_l = dgs,   qq <- qq + gamma(2) (...).
    e = a |z| + rho and h = sum_m bm_m |w_m| + qq are the elementwise bounds.  The backward recomputes x_l and s_l with the forward's arithmetic,
    so it carries the forward's e and ds."""
    f = np.float64
    x, w, b = np.asarray(x, f), np.asarray(w, f), np.asarray(b, f)
    sep = x0 is not None
    z = np.asarray(x0, f) if sep else x
    az = np.abs(z)
    NL, (B, D) = w.shape[0], x.shape
    ref = dcn(x, w, b, g, x0)
    gd = gamma(n_dot)
    a, rho = np.zeros((B, 1)), np.zeros_like(x)
    xs, es, ss, dss = [x], [np.zeros_like(x)], [], []
    for l in range(NL):
        xl, e, aw = xs[-1], es[-1], np.abs(w[l])
        s = (xl * w[l]).sum(1, keepdims=True)
        ds = a * np.abs((z * w[l]).sum(1, keepdims=True)) + (rho * aw).sum(1, keepdims=True) + gd * ((np.abs(xl) + e) * aw).sum(1, keepdims=True)
        rho = rho + gamma(3) * (az * (np.abs(s) + ds) + np.abs(b[l]) + np.abs(xl) + e)
        a = a + ds
        es.append(a * az + rho)
        xs.append(z * s + b[l] + xl)
        ss.append(s)
        dss.append(ds)
    bnd = dict(out=es[-1])
    if g is None:
        return ref, bnd
    g = np.asarray(g, f)
    h, qq, betas = np.zeros_like(g), np.zeros_like(g), []
    k_err, k_abs = np.zeros_like(g), np.zeros_like(g)
    bw, bb = np.zeros((NL, D)), np.zeros((NL, D))
    for l in reversed(range(NL)):
        ag, aw, axl, e, s, ds = np.abs(g), np.abs(w[l]), np.abs(xs[l]), es[l], np.abs(ss[l]), dss[l]
        gs = (g * z).sum(1, keepdims=True)
        dgs = sum((bm * np.abs((w[m] * z).sum(1, keepdims=True)) for m, bm in betas), np.zeros((B, 1))) + (qq * az).sum(1, keepdims=True) \
            + gd * ((ag + h) * az).sum(1, keepdims=True)
        bb[l] = h.sum(0) + gamma(B - 1) * (ag + h).sum(0)
        bw[l] = (dgs * (axl + e) + np.abs(gs) * e).sum(0) + gamma(B) * ((np.abs(gs) + dgs) * (axl + e)).sum(0)
        k_err = k_err + h * (s + ds) + ag * ds
        k_abs = k_abs + (ag + h) * (s + ds)
        qq = qq + gamma(2) * (ag + h + (np.abs(gs) + dgs) * aw)
        betas.append((l, dgs))
        h = sum((bm * np.abs(w[m]) for m, bm in betas), np.zeros_like(g)) + qq
        g = g + gs * w[l]
    k = k_err + gamma(NL) * k_abs
    bnd.update(g_x=h if sep else h + k + gamma(1) * (np.abs(g) + h + k_abs), g_x0=k if sep else None, g_w=bw, g_b=bb)
    return ref, bnd


# ------------------------------------------------------------------------------------------------- case lists
# (D, NL, vec, density).  vec: every pointer 16-byte aligned and every leading dimension a multiple of 4 (else the scalar form, V = 1).  The
# widths sit at each side of every switch of the dispatch; the layer counts go round 0, 1, 2, 3, 4, 5, 8 so that every body meets every R it
# can.  density: the densest of 1, 0.5, 0.25, 0.1, 0.05, 0.02 for which int_exact_margin stays below 2^24 at every batch of the case, with and
# without a separate x0 (tests/test_dcn_v1_ref.py runs the checker).
INT_CASES = [
    (4, 1, True, 1.0), (4, 0, True, 1.0), (124, 2, True, 1.0), (128, 3, True, 1.0), (128, 4, True, 1.0), (128, 5, True, 1.0), (128, 8, True, 0.25),
    (132, 1, True, 1.0), (132, 3, True, 1.0), (256, 2, True, 1.0), (256, 5, True, 0.5), (260, 4, True, 1.0), (512, 3, True, 1.0),
    (512, 4, True, 0.5), (516, 2, True, 1.0), (1024, 8, True, 0.1), (1028, 1, True, 1.0), (1028, 5, True, 0.25), (2048, 1, True, 1.0),
    (2048, 4, True, 0.25), (2048, 0, True, 1.0),
    (1, 1, False, 1.0), (1, 5, False, 1.0), (3, 2, False, 1.0), (63, 3, False, 1.0), (63, 8, False, 0.5), (65, 4, False, 1.0), (65, 0, False, 1.0),
    (127, 2, False, 1.0), (129, 1, False, 1.0), (255, 3, False, 1.0), (257, 5, False, 0.5), (513, 2, False, 1.0), (1001, 8, False, 0.1),
    (1025, 1, False, 1.0), (2047, 4, False, 0.25), (2047, 2, False, 1.0), (2047, 1, False, 1.0),
]
# three trips of the row loop and a ragged end (2 pass + rpb + 3 rows), one per body and rows-per-wavefront; narrow rows.  (344 x 8 is the
# narrowest stack whose slabs leave 128 KB: the atomic body.)
PIPE_CASES = [
    (12, 1, True, 1.0), (12, 2, True, 1.0), (20, 3, True, 1.0), (128, 4, True, 0.5), (16, 5, True, 1.0),           # two rows per wavefront
    (132, 1, True, 1.0), (5, 4, False, 1.0), (132, 5, True, 0.5), (3, 2, False, 1.0), (344, 8, True, 0.1),         # one row per wavefront
]
# the forward's own three trips (its passes are twice as long): two rows per wavefront, one, scalar
FWD_PIPE_CASES = [(12, 2, True, 1.0), (132, 1, True, 1.0), (3, 2, False, 1.0)]
# D % 4 == 0 rows sent down the scalar path by a leading dimension padded by 3 or a pointer one float on: scalar R = 2, 8, 16, 32
LAYOUT_CASES = [(112, 3, 1.0), (320, 2, 1.0), (1000, 1, 1.0), (2044, 2, 1.0)]
# real-valued inputs: one shape per body and rows-per-wavefront, plus the production shapes 112 x 3, 320 x 2, 640 x 3.  B = 101 = 3 x 32 + 5
REAL_CASES = [(112, 3, True), (320, 2, True), (640, 3, True), (128, 1, True), (64, 6, True), (37, 3, False), (255, 2, False), (344, 8, True),
              (2047, 4, False), (512, 4, True)]
REAL_BATCH = 101
# the block-order sum of dcn_v1_reduce_kernel: a stride of 32 blocks and a tail of 16 -- blocks at each side of 16, 32 and 48, one block, all 256
REDUCE_D, REDUCE_NL, REDUCE_DENSITY = 320, 1, 1.0
REDUCE_BLOCKS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 256]
# n_layers x D outputs of the reduce launch: 4 (one partial 64-thread group), 222 (the g_w / g_b boundary inside a group), 2728 = 2 x 1364, the
# most the ordered mode takes (it refuses every stack of the atomic body: n_layers Dp > 2730 -- 8192 outputs are beyond it, see LIMITS)
REDUCE_SHAPES = [(4, 1, 1.0), (111, 2, 1.0), (1364, 2, 1.0)]
# the largest stacks each entry point takes, the smallest it refuses: (D, NL, vec)
FWD_LARGEST = [(1024, 8, True), (2048, 4, True)]
BWD_LARGEST = [(1000, 8, True), (2048, 4, True), (512, 4, True), (512, 3, True)]
LARGEST_DENSITY = {(1024, 8): 0.1, (2048, 4): 0.25, (1000, 8): 0.1, (512, 4): 0.5, (512, 3): 1.0}
FWD_REFUSED = [(1028, 8), (2049, 1), (16, 9)]
BWD_REFUSED = [(2048, 5), (2049, 1), (16, 9)]

# the fused gather + cross: (dims, NL).  All 28 grouped instantiations come from GROUPED_N x GROUPED_D0 x index width; the general kernel gets
# mixed feature widths at each side of its R = 1 / 2 / 4 / 8 switches
GROUPED_N, GROUPED_D0 = range(2, 9), (32, 64)
GENERAL_CASES = [([16], 2), ([128, 64, 32, 16, 16], 3), ([128, 128, 4], 2), ([256, 128, 64, 64], 4), ([256, 256, 4], 1), ([512, 256, 128, 64, 64], 8),
                 ([1024, 4], 3), ([1024, 512, 256, 256], 4)]
GENERAL_DENSITY = [1.0, 1.0, 1.0, 0.5, 1.0, 0.1, 1.0, 0.5]
GROUPED_DENSITY = {(64, 7): 0.5}                                     # every other (D0, N): 1.0
GROUPED_WRAPS = [(64, 32, 65536 + 21), (32, 64, 131072 + 37)]          # (D0, index bits, batch), N = 2: a second tile for some blocks
GENERAL_WRAP = ([16], 2, 65536 + 9)


def grouped_layers(N):
    return N % 4 + 1


def fused_inputs(dims, NL, B, density, bad=None):
    """Integer tables of 40 + 3 k rows, ids, w, b, and the concat x the gather must produce.  bad = (feature, sample, id): an id outside the
    table, which the kernels report and replace by row 0."""
    rng = np.random.default_rng([32, len(dims), dims[0], NL, B])

    def draw(*shape):
        return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < density)

    W = sum(dims)
    tables = [draw(40 + 3 * k, d) for k, d in enumerate(dims)]
    ids = [rng.integers(0, t.shape[0], B) for t in tables]
    look = [i.copy() for i in ids]
    if bad is not None:
        ids[bad[0]][bad[1]], look[bad[0]][bad[1]] = bad[2], 0
    w, b = draw(NL, W), draw(NL, W)
    w[:, -1] = rng.integers(0, 2, NL) * 2 - 1
    x = np.concatenate([t[i] for t, i in zip(tables, look)], axis=1)
    return dict(tables=tables, ids=ids, w=w, b=b, x=x)


def grouped_batches(D0):
    tb = fused_form([D0, D0])["TB"]
    return [tb - 1, tb, tb + 1, 3 * tb + 5]


def general_batches(dims):
    """Around the S-sample tail of a wavefront and of a block of four."""
    s = fused_form(dims)["S"]
    return sorted({1, s - 1, s, s + 1, 4 * s - 1, 4 * s, 4 * s + 1, 12 * s + 5} - {0})


def fwd_pipe_batch(D, NL, vec):
    f = fwd_form(D, NL, vec)
    return 2 * f["pass_rows"] + f["rpb"] + 3


def pipe_batch(D, NL, vec, sep):
    f = bwd_form(D, NL, vec, sep)
    return 2 * f["pass_rows"] + f["rpb"] + 3
