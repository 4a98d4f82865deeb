"""Case lists for the batch-split weight-gradient kernels of csrc/nrx_dcn2_bwd.hip (dcn2_gemm_kernel<WGRAD>, dcn2_gemm_split_kernel<WGRAD>,
wgrad_reduce_kernel; driven by launch_wgrad / wgrad_shape), with operands for which every summation order gives the same bits.

Operands are integers in [-4, 4] stored as float32.  Every product and every partial sum of such operands is an integer below 2^24, hence exact in
fp32 (and the operands are exact in bf16 with a zero low part, so the bf16x3 form computes the same integers): float atomics, ordered slices and the
MFMA chains must all give the int64 result word for word.  The bounds that make this true are asserted below, at import, for every case.

No GPU and no torch here: tests/test_wgrad_cases.py checks this module on the CPU, tests/test_wgrad_exact_gpu.py runs the cases."""
from dataclasses import dataclass

import numpy as np

SEED = 20240611
EXACT = 1 << 24            # integers of magnitude <= 2^24 are exact in fp32; the asserts below keep every sum strictly under it
VMAX = 4                   # operands are integers in [-VMAX, VMAX]
BF16_EXACT = 256           # integers of magnitude <= 256 are exact in bf16 (8 significant bits)


def _cdiv(a, b):
    return -(-a // b)


def wgrad_shape(M, N, batch):
    """wgrad_shape() of nrx_dcn2_bwd.hip at its defaults (NRX_WGRAD_XCD = 1, no tuning variables): (small, nt, splits, kslice) -- the 64 x 64 block
    tile or the 128 x 64 one, the tiles of g_W, the batch slices and the rows of one slice.  batch >= 1."""
    small = M <= 384
    bm = 64 if small else 128
    nt = _cdiv(N, 64) * _cdiv(M, bm)
    want = 1536 if small else 1024
    kmin = 32 * (16 if small and nt > 1 else 8)
    per_round = max(128 // nt, 1)
    rounds = max((want + 4 * per_round * nt) // (8 * per_round * nt), 1)
    splits = 8 * per_round * rounds
    kslice = max(_cdiv(_cdiv(batch, splits), 32) * 32, kmin)
    splits = _cdiv(batch, kslice)
    return small, nt, splits, kslice


def linear_workspace_bytes(batch, M, N):
    """What nrx_linear_wgrad_ordered_workspace(batch, M, N) returns if the library's wgrad_shape is the one above."""
    if batch < 0 or M < 1 or N < 1:
        return -1
    if batch == 0:
        return 256
    return wgrad_shape(M, N, batch)[2] * (M * N + M) * 4 + 512


def dcn2_workspace_bytes(batch, dim):
    """The same for nrx_dcn_v2_layer_bwd_workspace(batch, dim): glin + the ReLU mask bits + the ordered wgrad's partial tiles."""
    if batch < 0 or dim < 1:
        return -1
    ld = (dim + 3) & ~3
    part = wgrad_shape(dim, dim, batch)[2] * (dim * dim + dim) * 4 + 256 if batch > 0 else 0
    return (batch + _cdiv(batch, 32)) * ld * 4 + 512 + part + 256


def _slice_key(M, N, batch):
    small, nt, splits, kslice = wgrad_shape(M, N, batch)
    last = batch - (splits - 1) * kslice
    return dict(tile=64 if small else 128, tiles=nt, slices=splits, kslice=kslice, partial_slab=batch % 32 != 0, short_last=last < 32,
                ragged=M % 64 != 0 or N % 64 != 0)


# ---- nrx_linear_wgrad / nrx_linear_wgrad_ordered ----------------------------------------------------------------------------------------------------
PATHS = ("vec", "scalar-by-width", "scalar-by-ld", "scalar-by-pointer")
MODES = ("atomic", "ordered")


@dataclass(frozen=True)
class LinearCase:
    """One C-level call: g [batch, M] with leading dimension g_ld, a [batch, N] with a_ld; the base pointers sit g_off / a_off floats into
    16-byte-aligned allocations."""
    index: int
    M: int
    N: int
    batch: int
    g_ld: int
    a_ld: int
    g_off: int
    a_off: int
    bias: bool
    mode: str

    @property
    def path(self):
        """Which loads the kernel takes, and why: the entry points take the float4 path only if widths, leading dimensions and pointers all allow it."""
        if self.M % 4 or self.N % 4:
            return "scalar-by-width"
        if self.g_ld % 4 or self.a_ld % 4:
            return "scalar-by-ld"
        if self.g_off % 4 or self.a_off % 4:
            return "scalar-by-pointer"
        return "vec"

    @property
    def key(self):
        return dict(_slice_key(self.M, self.N, self.batch), path=self.path, mode=self.mode, bias=self.bias)

    @property
    def name(self):
        return (f"lin{self.index}-{self.M}x{self.N}-b{self.batch}-{self.mode}-{'bias' if self.bias else 'nobias'}-{self.path}"
                f"-ld{self.g_ld}.{self.a_ld}-off{self.g_off}.{self.a_off}")


# (M, N, batch): the smallest shapes that reach each form
_LINEAR_SHAPES = (
    [(8, 8, b) for b in (255, 256, 257, 4096, 4097, 8192, 8193, 12545)]       # one tile, kslice 256: 1, 1, 2, 16, 17, 32, 33, 50 slices
    + [(64, 72, 1025), (68, 8, 513)]                                          # several tiles: slices of at least 512 rows
    + [(384, 8, 600), (388, 8, 600)]                                          # either side of the tile switch
    + [(388, 68, 2000)]                                                       # the 128 x 64 tile, two column tiles, 8 slices
    + [(19, 37, 777), (1, 64, 1000), (390, 10, 333)]                          # odd widths, the last one on the 128 x 64 tile
    + [(64, 128, 300)]                                                        # whole tiles only
    + [(m, n, b) for (m, n) in ((4, 12), (12, 4)) for b in (1, 7, 31, 33)]    # a slice shorter than one slab of 32 rows
)
_LINEAR_LARGE = (16, 16, 300000)                                               # 1 172 slices; once per mode
# aligned shapes that are also run with a leading dimension and with a base pointer that force the scalar loads
_LINEAR_LAYOUT_SHAPES = [(8, 8, 257), (8, 8, 4097), (64, 72, 1025), (388, 8, 600), (388, 68, 2000), (4, 12, 7), (12, 4, 33)]
_PADS_ALIGNED = ((4, 8), (0, 4), (8, 0), (0, 0))
_PADS_ODD = ((1, 2), (0, 3), (5, 0), (0, 0))


def linear_cases():
    """The fixed list of C-level calls (deterministic: no randomness in the list itself, the operands are seeded by the case index)."""
    cases = []

    def add(M, N, batch, pg, pa, g_off, a_off, bias, mode):
        cases.append(LinearCase(len(cases), M, N, batch, M + pg, N + pa, g_off, a_off, bias, mode))

    for si, (M, N, batch) in enumerate(_LINEAR_SHAPES):
        aligned = M % 4 == 0 and N % 4 == 0
        for vi, (mode, bias) in enumerate((m, b) for m in MODES for b in (True, False)):
            pg, pa = (_PADS_ALIGNED if aligned else _PADS_ODD)[(si + vi) % 4]
            off = 4 * ((si + vi) % 2)              # (a multiple of 4 floats keeps the pointer 16-byte aligned)
            add(M, N, batch, pg, pa, off, 4 - off, bias, mode)
    for si, (M, N, batch) in enumerate(_LINEAR_LAYOUT_SHAPES):
        for vi, (mode, bias) in enumerate((m, b) for m in MODES for b in (True, False)):
            k = si + vi
            pg, pa = ((3, 4), (4, 1), (1, 1), (0, 2))[k % 4]                    # a leading dimension that is no multiple of 4
            add(M, N, batch, pg, pa, 0, 4 * (k % 2), bias, mode)
            g_off, a_off = ((1, 0), (0, 3), (2, 2), (4, 1))[k % 4]              # a base pointer that is not 16-byte aligned
            pg, pa = _PADS_ALIGNED[k % 4]
            add(M, N, batch, pg, pa, g_off, a_off, bias, mode)
    for mode in MODES:
        add(*_LINEAR_LARGE, 4, 0, 0, 4, True, mode)
    return cases


# ---- nrx_dcn_v2_layer_bwd -----------------------------------------------------------------------------------------------------------------------------
ACCS = (0, 1, 3)
PADS = (0, 4, 7)
_DCN2_COMMON_BATCHES = (1, 7, 8, 63, 64, 65)          # 7 / 8: the `batch >= 8` condition of the split form
_DCN2_DIMS = (
    (8, (257, 4097)),         # panel form; one tile, kslice 256: 2 and 17 slices
    (112, (513, 1025)),       # panel form at its widest; four tiles, kslice 512: 2 and 3 slices
    (116, (513,)),            # float4 loads, three launches, ordered whatever bit 2 says (dim <= 128)
    (37, (257,)),             # scalar loads
    (132, (513, 1025)),       # 64 x 64 tile, float atomics by default: 2 and 3 slices
    (388, (257,)),            # 128 x 64 tile: 2 slices
)


@dataclass(frozen=True)
class Dcn2Case:
    """One nrx_dcn_v2_layer_bwd call.  Leading dimensions as tests/stress_dcn2_bwd.py: x0 / xl / lin / out and g_x0 dim + pad, g_out dim + 2 pad,
    g_xl dim + 3 pad."""
    index: int
    dim: int
    batch: int
    flags: int             # bit 0 ReLU, bit 1 split-bf16 matrix math, bit 2 ordered weight gradient
    acc: int               # accumulate_x0
    pad: int

    @property
    def ld(self):
        return self.dim + self.pad

    @property
    def g_ld(self):
        return self.dim + 2 * self.pad

    @property
    def gxl_ld(self):
        return self.dim + 3 * self.pad

    @property
    def key(self):
        """The forms the call takes at the library's defaults (NRX_DCN2_PANEL, NRX_DCN2_NARROW_ORDERED and NRX_WGRAD_XCD unset)."""
        vec = self.dim % 4 == 0 and self.pad % 4 == 0
        split = bool(self.flags & 2)
        panel = vec and not split and 8 <= self.dim <= 112
        ordered = bool(self.flags & 4) or self.dim <= 128
        split_gemm = vec and split and self.batch >= 8
        return dict(_slice_key(self.dim, self.dim, self.batch), path="vec" if vec else "scalar", relu=bool(self.flags & 1), split_bit=split,
                    ordered_bit=bool(self.flags & 4), form="panel" if panel else "three-launch",
                    dgrad="panel" if panel else "split" if split_gemm else "fp32",
                    wgrad="ordered" if ordered else "split-atomic" if split_gemm else "atomic")

    @property
    def name(self):
        return f"dcn{self.index}-d{self.dim}-b{self.batch}-f{self.flags}-acc{self.acc}-pad{self.pad}"


def dcn2_cases():
    """Every flag value at every (dim, batch); accumulate_x0 and the pad walk their values at different rates, so every pair of them appears."""
    cases = []
    for dim, edges in _DCN2_DIMS:
        for bi, batch in enumerate(_DCN2_COMMON_BATCHES + edges):
            for flags in range(8):
                i = len(cases)
                # (the two flag values of a math mode get neighbouring pads: at every batch one of them keeps the float4 path)
                cases.append(Dcn2Case(i, dim, batch, flags, ACCS[i % 3], PADS[(flags + (flags >> 1) + bi) % 3]))
    return cases


# ---- operands and the exact reference -------------------------------------------------------------------------------------------------------------------
def case_rng(case):
    """The generator of a case's operands: seeded by the case alone."""
    return np.random.default_rng([SEED, 0 if isinstance(case, LinearCase) else 1, case.index])


def _ints(rng, *shape):
    return rng.integers(-VMAX, VMAX + 1, size=shape).astype(np.float32)


def _no_zeros(x, rows, rng):
    """Rows next to a slice boundary get no zero entry: dropping or doubling such a row always changes the sums."""
    for r in rows:
        z = x[r] == 0
        x[r][z] = rng.choice(np.array([-1.0, 1.0], np.float32), size=int(z.sum()))


def _boundary_rows(M, N, batch):
    _, _, splits, kslice = wgrad_shape(M, N, batch)
    rows = {0, batch - 1}
    for s in range(1, splits):
        rows.update((s * kslice - 1, s * kslice))
    return sorted(rows)


def int_operands(case, rng):
    """float32 arrays holding integers in [-4, 4].  Linear: g [batch, M], a [batch, N].  DCN-v2: x0, xl, lin, g, gx0 [batch, dim], W [dim, dim] and
    `out`, the forward output whose sign is the ReLU mask: negatives, +0.0, -0.0 (both masked: the mask is out > 0) and positives, tiny ones among
    them; unevenly mixed, one column all on and, beyond one row, one row all off."""
    if isinstance(case, LinearCase):
        g, a = _ints(rng, case.batch, case.M), _ints(rng, case.batch, case.N)
        rows = _boundary_rows(case.M, case.N, case.batch)
        _no_zeros(g, rows, rng)
        _no_zeros(a, rows, rng)
        return dict(g=g, a=a)
    B, D = case.batch, case.dim
    ops = {k: _ints(rng, B, D) for k in ("x0", "xl", "lin", "g", "gx0")}
    ops["W"] = _ints(rng, D, D)
    out = rng.choice(np.array([-2.5, -0.0, 0.0, 1e-30, 3.0], np.float32), size=(B, D), p=[0.25, 0.2, 0.2, 0.15, 0.2])          # 35 % on
    out[:, 1 % D] = 0.5
    if B > 1:
        out[B // 2, :] = -1.0
    ops["out"] = out
    return ops


def exact_reference(case, operands):
    """int64 numpy of the definitions in the header comment of nrx_dcn2_bwd.hip.  Linear: g_W = g^T a, g_b = column sums of g.  DCN-v2:
    gm = g (x) [out > 0] (ReLU) or g;  glin = gm x0;  g_x0 = gm lin (+ its old value: acc bit 0);  g_xl = gm + glin W (+ g_x0: acc bit 1);
    g_W = glin^T xl;  g_b = column sums of glin.  Every entry is checked against the bound that makes fp32 exact."""
    i64 = lambda x: x.astype(np.int64)
    if isinstance(case, LinearCase):
        g, a = i64(operands["g"]), i64(operands["a"])
        ref = dict(g_W=np.einsum("bi,bj->ij", g, a), g_b=g.sum(0))
    else:
        x0, xl, lin, g, gx0, W = (i64(operands[k]) for k in ("x0", "xl", "lin", "g", "gx0", "W"))
        gm = g * (operands["out"] > 0) if case.flags & 1 else g
        glin = gm * x0
        g_x0 = gm * lin + (gx0 if case.acc & 1 else 0)
        g_xl = gm + glin @ W + (g_x0 if case.acc & 2 else 0)
        ref = dict(g_xl=g_xl, g_x0=g_x0, g_W=np.einsum("bi,bj->ij", glin, xl), g_b=glin.sum(0))
    bound = reference_bound(case)
    for k, v in ref.items():
        assert v.dtype == np.int64 and np.abs(v).max(initial=0) <= bound[k] < EXACT, (case.name, k)
    return ref


def reference_bound(case):
    """Bounds on the magnitude of every output entry AND of every partial sum on the way to it (a partial sum of the same products is bounded by the
    same count of terms), derived from the operand range alone."""
    v = VMAX
    if isinstance(case, LinearCase):
        return dict(g_W=v * v * case.batch, g_b=v * case.batch)          # 16 * batch bounds both
    B, D = case.batch, case.dim
    glin = v * v                                    # |gm x0|
    g_x0 = v * v + v                                # |gm lin + old|
    return dict(glin=glin, g_x0=g_x0, g_xl=v + glin * v * D + g_x0, g_W=glin * v * B, g_b=glin * B)


def _assert_exact_by_construction():
    for c in linear_cases():
        assert 16 * c.batch < EXACT and all(b < EXACT for b in reference_bound(c).values()), c.name
    for c in dcn2_cases():
        b = reference_bound(c)
        assert all(x < EXACT for x in b.values()), c.name
        assert b["glin"] <= BF16_EXACT and VMAX <= BF16_EXACT, c.name          # the MFMA operands of the bf16x3 form: exact in bf16, low part zero


_assert_exact_by_construction()
