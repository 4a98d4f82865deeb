"""numpy restatement of the bf16 tables' stochastic rounding (include/nrx_embed.h, nrx_sparse_adam_step_bf16):

    bits16 = h >> 48,   h = mix(mix(mix(mix(mix(seed) ^ step) ^ table) ^ row) ^ col)     (mix = splitmix64's finaliser of z + golden)
    bf16   = (f32_bits(w) + bits16) >> 16     for finite w;  inf / NaN: a plain cast (a NaN stays a NaN)

Used by the CPU tests (hand-picked cases) and the GPU tests (the kernel's weights against this, bit for bit -- NaNs by NaN-ness only)."""
import numpy as np

M64 = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)


def mix(z):
    """splitmix64 step on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
    return z ^ (z >> np.uint64(31))


def sr_bits(seed: int, step: int, table: int, rows, cols):
    """The 16 random bits of every (row, col): rows [R] x cols [C] -> uint32 [R, C]."""
    h_table = mix(mix(mix(np.uint64(seed & M64)) ^ np.uint64(step & M64)) ^ np.uint64(table))
    h_row = mix(h_table ^ np.asarray(rows, dtype=np.uint64).reshape(-1, 1))
    h = mix(h_row ^ np.asarray(cols, dtype=np.uint64).reshape(1, -1))
    return (h >> np.uint64(48)).astype(np.uint32)


def sr_round(w, bits):
    """fp32 values + their 16 random bits -> bf16 bit patterns (uint16)."""
    u = np.asarray(w, dtype=np.float32).view(np.uint32)
    bits = np.asarray(bits, dtype=np.uint32)
    finite = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    with np.errstate(over="ignore"):
        sr = ((u + bits) >> np.uint32(16)).astype(np.uint16)
    # inf / NaN: a plain cast.  inf is exact; for a NaN the contract is only that it stays a NaN -- the pattern below is one such NaN,
    # not the one the hardware cast must produce: compare with `matches` (NaN-ness for NaNs, bits otherwise)
    plain = ((u >> np.uint32(16)) | np.where((u & np.uint32(0x7FFFFF)) != 0, np.uint32(0x40), np.uint32(0))).astype(np.uint16)
    return np.where(finite, sr, plain)


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def matches(got, want):
    """bf16 patterns equal, except that a NaN only has to be met by a NaN (any payload, any sign)."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    nan_g, nan_w = np.isnan(bf16_to_f32(got)), np.isnan(bf16_to_f32(want))
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got[~nan_w], want[~nan_w]))
