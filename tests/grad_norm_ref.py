"""numpy + Python-int restatement of the row-sparse gradient norm (nrx_rows_sqnorm / nrx_rows_sqnorm_finish, include/nrx_embed.h): float64 lane sums
and tree, one cast to float32 per row, integer bins, the ascending finish with math.ldexp.  No GPU, no torch.  Bit-exact by construction: numpy's
float64 arithmetic and its float64 -> float32 cast are the device's roundings (round to nearest even, denormals kept)."""
import math

import numpy as np

BIG = np.iinfo(np.int64).max
ROW_MASK = (1 << 40) - 1
N_BINS = 258


def lanes_for(dim):
    """Q: the smallest power of two with 4 Q >= dim, at most 64."""
    q = 1
    while 4 * q < dim and q < 64:
        q *= 2
    return q


def is_live(k, n_tables, skip_tables=0):
    k = int(k)
    t, r = k >> 40, k & ROW_MASK
    return k >= 0 and k != BIG and t < n_tables and r != 0 and not (skip_tables >> t) & 1


def row_sums(g):
    """The double S of every row of g [n, dim] (vectorised over the rows; the order inside a row is the definition's): chunk j of four columns belongs
    to lane j % Q, a lane adds its squares in ascending column order from 0.0, the lanes are combined by x[l] = x[l] + x[l ^ s], s = 1, 2, 4, ..."""
    g = np.asarray(g, dtype=np.float32)
    n, dim = g.shape
    q = lanes_for(dim)
    x = np.zeros((n, q), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(dim):
            d = g[:, k].astype(np.float64)
            x[:, (k // 4) % q] = x[:, (k // 4) % q] + d * d
        s = 1
        while s < q:
            x = x + x[:, np.arange(q) ^ s]
            s *= 2
    return x[:, 0]


def row_sum(g):
    return row_sums(np.asarray(g, dtype=np.float32)[None])[0]


def row_words(g):
    """(bin, amount) int64 arrays for the rows of g [n, dim]: the float32 of each sum, split into exponent and significand."""
    with np.errstate(all="ignore"):
        s32 = row_sums(g).astype(np.float32)
    b = (s32.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    e, m = b >> 23, b & 0x7FFFFF
    bins = np.where(e == 0, 1, np.where(e <= 254, e, np.where(m == 0, 256, 257)))
    amount = np.where(e == 0, m, np.where(e <= 254, m | 0x800000, 1))
    return bins, amount


def row_word(g):
    b, a = row_words(np.asarray(g, dtype=np.float32)[None])
    return int(b[0]), int(a[0])


def bins_of(keys, grads, n_tables, n_dev=None, skip_tables=0, bins=None):
    """nrx_rows_sqnorm: the live rows of (keys [n], grads [n, dim]) added into `bins` (a list of 258 Python ints; a new one when None)."""
    bins = [0] * N_BINS if bins is None else list(bins)
    n = len(keys) if n_dev is None else min(len(keys), int(n_dev))
    live = [i for i in range(n) if is_live(keys[i], n_tables, skip_tables)]
    if live:
        b, amount = row_words(np.asarray(grads, dtype=np.float32)[live])
        for bi, ai in zip(b.tolist(), amount.tolist()):
            bins[bi] += ai
    return bins


def finish(bins, max_norm, extra_sq=None):
    """nrx_rows_sqnorm_finish: (norm as a Python float, coef as np.float32)."""
    total = 0.0
    for e in range(1, 255):
        total = total + math.ldexp(float(bins[e]), e - 150)
    if extra_sq is not None:
        total = total + float(extra_sq)
    if bins[257] > 0 or total != total:
        norm = math.nan
    elif bins[256] > 0:
        norm = math.inf
    else:
        norm = math.sqrt(total)
    c = max_norm / (norm + 1e-6)
    c = 1.0 if c > 1.0 else c
    return norm, np.float32(c)
