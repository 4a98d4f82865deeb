"""Seeded segments for the per-user ranking metrics (nrx_user_rank_metrics / csrc/nrx_rank_metrics.h) and their reference: one user at a time through
oracle.ref_np.user_rank_metrics.  A segment is one user's (scores, labels) float32 arrays ALREADY in ranked order; the named edge segments go
to the host program first (tests/test_rank_metrics_host.py) and to the device afterwards (tests/test_rank_metrics_gpu.py), the same arrays."""
from collections import namedtuple

import numpy as np

from oracle import ref_np as R

SEED = 20240611
Segment = namedtuple("Segment", "name scores labels k")
NAN, INF = float("nan"), float("inf")
F32 = np.float32


def _seg(name, scores, labels, k):
    return Segment(name, np.asarray(scores, F32), np.asarray(labels, F32), k)


def edge_segments():
    """Non-finite scores wherever they can sit, signed zeros, and the smallest segments; finite ones are in descending order."""
    return [
        _seg("nan-first", [NAN, 0.5, 0.5, 0.3], [1, 0, 1, 0], 10),
        _seg("nan-middle", [0.9, 0.5, NAN, 0.5, 0.1], [0, 1, 1, 0, 1], 10),
        _seg("nan-last", [0.9, 0.5, 0.1, NAN], [0, 1, 0, 1], 10),
        _seg("all-nan", [NAN, NAN, NAN, NAN, NAN], [0, 1, 0, 1, 1], 10),
        _seg("one-nan", [NAN], [1], 10),
        _seg("nan-pair-then-numbers-k-cuts-inside", [NAN, NAN, 0.7, 0.7, 0.2], [0, 0, 1, 0, 1], 3),
        _seg("plus-inf", [INF, 0.5, 0.2], [1, 0, 1], 10),
        _seg("minus-inf", [0.5, 0.2, -INF], [0, 1, 1], 10),
        _seg("both-inf-tied", [INF, INF, 0.0, -INF, -INF], [1, 0, 1, 0, 1], 10),
        _seg("nan-and-inf", [NAN, INF, 0.3, -INF], [0, 1, 0, 1], 10),
        _seg("neg-zero-against-zero", [0.5, 0.0, -0.0, 0.0, -0.0, -0.3], [0, 1, 0, 1, 0, 1], 10),
        _seg("empty", [], [], 10),
        _seg("one-entry-positive", [0.4], [1], 10),
        _seg("one-entry-negative", [0.4], [0], 10),
        _seg("all-one-class-positive", [0.9, 0.9, 0.4, 0.1], [1, 1, 1, 1], 10),
        _seg("all-one-class-negative", [0.9, 0.9, 0.4, 0.1], [0, 0, 0, 0], 10),
        _seg("k-larger-than-segment", [0.9, 0.8, 0.8, 0.2, 0.1], [0, 1, 0, 0, 1], 50),
        _seg("k-smaller-than-segment", [0.9, 0.8, 0.8, 0.7, 0.2, 0.1, 0.1], [0, 0, 1, 1, 0, 1, 0], 2),
        _seg("k-1-positive-below-the-cut", [0.9, 0.8, 0.1], [0, 1, 1], 1),
        _seg("more-positives-than-k", [0.9, 0.8, 0.8, 0.7, 0.2, 0.1], [1, 1, 0, 1, 1, 1], 3),
        _seg("all-tied", [0.5] * 6, [1, 0, 0, 1, 0, 1], 10),
    ]


def random_segments(k, n=400, seed=SEED):
    """Lengths 1..40, scores rounded to one decimal (heavy ties), descending with arrival order among ties; every tenth user has no positive,
    only positives, or more positives than k (where the length allows)."""
    rng = np.random.default_rng([seed, k])
    out = []
    for u in range(n):
        length = int(rng.integers(1, 41))
        scores = np.sort(np.round(rng.random(length), 1).astype(F32))[::-1].copy()
        labels = (rng.random(length) < rng.choice([0.1, 0.4, 0.8])).astype(F32)
        kind = "random"
        if u % 10 == 3:
            labels[:], kind = 0, "no-positive"
        elif u % 10 == 6:
            labels[:], kind = 1, "only-positives"
        elif u % 10 == 9:
            labels[rng.permutation(length)[: k + 1 + int(rng.integers(0, 3))]] = 1
            kind = "more-positives-than-k" if labels.sum() > k else "random"
        out.append(Segment(f"{kind}-{u}", scores, labels, k))
    return out


def palette():
    """64 distinct segments of length 1..3 for the grid-cap case: every label pattern over tied and untied scores."""
    out = []
    shapes = [([0.5], 1), ([0.7, 0.2], 2), ([0.4, 0.4], 2), ([0.9, 0.5, 0.1], 3), ([0.6, 0.6, 0.1], 3), ([0.6, 0.1, 0.1], 3), ([0.3, 0.3, 0.3], 3),
              ([0.8, -0.0, 0.0], 3), ([NAN, 0.5, 0.2], 3), ([0.25, 0.125], 2), ([1.0, 0.0, -1.0], 3)]
    for scores, length in shapes:
        for bits in range(1 << length):
            out.append(_seg(f"p{len(out)}", scores, [(bits >> i) & 1 for i in range(length)], 10))
    assert len(out) >= 64
    out = out[:64]
    assert len({(s.scores.tobytes(), s.labels.tobytes()) for s in out}) == 64
    return out


def pack(segments):
    """(scores, labels, seg_start) of the segments laid end to end."""
    scores = np.concatenate([s.scores for s in segments] + [np.zeros(0, F32)]).astype(F32)
    labels = np.concatenate([s.labels for s in segments] + [np.zeros(0, F32)]).astype(F32)
    seg = np.concatenate([[0], np.cumsum([len(s.scores) for s in segments])]).astype(np.int64)
    return scores, labels, seg


def reference(segments, k=None):
    """float64 [n, 4] (auc, ndcg, hr, mrr): a plain loop, one user at a time."""
    out = np.empty((len(segments), 4), np.float64)
    for i, s in enumerate(segments):
        out[i] = R.user_rank_metrics(s.scores, s.labels, s.k if k is None else k)
    return out


def assert_matches(got, want, names):
    """The bars: NaN in the same places; AUC, HR, MRR bit-equal (sums of integers and halves far below 2^53, then one correctly rounded float64
    division); NDCG within 1e-12 absolute (at most k <= 50 terms in [0, 1], each off by a few ulp of log2)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn).any(axis=1))
    assert bad.size == 0, ("NaN positions", names[bad[0]], got[bad[0]], want[bad[0]])
    assert not wn[:, 1:].any()
    for col, what in ((0, "auc"), (2, "hr"), (3, "mrr")):
        ok = wn[:, col] | (got[:, col].view(np.int64) == want[:, col].view(np.int64))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (what, names[bad[0]], got[bad[0]], want[bad[0]])
    bad = np.flatnonzero(~(np.abs(got[:, 1] - want[:, 1]) <= 1e-12))
    assert bad.size == 0, ("ndcg", names[bad[0]], got[bad[0]], want[bad[0]])
    fin = got[:, 1:]
    assert np.isfinite(fin).all() and (fin >= 0).all() and (fin <= 1).all()
