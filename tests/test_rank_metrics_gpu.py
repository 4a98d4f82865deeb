"""nrx_user_rank_metrics alone: the C entry point on ranked segments against the oracle one user at a time (tests/rank_metrics_cases.py), and
ranking_metrics on generated streams against R.validation_metrics.

Bars (none measured; rank_metrics_cases.assert_matches): AUC, HR, MRR bit-equal, NDCG within 1e-12 absolute, NaN in the same places.
The non-finite segments are the arrays that tests/test_rank_metrics_host.py ran through the host build of the same function first."""
import numpy as np
import pytest

from oracle import ref_np as R
from tests import rank_metrics_cases as rc

pytestmark = pytest.mark.gpu

POISON = -7.25
GUARD = 2


def launch(scores, labels, seg, n_users, k):
    """float64 [n_users, 4] from the kernel; every output array has GUARD entries behind it that must keep their poison."""
    import torch
    from news_recsys_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sc = d(scores) if len(scores) else torch.zeros(1, dtype=torch.float32, device=dev)
    lb = d(labels) if len(labels) else torch.zeros(1, dtype=torch.float32, device=dev)
    sg = d(seg)
    outs = [torch.full((n_users + GUARD,), POISON, dtype=torch.float64, device=dev) for _ in range(4)]
    _lib.check(lib.nrx_user_rank_metrics(sc.data_ptr(), lb.data_ptr(), sg.data_ptr(), n_users, k, *[o.data_ptr() for o in outs], None),
               "nrx_user_rank_metrics")
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for name, h in zip(("auc", "ndcg", "hr", "mrr"), host):
        assert (h[n_users:] == POISON).all(), f"{name}: the {GUARD} entries past the output changed"
    return np.stack([h[:n_users] for h in host], axis=1)


def run_segments(segments, k):
    scores, labels, seg = rc.pack(segments)
    return launch(scores, labels, seg, len(segments), k)


@pytest.mark.parametrize("k", [1, 10, 50])
def test_random_tied_segments_per_user(k):
    segs = rc.random_segments(k)
    kinds = {s.name.rsplit("-", 1)[0] for s in segs}
    assert {"no-positive", "only-positives"} <= kinds and (k == 50 or "more-positives-than-k" in kinds)
    rc.assert_matches(run_segments(segs, k), rc.reference(segs, k), [s.name for s in segs])


def test_no_positive_only_positives_and_more_positives_than_k():
    segs = [s for s in rc.random_segments(3, 200) if not s.name.startswith("random")]
    assert {s.name.rsplit("-", 1)[0] for s in segs} == {"no-positive", "only-positives", "more-positives-than-k"}
    got = run_segments(segs, 3)
    rc.assert_matches(got, rc.reference(segs, 3), [s.name for s in segs])
    for s, g in zip(segs, got):
        if s.name.startswith("no-positive"):
            assert np.isnan(g[0]) and (g[1:] == 0).all()
        if s.name.startswith("only-positives"):
            assert np.isnan(g[0]) and (g[1:] == 1).all()


@pytest.mark.parametrize("k", sorted({s.k for s in rc.edge_segments()}))
def test_non_finite_and_edge_segments(k):
    """NaN first / middle / last / all-NaN, +-inf, -0.0 against 0.0, empty, one entry, one class, k larger and smaller than the segment: all in
    ONE launch per k, neighbours of each other (an empty segment between two real ones included)."""
    segs = [s for s in rc.edge_segments() if s.k == k]
    got = run_segments(segs, k)
    rc.assert_matches(got, rc.reference(segs), [s.name for s in segs])
    for s, g in zip(segs, got):
        if len(s.scores) == 0 or not np.isfinite(s.scores).all():
            assert np.isnan(g[0]), s.name
        if len(s.scores) == 0:
            assert (g[1:] == 0).all()


@pytest.mark.parametrize("seg", rc.edge_segments(), ids=lambda s: s.name)
def test_edge_segment_alone(seg):
    """One segment per launch, at its own k: the arrays the host program returned on."""
    got = run_segments([seg], seg.k)
    rc.assert_matches(got, rc.reference([seg]), [seg.name])
    if len(seg.scores) == 0 or not np.isfinite(seg.scores).all():
        assert np.isnan(got[0, 0])


def test_every_edge_segment_at_every_k():
    for k in (1, 2, 10, 50):
        segs = [s._replace(k=k) for s in rc.edge_segments()]
        rc.assert_matches(run_segments(segs, k), rc.reference(segs), [s.name for s in segs])


def test_zero_users_returns_ok_with_null_pointers():
    from news_recsys_amd import _lib
    lib = _lib.load()
    assert lib.nrx_user_rank_metrics(None, None, None, 0, 10, None, None, None, None, None) == 0


def test_grid_cap_stride_loop_at_1048576_plus_300_users():
    """The launch is capped at 4096 blocks of 256: users past 1 048 576 are reached only by the stride loop.  User u = palette pattern u % 64."""
    n = 4096 * 256 + 300
    pal = rc.palette()
    ref = rc.reference(pal, 10)
    p_scores, p_labels, p_seg = rc.pack(pal)
    cycles, rest = divmod(n, 64)
    scores = np.concatenate([np.tile(p_scores, cycles), p_scores[:p_seg[rest]]])
    labels = np.concatenate([np.tile(p_labels, cycles), p_labels[:p_seg[rest]]])
    lens = np.diff(p_seg)
    seg = np.concatenate([[0], np.cumsum(np.concatenate([np.tile(lens, cycles), lens[:rest]]))]).astype(np.int64)
    assert seg.size == n + 1 and seg[-1] == scores.size == labels.size
    got = launch(scores, labels, seg, n, 10)
    rc.assert_matches(got, ref[np.arange(n) % 64], np.arange(n))


# ------------------------------------------------------------------------------------------------ through ranking_metrics
def _stream(name):
    """(user ids, scores, labels) in a shuffled arrival order; scores rounded to one decimal in [0.1, 0.9]: ties across and within users."""
    rng = np.random.default_rng([rc.SEED, sum(map(ord, name))])
    if name == "empty-epoch":
        return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32)
    n_users = 1 if name == "single-user" else 120
    counts = rng.integers(1, 41, n_users)
    uid = np.repeat(rng.permutation(10 * n_users)[:n_users] + 1, counts).astype(np.int64)
    scores = np.round(0.1 + 0.8 * rng.random(uid.size), 1).astype(np.float32)
    labels = (rng.random(uid.size) < 0.35).astype(np.float32)
    if name == "every-user-single-class":
        labels = (uid % 2).astype(np.float32)
    if name == "nan-scores":
        scores[rng.random(uid.size) < 0.02] = np.nan          # a few users hold one or more NaN, most hold none
        assert np.isnan(scores).any() and len(set(uid[np.isnan(scores)])) < n_users / 2
    order = rng.permutation(uid.size)
    return uid[order], scores[order], labels[order]


STREAMS = ["shuffled-ties", "single-user", "every-user-single-class", "empty-epoch", "nan-scores"]
WARM = ["none", "empty-list", "ids-that-never-occur", "all-ids", "half-of-the-ids"]


def _warm(kind, uid):
    users = sorted(set(uid.tolist()))
    return {"none": None, "empty-list": [], "ids-that-never-occur": [10 ** 9, 10 ** 9 + 1], "all-ids": users, "half-of-the-ids": users[::2]}[kind]


_REF = {}


def _reference(stream, warm):
    if (stream, warm) not in _REF:
        uid, sc, lb = _stream(stream)
        _REF[stream, warm] = R.validation_metrics(uid, sc, lb, _warm(warm, uid))
    return _REF[stream, warm]


@pytest.mark.parametrize("warm", WARM)
@pytest.mark.parametrize("stream", STREAMS)
def test_ranking_metrics_on_generated_streams(stream, warm):
    import torch
    from news_recsys_amd.metrics import format_val_log, ranking_metrics
    uid, sc, lb = _stream(stream)
    ref = _reference(stream, warm)
    res = ranking_metrics(torch.from_numpy(uid).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(lb).cuda(), _warm(warm, uid))
    assert sorted(res) == sorted(ref)
    for grp in ref:
        assert sorted(res[grp]) == sorted(ref[grp])
        for key, val in ref[grp].items():
            got = res[grp][key]
            if key == "LogLoss":            # float32 mean (as the reference computes it): summation order differs
                assert (np.isnan(val) and np.isnan(got)) or got == val or abs(got - val) < 2e-6 * max(1.0, abs(val)), (grp, key, got, val)
            else:
                assert abs(got - val) < 1e-9, (grp, key, got, val)
    assert "Epoch 1 Validation Results" in format_val_log(res, 1)          # renders without raising, NaN and zero counts included
    if stream == "every-user-single-class":
        assert res["Overall"]["GAUC"] == 0.0 and res["Overall"]["AUC"] != 0.0
    if stream == "nan-scores":
        assert res["Overall"]["AUC"] == 0.0 and np.isnan(res["Overall"]["LogLoss"]) and 0.0 < res["Overall"]["GAUC"] < 1.0
    if stream == "empty-epoch":
        assert all(v == 0 for grp in res.values() for v in grp.values())


@pytest.mark.parametrize("k", [1, 3, 50])
def test_ranking_metrics_at_other_k(k):
    import torch
    from news_recsys_amd.metrics import format_val_log, ranking_metrics
    uid, sc, lb = _stream("shuffled-ties")
    warm = _warm("half-of-the-ids", uid)
    ref = R.validation_metrics(uid, sc, lb, warm, k)
    res = ranking_metrics(torch.from_numpy(uid).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(lb).cuda(), warm, k)
    for grp in ref:
        assert sorted(res[grp]) == sorted(ref[grp]) and f"NDCG@{k}" in res[grp]
        for key, val in ref[grp].items():
            assert abs(res[grp][key] - val) < (2e-6 * max(1.0, abs(val)) if key == "LogLoss" else 1e-9), (grp, key)
    assert f"NDCG@{k}:" in format_val_log(res, 2, k)
