"""ItemCF recall on the GPU (csrc/nrx_itemcf.hip through ops.itemcf_similarity / ops.itemcf_recall and the drop-in module) against the numpy
restatement tests/itemcf_ref.py and the fixture recorded from the reference's own Python (tests/golden/data/itemcf.npz).

Similarity: the counts word for word; sim bit for bit.  The issue allowed 1 fp32 ulp -- both sides round a float64 quotient that could differ
in its last bit -- and asked for equality if the observed maximum was 0.  It was 0 on every shape below (the device's fp64 sqrt and divide are
correctly rounded), so the test asks for equality.  Against the RECORDED float64 sim the bound stays 1 ulp: the reference computes
x ** 0.5, which need not be the correctly rounded square root.
Recall: ops.itemcf_recall on the GPU's own sim against the restatement fed that same sim, bit for bit, for every col_splits."""
import os

import numpy as np
import pytest
import torch

from news_recsys_amd import ops
from news_recsys_amd.model.recall.ItemCF import itemCF_base as M
from tests import itemcf_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN = os.path.join(GOLDEN, "data", "itemcf_ratings_small.dat")
TEST = os.path.join(GOLDEN, "data", "itemcf_ratings_test.dat")


def _t(a, dtype=torch.int64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    flat = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) and off[-1] else np.zeros(0, dtype=np.int64)
    return off, flat


def _random_lists(rng, n_users, num_items, lengths=None, zipf=0.8):
    pop = 1.0 / (np.arange(num_items) + 1.0) ** zipf
    pop = pop / pop.sum()
    out = []
    for u in range(n_users):
        L = int(lengths[u]) if lengths is not None else int(rng.integers(0, min(num_items, 24) + 1))
        out.append(rng.choice(num_items, size=min(L, num_items), replace=False, p=pop))        # unsorted on purpose
    return out


def _check_similarity(lists, num_items, col_tile=0, dtype=torch.int64):
    off, flat = _csr(lists)
    sim, count, co = ops.itemcf_similarity(_t(off), _t(flat, dtype), num_items, return_counts=True, col_tile=col_tile)
    n, want_co = R.counts(off, flat, num_items)
    want = R.similarity(want_co, n)
    assert sim.dtype == torch.float32 and co.dtype == torch.int32 and count.dtype == torch.int64
    assert np.array_equal(count.cpu().numpy(), n)
    assert np.array_equal(co.cpu().numpy(), want_co.astype(np.int32))
    got = sim.cpu().numpy()
    ulp = R.ulp_distance(got, want)
    print(f"itemcf_similarity I={num_items} U={len(lists)} col_tile={col_tile}: max ulp distance {int(ulp.max())}")
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    only_sim, _ = ops.itemcf_similarity(_t(off), _t(flat, dtype), num_items, col_tile=col_tile)      # the same bits without the counts
    assert torch.equal(only_sim, sim)
    return sim, co


# ---- similarity ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "data", "itemcf.npz")))


@pytest.fixture(scope="module")
def fixture_lists(gold):
    history = M.build_user_item_history(TRAIN)
    index = {str(n): i for i, n in enumerate(gold["item_order"])}
    return history, [[index[i] for i in items] for items in history.values()]


def test_similarity_on_the_fixture_matches_the_reference(gold, fixture_lists):
    _, lists = fixture_lists
    I = len(gold["item_order"])
    sim, co = _check_similarity(lists, I)
    assert np.array_equal(co.cpu().numpy(), gold["co"])
    assert int(R.ulp_distance(sim.cpu().numpy(), gold["sim"].astype(np.float32)).max()) <= 1


@pytest.mark.parametrize("lists,num_items", [
    ([[0]], 1),                                             # I = 1, U = 1
    ([[0, 1]], 2),                                          # one user holding both items
    ([[], [3], [], [1, 3], [2]], 4),                        # empty and one-item lists
    ([[], []], 3),                                          # nobody holds anything
    ([[1, 4], [4, 1, 0], [0]], 9),                          # num_items past every id seen: empty rows and columns
    ([[2, 0, 2, 1, 0]], 3),                                 # an item listed twice counts once
], ids=["one", "pair", "short_lists", "all_empty", "unused_ids", "duplicates"])
def test_similarity_smallest_shapes(lists, num_items):
    sim, co = _check_similarity(lists, num_items)
    assert torch.all(torch.diagonal(sim) == 0) and torch.all(torch.diagonal(co) == 0)


@pytest.mark.parametrize("num_items", [63, 64, 65, 129, 200])
def test_similarity_tile_edges(num_items):
    """col_tile = 64: tile edges and the diagonal element in every tile position; int32 ids on the odd sizes."""
    rng = np.random.default_rng(num_items)
    lists = _random_lists(rng, 70, num_items)
    lists.append(np.arange(num_items))                      # one user holding everything: every entry off the diagonal is non-zero
    _check_similarity(lists, num_items, col_tile=64, dtype=torch.int32 if num_items % 2 else torch.int64)


@pytest.mark.parametrize("n_users", [300, 1100])
def test_similarity_one_item_held_by_every_user(n_users):
    """300: more users of one item than one wave takes at a time (64); 1100: more than one pass of a workgroup's 16 waves takes (1024)."""
    rng = np.random.default_rng(n_users)
    lists = [np.concatenate([[5], rng.choice(np.delete(np.arange(40), 5), size=int(rng.integers(0, 9)), replace=False)]) for _ in range(n_users)]
    sim, co = _check_similarity(lists, 40, col_tile=64)
    assert int(co[5].sum()) == sum(len(l) - 1 for l in lists)


def test_similarity_list_lengths_around_the_wave_width():
    rng = np.random.default_rng(257)
    lengths = [1, 63, 64, 65, 257, 64, 65, 1, 257]
    _check_similarity(_random_lists(rng, len(lengths), 300, lengths=lengths, zipf=0.3), 300)
    _check_similarity(_random_lists(rng, len(lengths), 300, lengths=lengths, zipf=0.3), 300, col_tile=64)


def test_similarity_does_not_depend_on_the_order_of_the_users():
    rng = np.random.default_rng(11)
    lists = _random_lists(rng, 90, 150)
    off, flat = _csr(lists)
    a = ops.itemcf_similarity(_t(off), _t(flat), 150, return_counts=True, col_tile=64)
    perm = rng.permutation(len(lists))
    off2, flat2 = _csr([lists[p][::-1] for p in perm])
    b = ops.itemcf_similarity(_t(off2), _t(flat2), 150, return_counts=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_similarity_past_the_default_tile_width():
    """I = 16 385 = the default tile width plus one (a 1.07 GB sim), 64 users; checked on the device, the matrix never comes to the host."""
    I = ops.ITEMCF_TILE_MAX + 1
    rng = np.random.default_rng(16385)
    lists = [np.concatenate([rng.choice(I, size=36, replace=False), [0, 16383, 16384][: 1 + u % 3]]) for u in range(64)]
    off, flat = _csr(lists)
    sim, count = ops.itemcf_similarity(_t(off), _t(flat), I)
    rows, cols, c, want = R.pair_list(off, flat, I)
    assert int(torch.count_nonzero(sim)) == len(c)
    got = sim[_t(rows), _t(cols)].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(count.cpu().numpy(), np.bincount(np.concatenate([np.unique(l) for l in lists]), minlength=I))
    assert float(sim[16384, 0]) > 0 and float(sim[0, 16384]) == float(sim[16384, 0])        # the one-column second tile is reached from both sides
    del sim
    torch.cuda.empty_cache()


def test_similarity_refuses_what_does_not_fit():
    with pytest.raises(ValueError, match="free"):
        ops.itemcf_similarity(_t([0, 1]), _t([0]), 1 << 20)                                 # a 4 TiB matrix
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        ops.itemcf_similarity(_t([0, 1]), _t([4]), 4)
    with pytest.raises(ValueError, match="offsets"):
        ops.itemcf_similarity(_t([0, 3]), _t([0]), 4)


# ---- recall -------------------------------------------------------------------------------------------------------------------------------
def _recall_case(num_items):
    """(sim on the device, sim on the host, query histories): lengths 0, 1, 64, 65 where the items allow, and one history of every item."""
    rng = np.random.default_rng(1000 + num_items)
    lists = _random_lists(rng, 80, num_items, zipf=0.5)
    off, flat = _csr(lists)
    sim, _ = ops.itemcf_similarity(_t(off), _t(flat), num_items)
    hists = [rng.choice(num_items, size=L, replace=False) for L in (0, 1, 64, 65, 7, 20) if L <= num_items]
    hists.append(np.arange(num_items))
    hists.append(np.zeros(0, dtype=np.int64))
    return sim, sim.cpu().numpy(), hists


@pytest.fixture(scope="module", params=[31, 65, 200])
def recall_case(request):
    return _recall_case(request.param)


def _same(got, want):
    idx, sc = got
    return np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(sc.cpu().numpy().view(np.int32), want[1].view(np.int32))


@pytest.mark.parametrize("k", [1, 32, 33, 50])
def test_recall_is_the_restatement_on_the_gpus_own_sim_for_every_split(recall_case, k):
    sim, sim_host, hists = recall_case
    off, flat = _csr(hists)
    want = R.recall(sim_host, off, flat, k)
    I = sim.shape[0]
    assert np.all(want[0][-2:] == -1) and np.all(want[1][-2:] == -R.FLT_MAX)                 # every item held; the empty history
    assert np.all(want[0][0] == -1)
    if I == 31 and k >= 32:
        assert np.all(want[0][:, -1] == -1)                                                   # fewer candidates than k: the tail is filled
    for splits in (1, 2, 3, 0):
        got = ops.itemcf_recall(sim, (_t(off), _t(flat)), k, col_splits=splits)
        assert got[0].dtype == torch.int64 and got[0].shape == (len(hists), k) and got[1].dtype == torch.float32
        assert _same(got, want), (I, k, splits)
    got = ops.itemcf_recall(sim, (_t(off), _t(flat, torch.int32)), k, col_splits=2)          # 32-bit ids
    assert _same(got, want)


@pytest.mark.parametrize("k", [10, 40])
def test_recall_with_an_exclusion_list_of_its_own(recall_case, k):
    sim, sim_host, hists = recall_case
    I = sim.shape[0]
    rng = np.random.default_rng(I + k)
    excl = [rng.choice(I, size=int(rng.integers(0, I // 2)), replace=False) for _ in hists]
    excl[1] = np.zeros(0, dtype=np.int64)                                                   # nothing excluded: the history's own items may return
    off, flat = _csr(hists)
    eoff, eflat = _csr(excl)
    want = R.recall(sim_host, off, flat, k, eoff, np.concatenate([np.sort(e) for e in excl]))
    for splits in (1, 3):
        assert _same(ops.itemcf_recall(sim, (_t(off), _t(flat)), k, exclude=(_t(eoff), _t(eflat)), col_splits=splits), want)
    for q, e in enumerate(excl):
        assert not set(want[0][q].tolist()) & set(e.tolist())
    with pytest.raises(ValueError, match="exclude"):
        ops.itemcf_recall(sim, (_t(off), _t(flat)), k, exclude=(_t(eoff[:-1]), _t(eflat[:eoff[-2]])))


def test_recall_without_queries_and_bad_shapes():
    sim = torch.zeros(4, 4, device=DEV)
    idx, sc = ops.itemcf_recall(sim, (_t([0]), _t([])), 5)
    assert idx.shape == (0, 5) and sc.shape == (0, 5)
    idx, sc = ops.itemcf_recall(sim, (_t([0, 2]), _t([1, 3])), 40)                         # an all-zero matrix has no candidate
    assert torch.all(idx == -1) and torch.all(sc == -float(R.FLT_MAX))
    with pytest.raises(ValueError, match="square"):
        ops.itemcf_recall(torch.zeros(4, 5, device=DEV), (_t([0]), _t([])), 5)
    with pytest.raises(ValueError, match="k must"):
        ops.itemcf_recall(sim, (_t([0]), _t([])), 0)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        ops.itemcf_recall(sim, (_t([0, 1]), _t([4])), 5)


@pytest.mark.parametrize("k", [5, 10])
def test_recall_against_the_recorded_reference_scores_tie_aware(gold, fixture_lists, k):
    """tol = 1e-5 relative: four times the 40 * 2^-24 bound on an fp32 sum of at most 40 positive terms, ten times below the fixture's gap."""
    _, lists = fixture_lists
    I = len(gold["item_order"])
    off, flat = _csr(lists)
    sim, _ = ops.itemcf_similarity(_t(off), _t(flat), I)
    idx, sc = (t.cpu().numpy() for t in ops.itemcf_recall(sim, (_t(off), _t(flat)), k))
    for u in range(len(lists)):
        rec = gold["scores"][u]
        ranked = np.sort(rec[rec > 0])[::-1]
        live = idx[u] >= 0
        assert live.sum() == min(k, len(ranked))
        if not len(ranked):
            continue
        s_k = ranked[min(k, len(ranked)) - 1]
        tol = 1e-5 * s_k
        assert np.all(rec[idx[u][live]] >= s_k - tol)
        assert set(np.nonzero(rec > s_k + tol)[0].tolist()) <= set(idx[u][live].tolist())
        np.testing.assert_allclose(sc[u][live], rec[idx[u][live]], rtol=1e-5, atol=0)


# ---- the drop-in module -------------------------------------------------------------------------------------------------------------------
def test_drop_in_functions_on_the_fixture_files(gold):
    history = M.build_user_item_history(TRAIN)
    item_sim = M.compute_item_similarity(history)
    assert item_sim.item_names == [str(n) for n in gold["item_order"]] and len(item_sim) == len(gold["item_order"])
    assert np.array_equal(item_sim.item_count.cpu().numpy(), gold["item_count"])
    d = item_sim.to_dict()
    names = item_sim.item_names
    want_keys = {(names[i], names[j]) for i, j in zip(*np.nonzero(gold["sim"]))}
    assert {(a, b) for a, row in d.items() for b in row} == want_keys
    for a, row in d.items():
        for b, v in row.items():
            assert isinstance(v, float) and abs(v - gold["sim"][item_sim.item_index[a], item_sim.item_index[b]]) <= 1e-6 * v
    for k in (5, 10):
        for u, user in enumerate(gold["users"][:6]):
            got = M.recall_top_k_items(str(user), history, item_sim, k)
            assert isinstance(got, list) and set(got) == {str(x) for x in gold[f"top{k}_names"][u] if x}
        assert M.hit_rate(TEST, history, item_sim, k=k) == float(gold[f"hit_rate{k}"])
    assert M.recall_top_k_items("no such user", history, item_sim) == []
    short = M.recall_top_k_items("1", history, item_sim, k=40)                   # fewer than k candidates: a shorter list
    assert 0 < len(short) == int((gold["scores"][0] > 0).sum()) < 40 and not set(short) & set(history["1"])


def test_itemcf_class_on_index_tensors(gold, fixture_lists):
    history, lists = fixture_lists
    I = len(gold["item_order"])
    off, flat = _csr(lists)
    model = M.ItemCF().fit(_t(off), _t(flat), I)
    assert np.array_equal(model.item_count.cpu().numpy(), gold["item_count"])
    idx, _ = model.recall((_t(off), _t(flat)), 10)
    names = [str(n) for n in gold["item_order"]]
    assert {names[i] for i in idx[0].tolist() if i >= 0} == {str(x) for x in gold["top10_names"][0] if x}
    users = {str(u): i for i, u in enumerate(gold["users"])}
    index = {n: i for i, n in enumerate(names)}
    pairs = [line.split("::")[:2] for line in open(TEST, encoding="ISO-8859-1").read().splitlines()]
    tu = _t([users.get(u, len(users) + 5) for u, _ in pairs])                     # the stranger: an index past the fitted users
    ti = _t([index[i] for _, i in pairs])
    for k in (5, 10):
        assert model.hit_rate(tu, ti, k) == float(gold[f"hit_rate{k}"])


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------
def test_similarity_and_recall_replay_from_a_captured_graph():
    """The two launch functions allocate, copy and synchronise nothing: captured once, replayed on changed inputs of the same shape."""
    I, U, K = 150, 60, 10
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, 25, U)

    def prepared(seed):
        off, flat = _csr(_random_lists(np.random.default_rng(seed), U, I, lengths=lengths))
        u_off, u_items, owner = ops._csr_pair((_t(off), _t(flat)), None, I, "test")
        item_off, users, _ = ops._itemcf_csc(u_items, owner, I)
        return [u_off, u_items, item_off, users]

    datasets = [prepared(s) for s in (1, 2, 3)]
    eager = []
    for d in datasets:
        sim, _, co = ops.itemcf_similarity(d[0], d[1], I, return_counts=True)
        eager.append((sim, co) + ops.itemcf_recall(sim, (d[0], d[1]), K, col_splits=2))
    static = [t.clone() for t in datasets[0]]
    sim = torch.empty(I, I, device=DEV)
    co = torch.empty(I, I, dtype=torch.int32, device=DEV)
    idx = torch.empty(U, K, dtype=torch.int64, device=DEV)
    sc = torch.empty(U, K, device=DEV)
    ws = torch.empty(ops.itemcf_recall_workspace(I, U, K, 2), dtype=torch.uint8, device=DEV)

    def step():
        ops._itemcf_similarity_launch(static[0], static[1], static[2], static[3], I, sim, co)
        ops._itemcf_recall_launch(sim, static[0], static[1], static[0], static[1], K, 2, idx, sc, ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for d, want in zip(datasets[1:], eager[1:]):
        for dst, src in zip(static, d):
            dst.copy_(src)
        for out in (sim, co, idx, sc):
            out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sim, want[0]) and torch.equal(co, want[1]) and torch.equal(idx, want[2])
        assert torch.equal(sc.view(torch.int32), want[3].view(torch.int32))
