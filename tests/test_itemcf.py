"""ItemCF recall without a GPU: the numpy restatement (tests/itemcf_ref.py) against what the reference's own Python recorded
(tests/golden/data/itemcf.npz, tests/golden/gen_itemcf_golden.py), the drop-in module's host half, and the argument validation of the two
entry points (nothing is launched).  The kernels themselves: tests/test_itemcf_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.recall.ItemCF import itemCF_base as M
from tests import itemcf_ref as R
from tests.conftest import GOLDEN, ROOT

TRAIN = os.path.join(GOLDEN, "data", "itemcf_ratings_small.dat")
TEST = os.path.join(GOLDEN, "data", "itemcf_ratings_test.dat")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "data", "itemcf.npz")))


@pytest.fixture(scope="module")
def fixture_csr(gold):
    """The training file as index CSR (user order and item indices of the fixture), through the module's own host parse."""
    history = M.build_user_item_history(TRAIN)
    index = {str(n): i for i, n in enumerate(gold["item_order"])}
    off, flat = M._history_csr(history, index)
    return history, np.array(off, dtype=np.int64), np.array(flat, dtype=np.int64)


def test_fixture_has_the_shape_the_generator_promises(gold):
    lines = open(TRAIN, encoding="ISO-8859-1").read().splitlines()
    per_user = {}
    for line in lines:
        u, i, _, _ = line.split("::")
        per_user.setdefault(u, set()).add(i)
    assert len(per_user) == 48 and len(gold["item_order"]) <= 40
    assert all(3 <= len(s) <= 18 for s in per_user.values())
    assert len(lines) == sum(len(s) for s in per_user.values()) + 3            # three re-ratings
    assert len(open(TEST, encoding="ISO-8859-1").read().splitlines()) == 49      # one per user and one stranger
    assert os.path.getsize(os.path.join(GOLDEN, "data", "itemcf.npz")) < (1 << 20)


def test_host_parse_and_name_map_match_the_fixture(gold, fixture_csr):
    history, off, flat = fixture_csr
    assert list(history) == [str(u) for u in gold["users"]]
    order = list(dict.fromkeys(i for items in history.values() for i in items))
    assert order == [str(n) for n in gold["item_order"]]
    first = next(iter(history["1"].values()))
    assert isinstance(first, tuple) and isinstance(first[0], float) and isinstance(first[1], str)
    # the index map compute_item_similarity builds is the same order of first appearance
    index = {}
    off2, flat2 = M._history_csr(history, index, grow=True)
    assert list(index) == order and off2 == off.tolist() and flat2 == flat.tolist()
    # items the map does not know are skipped when it may not grow
    assert M._history_csr({"u": {"nope": (1.0, "0"), order[3]: (1.0, "0")}}, dict(index)) == ([0, 1], [3])


def test_duplicate_ratings_of_one_pair_collapse_to_one(tmp_path, gold, fixture_csr):
    p = tmp_path / "r.dat"
    p.write_text("7::a::3::10\n7::b::4::11\n7::a::5::12\n8::b::1::13\n", encoding="ISO-8859-1")
    h = M.build_user_item_history(str(p))
    assert h == {"7": {"a": (5.0, "12"), "b": (4.0, "11")}, "8": {"b": (1.0, "13")}}
    # ... and in the restatement: a list that names an item twice counts it once
    n, co = R.counts([0, 3, 4], [0, 1, 0, 1], 2)
    assert n.tolist() == [1, 2] and co.tolist() == [[0, 1], [1, 0]]
    # the fixture's three re-rated pairs are one entry each
    history, off, flat = fixture_csr
    assert len(flat) == sum(len(v) for v in history.values()) == int(gold["item_count"].sum())


def test_ref_counts_and_similarity_match_the_reference(gold, fixture_csr):
    _, off, flat = fixture_csr
    I = len(gold["item_order"])
    n, co = R.counts(off, flat, I)
    assert np.array_equal(n, gold["item_count"]) and np.array_equal(co, gold["co"])
    s64 = R.similarity64(co, n)
    assert np.array_equal(s64 != 0, gold["sim"] != 0)
    np.testing.assert_allclose(s64, gold["sim"], rtol=1e-12, atol=0)
    assert R.similarity(co, n).dtype == np.float32
    rows, cols, c, s = R.pair_list(off, flat, I)                                # the sparse form the large GPU case uses
    assert np.array_equal(co[rows, cols], c) and len(c) == np.count_nonzero(co) and np.array_equal(R.similarity(co, n)[rows, cols], s)


@pytest.mark.parametrize("k", [5, 10])
def test_ref_recall_returns_the_references_top_k_sets_and_hit_rate(gold, fixture_csr, k):
    history, off, flat = fixture_csr
    I = len(gold["item_order"])
    n, co = R.counts(off, flat, I)
    idx, sc = R.recall(R.similarity(co, n), off, flat, k)
    names = [str(x) for x in gold["item_order"]]
    users = [str(u) for u in gold["users"]]
    recalled = {}
    for u in range(len(users)):
        want = {str(x) for x in gold[f"top{k}_names"][u] if x}
        got = {names[i] for i in idx[u] if i >= 0}
        assert got == want, (u, got, want)
        recalled[users[u]] = got
        live = idx[u] >= 0
        np.testing.assert_allclose(sc[u][live], gold["scores"][u][idx[u][live]], rtol=1e-5)
        assert np.all(sc[u][~live] == -R.FLT_MAX) and np.all(np.diff(sc[u].astype(np.float64)) <= 0)
    pairs = [line.split("::")[:2] for line in open(TEST, encoding="ISO-8859-1").read().splitlines()]
    hits = sum(1 for u, i in pairs if i in recalled.get(u, ()))
    assert hits / len(pairs) == float(gold[f"hit_rate{k}"])


def test_ref_recall_order_exclusion_and_filling():
    sim = np.array([[0, .5, .5, 0], [.5, 0, .25, 0], [.5, .25, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    idx, sc = R.recall(sim, [0, 1, 1, 3], [0, 1, 2], 3)
    assert idx.tolist() == [[1, 2, -1], [-1, -1, -1], [0, -1, -1]]              # ties by index; empty history; item 3 never scores
    assert sc[0].tolist() == [0.5, 0.5, -float(R.FLT_MAX)] and sc[2, 0] == 1.0
    idx, _ = R.recall(sim, [0, 1], [0], 2, [0, 1], [1])                           # an explicit exclusion list replaces the history
    assert idx.tolist() == [[2, -1]]


# ---- argument validation through ctypes: -1 and the function's name before any launch (there is no device here) ----------------------------
class _Bufs:
    def __init__(self):
        self.keep = [ctypes.create_string_buffer(4096 + 64) for _ in range(9)]
        base = [(ctypes.addressof(b) + 63) & ~63 for b in self.keep]
        self.uoff, self.items, self.ioff, self.users, self.sim, self.co, self.oidx, self.osc, self.ws = base


def _sim(lib, b, **kw):
    a = dict(uoff=b.uoff, items=b.items, nu=4, ioff=b.ioff, users=b.users, ni=8, bits=64, tile=0, sim=b.sim, co=b.co)
    a.update(kw)
    return lib.nrx_itemcf_similarity(a["uoff"], a["items"], a["nu"], a["ioff"], a["users"], a["ni"], a["bits"], a["tile"], a["sim"], a["co"],
                                     None, None)


def _rec(lib, b, **kw):
    a = dict(sim=b.sim, ni=8, hoff=b.uoff, hitems=b.items, eoff=b.ioff, eitems=b.users, bits=64, nq=4, k=10, splits=0, oidx=b.oidx,
             osc=b.osc, ws=b.ws)
    a.update(kw)
    return lib.nrx_itemcf_recall(a["sim"], a["ni"], a["hoff"], a["hitems"], a["eoff"], a["eitems"], a["bits"], a["nq"], a["k"], a["splits"],
                                 a["oidx"], a["osc"], a["ws"], None)


@pytest.mark.parametrize("kw,word", [(dict(uoff=None), "null"), (dict(items=None), "null"), (dict(ioff=None), "null"), (dict(users=None), "null"),
                                     (dict(sim=None), "null"), (dict(ni=0), "n_items"), (dict(ni=-1), "n_items"), (dict(ni=2 ** 31 - 1), "n_items"),
                                     (dict(nu=-1), "n_users"), (dict(bits=16), "index_bits"), (dict(bits=0), "index_bits"),
                                     (dict(tile=-1), "col_tile"), (dict(tile=16385), "col_tile"), (dict(ni=2 ** 31 - 16, tile=64), "col_tile")])
def test_similarity_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    assert _sim(lib, _Bufs(), **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_itemcf_similarity" in lib.nrx_last_error()


@pytest.mark.parametrize("kw,word", [(dict(sim=None), "null"), (dict(hoff=None), "null"), (dict(hitems=None), "null"), (dict(eoff=None), "null"),
                                     (dict(eitems=None), "null"), (dict(oidx=None), "null"), (dict(osc=None), "null"), (dict(ws=None), "null"),
                                     (dict(ni=0), "n_items"), (dict(ni=2 ** 31 - 1), "n_items"), (dict(nq=-1), "n_queries"),
                                     (dict(k=0), "k must"), (dict(k=-2), "k must"), (dict(k=33), "k must"),
                                     (dict(bits=16), "index_bits"), (dict(bits=48), "index_bits"),
                                     (dict(splits=-1), "col_splits"), (dict(splits=1025), "col_splits")])
def test_recall_rejects_bad_arguments_before_any_launch(kw, word):
    lib = _lib.load()
    assert _rec(lib, _Bufs(), **kw) == -1
    assert word.encode() in lib.nrx_last_error() and b"nrx_itemcf_recall" in lib.nrx_last_error()


def test_misaligned_pointers_empty_calls_and_the_size_call():
    lib = _lib.load()
    b = _Bufs()
    assert _sim(lib, b, items=b.items + 4) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    assert _sim(lib, b, co=b.co + 2) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    assert _rec(lib, b, hoff=b.uoff + 4) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    assert _rec(lib, b, eitems=b.users + 2, bits=32) == -1 and b"misaligned pointer" in lib.nrx_last_error()
    # no query: NRX_OK without a launch (no device here: a launch would fail), whatever the pointers
    assert _rec(lib, b, nq=0) == 0
    assert _rec(lib, b, nq=0, sim=None, hoff=None, hitems=None, eoff=None, eitems=None, oidx=None, osc=None, ws=None) == 0
    assert lib.nrx_itemcf_recall_workspace(100, 7, 10, 3) >= 3 * 7 * 10 * 8
    assert lib.nrx_itemcf_recall_workspace(2, 7, 1, 3) >= 2 * 7 * 4 * 8
    for bad in ((0, 7, 10, 0), (100, -1, 10, 0), (100, 7, 0, 0), (100, 7, 33, 0), (100, 7, 10, -1), (100, 7, 10, 1025), (2 ** 31 - 1, 7, 10, 0)):
        assert lib.nrx_itemcf_recall_workspace(*bad) == -1, bad
    with pytest.raises(ValueError, match="itemcf_recall"):
        ops.itemcf_recall_workspace(100, 7, 33)
    assert lib.nrx_abi_version() == 3 == _lib.NRX_ABI_VERSION            # the additions are additive


def test_ops_have_no_cpu_path():
    off, items = torch.tensor([0, 2]), torch.tensor([0, 1])
    with pytest.raises(_lib.NrxError, match="itemcf_similarity"):
        ops.itemcf_similarity(off, items, 2)
    with pytest.raises(_lib.NrxError, match="itemcf_recall"):
        ops.itemcf_recall(torch.zeros(2, 2), (off, items), 1)
    with pytest.raises(ValueError, match="num_items"):
        ops.itemcf_similarity(off, items, 0)
    with pytest.raises(ValueError, match="fit"):
        M.ItemCF().recall((off, items), 1)
    assert M.recall_top_k_items("nobody", {"a": {}}, None, 5) == []            # an unknown user never reaches the device


# ---- the host half of the entry points under ASan + UBSan: a stand-alone driver with its own main, run directly
def test_itemcf_host_validation_is_clean_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    if not os.path.exists(os.path.join(ROOT, "tests", "sanitize", "itemcf.mk")):
        pytest.skip("tests/sanitize/ is not part of this tree (it does not travel to the GPU machines)")
    p = subprocess.run(["make", "-C", "tests/sanitize", "-f", "itemcf.mk", "run"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert "nrx_itemcf validation sanitize driver: OK" in out
