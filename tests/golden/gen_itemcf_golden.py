#!/usr/bin/env python3
"""Regenerates the ItemCF fixture from the reference's own Python (src/model/recall/ItemCF/itemCF_base.py of the checkout named by
NRX_REFERENCE_DIR; the suite never runs this script and needs no checkout):

    NRX_REFERENCE_DIR=<checkout> python tests/golden/gen_itemcf_golden.py          # rewrites the three files below
    NRX_REFERENCE_DIR=<checkout> python tests/golden/gen_itemcf_golden.py --check  # regenerates into a temp dir, compares bit for bit

  tests/golden/data/itemcf_ratings_small.dat   synthetic `user::item::rating::timestamp` lines: 48 users over 40 items, 3-18 distinct items
                                               per user drawn without replacement with popularity ~ 1 / (rank + 1)^0.8; three users rate
                                               their first item a second time (the reference's dicts keep one entry)
  tests/golden/data/itemcf_ratings_test.dat    one held-out line per user (an item outside the user's history) and one line of a user the
                                               training file does not know
  tests/golden/data/itemcf.npz                 what the reference's four functions give on them: item order (first appearance), item_count,
                                               the dense count matrix, sim (float64), every user's score of every candidate item (float64,
                                               summed in the reference's dict order; 0 = not a candidate), the top-k names and scores for
                                               k = 5 and 10, both hit rates.  Data only.
(The npz sits under data/: gen_golden.py --check treats every npz directly under tests/golden/ as its own.)

A seed is accepted only if, for every user and both k, the k-th and (k+1)-th reference scores differ by more than 1e-4 relative: an fp32
sum of at most 40 positive terms is off by at most about 40 * 2^-24 = 2.4e-6 relative, so no rounding can reorder items across the cut,
while a tie at the cut would leave the top-k set -- and the hit rate -- to the reference's dict insertion order."""
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NRX_REFERENCE_DIR", "")
USERS, ITEMS, KS, GAP = 48, 40, (5, 10), 1e-4
FILES = ("itemcf_ratings_small.dat", "itemcf_ratings_test.dat", "itemcf.npz")


def reference_module():
    path = os.path.join(REF, "src", "model", "recall", "ItemCF", "itemCF_base.py")
    spec = importlib.util.spec_from_file_location("reference_itemcf_base", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_ratings(seed, out_dir):
    rng = np.random.default_rng(seed)
    pop = 1.0 / (np.arange(ITEMS) + 1.0) ** 0.8
    names = [str(n) for n in rng.permutation(np.arange(1001, 1001 + ITEMS))]       # name of the item of popularity rank r
    train, test = [], []
    for u in range(USERS):
        held = rng.choice(ITEMS, size=int(rng.integers(3, 19)) + 1, replace=False, p=pop / pop.sum())
        stamp = 978300000 + 1000 * u
        for t, r in enumerate(held[:-1]):
            train.append(f"{u + 1}::{names[r]}::{int(rng.integers(1, 6))}::{stamp + t}")
        if u < 3:
            train.append(f"{u + 1}::{names[held[0]]}::{int(rng.integers(1, 6))}::{stamp + 500}")
        test.append(f"{u + 1}::{names[held[-1]]}::{int(rng.integers(1, 6))}::{stamp + 900}")
    test.append(f"{USERS + 1000}::{names[0]}::5::978399999")
    paths = [os.path.join(out_dir, f) for f in FILES[:2]]
    for path, lines in zip(paths, (train, test)):
        with open(path, "w", encoding="ISO-8859-1", newline="\n") as f:
            f.write("\n".join(lines) + "\n")
    return paths


def record(ref, train_path, test_path):
    """The arrays of the fixture, or None when some cut is closer than GAP."""
    history = ref.build_user_item_history(train_path)
    sim = ref.compute_item_similarity(history)
    order = list(dict.fromkeys(item for items in history.values() for item in items))
    index = {name: i for i, name in enumerate(order)}
    n_items = len(order)
    count = np.zeros(n_items, dtype=np.int64)
    co = np.zeros((n_items, n_items), dtype=np.int64)
    for items in history.values():
        idx = [index[i] for i in items]
        count[idx] += 1
        co[np.ix_(idx, idx)] += 1
    np.fill_diagonal(co, 0)
    sim64 = np.zeros((n_items, n_items), dtype=np.float64)
    for a, row in sim.items():
        for b, v in row.items():
            sim64[index[a], index[b]] = v
    assert np.array_equal(sim64 != 0, co != 0)
    users = list(history)
    scores = np.zeros((len(users), n_items), dtype=np.float64)
    for u, user in enumerate(users):                      # the reference's own summation order: the user's dict, then the row's dict
        acc = {}
        for a in history[user]:
            for b, v in sim.get(a, {}).items():
                if b not in history[user]:
                    acc[b] = acc.get(b, 0) + v
        for b, v in acc.items():
            scores[u, index[b]] = v
    out = {"item_order": np.array(order), "users": np.array(users), "item_count": count, "co": co, "sim": sim64, "scores": scores}
    for k in KS:
        names = np.full((len(users), k), "", dtype=f"<U{max(len(n) for n in order)}")
        top = np.full((len(users), k), np.nan, dtype=np.float64)
        for u, user in enumerate(users):
            got = ref.recall_top_k_items(user, history, sim, k)
            ranked = np.sort(scores[u][scores[u] > 0])[::-1]
            if len(ranked) > k and not ranked[k - 1] - ranked[k] > GAP * ranked[k - 1]:
                return None
            names[u, :len(got)] = got
            top[u, :len(got)] = [scores[u, index[g]] for g in got]
            assert np.array_equal(top[u, :len(got)], ranked[:len(got)])
        out[f"top{k}_names"] = names
        out[f"top{k}_scores"] = top
        out[f"hit_rate{k}"] = np.float64(ref.hit_rate(test_path, history, sim, k))
    assert ref.recall_top_k_items("no such user", history, sim, 5) == []
    return out


def generate(out_dir):
    ref = reference_module()
    os.makedirs(out_dir, exist_ok=True)
    for seed in range(60):
        train_path, test_path = write_ratings(seed, out_dir)
        arrays = record(ref, train_path, test_path)
        if arrays is not None:
            arrays["seed"] = np.int64(seed)
            np.savez(os.path.join(out_dir, FILES[2]), **arrays)
            return seed
    sys.exit("no seed below 60 keeps every top-k cut wider than the gap")


def differences(a_dir, b_dir):
    bad = []
    for f in FILES[:2]:
        if open(os.path.join(a_dir, f), "rb").read() != open(os.path.join(b_dir, f), "rb").read():
            bad.append(f)
    a, b = np.load(os.path.join(a_dir, FILES[2])), np.load(os.path.join(b_dir, FILES[2]))
    if sorted(a.files) != sorted(b.files):
        return bad + [FILES[2] + ": key sets differ"]
    for k in a.files:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(f"{FILES[2]}:{k}")
    return bad


if __name__ == "__main__":
    if not REF or not os.path.isdir(REF):
        sys.exit("set NRX_REFERENCE_DIR to a checkout of the reference project")
    data = os.path.join(HERE, "data")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            generate(tmp)
            bad = differences(data, tmp)
        if bad:
            sys.exit("the ItemCF fixture differs from a regeneration:\n  " + "\n  ".join(bad))
        print("OK: a regeneration reproduces the committed ItemCF fixture bit for bit")
    else:
        print(f"ItemCF fixture written from seed {generate(data)}")
