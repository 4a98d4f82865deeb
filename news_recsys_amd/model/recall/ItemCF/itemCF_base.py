"""Item-based collaborative filtering on the GPU: drop-in for the reference's src/model/recall/ItemCF/itemCF_base.py.

The four functions keep the reference's names and signatures (its `__main__` block runs against this module unchanged), but the
dict-of-dict loops are two HIP kernels (csrc/nrx_itemcf.hip through ops.itemcf_similarity / ops.itemcf_recall):
  compute_item_similarity   exact integer co-occurrence counts in LDS, one normalisation  -> an ItemSimilarity (device matrix + name map)
  recall_top_k_items        the sum of the history's rows of the matrix and a top-k, the history excluded
  hit_rate                  every distinct test user recalled in ONE launch, hits counted on the host
Differences from the reference, both in what it leaves open: scores are fp32 sums over the history in ascending item index (the reference
adds Python floats in dict order), and equal scores are ordered by item index (the reference: by dict insertion).
`ItemCF` is the same model on index tensors (CSR histories on the device), for data that never was strings -- the `history` bag column
of ColumnarLoader, say."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from news_recsys_amd import ops


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _rating_lines(path):
    """The fields of a MovieLens-style ratings file: `user::item::rating::timestamp` per line, ISO-8859-1."""
    with open(path, "r", encoding="ISO-8859-1") as f:
        for line in f:
            user, item, rating, stamp = line.strip().split("::")
            yield user, item, rating, stamp


def build_user_item_history(rating_file_path):
    """itemCF_base.py:6-14: {user: {item: (rating, timestamp)}} in file order; a later rating of the same pair replaces the earlier one."""
    history: Dict[str, Dict[str, Tuple[float, str]]] = {}
    for user, item, rating, stamp in _rating_lines(rating_file_path):
        history.setdefault(user, {})[item] = (float(rating), stamp)
    return history


class ItemSimilarity:
    """What compute_item_similarity returns: sim fp32 [I, I] on the device, item_names (index -> name, in the order of first appearance
    while iterating the history), item_index (name -> index) and item_count int64 [I] (users per item)."""

    def __init__(self, sim: torch.Tensor, item_names: Sequence[str], item_count: torch.Tensor):
        self.sim = sim
        self.item_names = list(item_names)
        self.item_index = {name: i for i, name in enumerate(self.item_names)}
        self.item_count = item_count

    def __len__(self):
        return len(self.item_names)

    def to_dict(self) -> Dict[str, Dict[str, float]]:
        """The reference's dict of dicts (only pairs with a co-occurrence; values are the fp32 entries as Python floats)."""
        sim = self.sim.cpu()
        rows, cols = torch.nonzero(sim, as_tuple=True)
        vals = sim[rows, cols].tolist()
        out: Dict[str, Dict[str, float]] = {}
        for i, j, v in zip(rows.tolist(), cols.tolist(), vals):
            out.setdefault(self.item_names[i], {})[self.item_names[j]] = v
        return out


def _history_csr(user_item_history, item_index, users=None, grow=False) -> Tuple[List[int], List[int]]:
    """Host CSR of the histories of `users` (default: all, in dict order) over item_index; items it does not know are added (grow) or skipped."""
    off, flat = [0], []
    for user in (user_item_history if users is None else users):
        for item in user_item_history[user]:
            idx = item_index.get(item)
            if idx is None:
                if not grow:
                    continue
                idx = item_index[item] = len(item_index)
            flat.append(idx)
        off.append(len(flat))
    return off, flat


def compute_item_similarity(user_item_history) -> ItemSimilarity:
    item_index: Dict[str, int] = {}
    off, flat = _history_csr(user_item_history, item_index, grow=True)
    if not item_index:
        raise ValueError("compute_item_similarity: the history holds no item")
    dev = _device()
    sim, item_count = ops.itemcf_similarity(torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(flat, dtype=torch.int64, device=dev),
                                            len(item_index))
    return ItemSimilarity(sim, list(item_index), item_count)


def _recall_names(users, user_item_history, item_similarity: ItemSimilarity, k) -> List[List[str]]:
    off, flat = _history_csr(user_item_history, item_similarity.item_index, users=users)
    dev = item_similarity.sim.device
    hist = (torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(flat, dtype=torch.int64, device=dev))
    idx, _ = ops.itemcf_recall(item_similarity.sim, hist, k)
    names = item_similarity.item_names
    return [[names[i] for i in row if i >= 0] for row in idx.tolist()]


def recall_top_k_items(user_id, user_item_history, item_similarity, k=10):
    """itemCF_base.py:43-58: the names of the k best items outside the user's history; [] for an unknown user."""
    if user_id not in user_item_history:
        return []
    return _recall_names([user_id], user_item_history, item_similarity, k)[0]


def hit_rate(test_file_path, user_item_history, item_similarity, k=10):
    """itemCF_base.py:61-74: the share of test lines whose item is among its user's k recalled items (users absent from training: misses)."""
    pairs = [(user, item) for user, item, _, _ in _rating_lines(test_file_path)]
    users = list(dict.fromkeys(u for u, _ in pairs if u in user_item_history))
    recalled = dict(zip(users, map(set, _recall_names(users, user_item_history, item_similarity, k)))) if users else {}
    hits = sum(1 for u, it in pairs if it in recalled.get(u, ()))
    return hits / len(pairs) if pairs else 0.0


class ItemCF:
    """ItemCF on index tensors.  fit() takes the users' histories as a device CSR (user_off [U + 1], items in [0, num_items));
    recall() takes query histories in the same form; hit_rate() scores held-out (user, item) index pairs against the fitted histories."""

    def __init__(self):
        self.sim: Optional[torch.Tensor] = None
        self.item_count: Optional[torch.Tensor] = None
        self.user_off: Optional[torch.Tensor] = None
        self.items: Optional[torch.Tensor] = None

    def fit(self, user_off: torch.Tensor, items: torch.Tensor, num_items: int) -> "ItemCF":
        self.sim, self.item_count = ops.itemcf_similarity(user_off, items, num_items)
        self.user_off = user_off.to(torch.int64).reshape(-1)
        self.items = items.reshape(-1)
        return self

    def recall(self, hist, k: int = 10, exclude=None):
        if self.sim is None:
            raise ValueError("ItemCF.recall: call fit() first")
        return ops.itemcf_recall(self.sim, hist, k, exclude=exclude)

    def hit_rate(self, test_users: torch.Tensor, test_items: torch.Tensor, k: int = 10) -> float:
        """hits / len(test): pair (u, i) is a hit when i is among the k items recalled from user u's fitted history.  Users outside
        [0, U) count as misses, as users absent from training do in the reference."""
        if self.sim is None:
            raise ValueError("ItemCF.hit_rate: call fit() first")
        ops._dev(test_users, "ItemCF.hit_rate: test_users")
        ops._dev(test_items, "ItemCF.hit_rate: test_items")
        test_users, test_items = test_users.reshape(-1).to(torch.int64), test_items.reshape(-1).to(torch.int64)
        if test_users.numel() != test_items.numel():
            raise ValueError("ItemCF.hit_rate: one item per test user entry")
        total = test_users.numel()
        if total == 0:
            return 0.0
        n_users = self.user_off.numel() - 1
        known = (test_users >= 0) & (test_users < n_users)
        users, inverse = torch.unique(test_users[known], return_inverse=True)
        if users.numel() == 0:
            return 0.0
        lens = self.user_off[users + 1] - self.user_off[users]
        off = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
        torch.cumsum(lens, 0, out=off[1:])
        pos = torch.arange(int(off[-1]), device=users.device) - torch.repeat_interleave(off[:-1] - self.user_off[users], lens)
        idx, _ = self.recall((off, self.items[pos]), k)
        hits = (idx[inverse] == test_items[known][:, None]).any(dim=1).sum()
        return int(hits) / total


if __name__ == "__main__":
    import sys
    if len(sys.argv) != 3:
        sys.exit("usage: python -m news_recsys_amd.model.recall.ItemCF.itemCF_base <train_ratings.dat> <test_ratings.dat>")
    train_path, test_path = sys.argv[1:]
    train_history = build_user_item_history(train_path)
    print(f"Hit Rate@10: {hit_rate(test_path, train_history, compute_item_similarity(train_history), k=10):.6f}")
