"""Host-side caches of the embedding call that must follow a table set that changes (no GPU needed), and the seed selection of
tests/test_host_paths_gpu.py.

ops._sparse_group_cache holds every table's row count for the row-sparse backward: the planner clamps an id at or above that count to the
padding row, so a stale count silently takes the gradient of every row a grown table gained.  BaseModel._embed holds the list of table
Parameters it hands to ops.embed_apply: a Parameter replaced on the module must be the one the next call reads.  Both once looked at the
FIRST table only."""
import os

import pytest
import torch

from news_recsys_amd import ops
from news_recsys_amd._lib import (NRX_BAG_MASKED_MEAN, NRX_BAG_SUM, NRX_DENSE, NRX_FEAT_BAG_CSR, NRX_MAX_FEATURES, NRX_SPARSE)
from tests import embed_cases as E
from tests.conftest import CONFIGS


def binding_can_serve(case) -> bool:
    """A launch the compiled host binding takes (ops._bound_plan, BoundPlan.forward): at most 64 features, no CSR bag."""
    return len(case.slots) <= NRX_MAX_FEATURES and not any(s.flags & NRX_FEAT_BAG_CSR for s in case.slots)


def servable_seeds():
    return [sd for sd in E.SEEDS if binding_can_serve(E.make_case(sd))]


def test_the_seeds_the_binding_serves_cover_every_kind():
    """The generated seeds both host paths are compared on are chosen by predicate; the choice must stay wide enough to mean something."""
    cases = [E.make_case(sd) for sd in servable_seeds()]
    assert len(cases) >= 15, len(cases)
    kinds = {"fm": sum(c.use_fm for c in cases), "wide": sum(c.wide_width > 0 for c in cases), "bf16": sum(c.bf16 for c in cases),
             "dense_value": sum(any(s.kind == NRX_DENSE for s in c.slots) for c in cases),
             "padded_bag": sum(any(s.bag_len and not s.flags & NRX_FEAT_BAG_CSR for s in c.slots) for c in cases)}
    assert all(v >= 1 for v in kinds.values()), kinds
    # (a sum bag without weights is one more thing the binding hands back: such seeds still run on both paths, and end on ctypes on both)
    served = [c for c in cases if not any(s.kind == NRX_BAG_SUM and w is None for s, w in zip(c.slots, c.weights))]
    assert len(served) >= 10 and any(c.use_fm for c in served) and any(c.wide_width for c in served), len(served)


def _three_table_plan():
    D = 16
    slots = [ops.Slot("a", NRX_SPARSE, 0, D, 0, 0), ops.Slot("b", NRX_SPARSE, 1, D, 0, D), ops.Slot("c", NRX_SPARSE, 2, D, 0, 2 * D),
             ops.Slot("h", NRX_BAG_MASKED_MEAN, 2, D, 4, 3 * D)]
    return ops.EmbedPlan(slots, out_width=4 * D)


def _rows_of(groups):
    """{table: row count} as the backward will hand it to the planner, from both copies the cache keeps (the list and the ctypes array)."""
    got = {}
    for g in groups:
        assert list(g["static"][1]) == list(g["rows"])
        assert list(g["static"][0]) == list(g["tabs"])
        for t, r in zip(g["tabs"], g["rows"]):
            assert got.setdefault(t, r) == r
    return got


@pytest.mark.parametrize("which", [0, 1, 2])
def test_sparse_group_cache_reports_the_current_row_counts(which):
    plan = _three_table_plan()
    tables = [torch.zeros(50, 16), torch.zeros(70, 16), torch.zeros(90, 16)]
    assert _rows_of(ops._sparse_group_cache(plan, tables)) == {0: 50, 1: 70, 2: 90}
    old = tables[which]
    tables[which] = torch.zeros(2 * old.shape[0], 16)            # the same list object, one table grown
    want = {0: 50, 1: 70, 2: 90}
    want[which] = 2 * old.shape[0]
    assert _rows_of(ops._sparse_group_cache(plan, tables)) == want
    tables[which] = old                                          # ... and shrunk again
    assert _rows_of(ops._sparse_group_cache(plan, tables)) == {0: 50, 1: 70, 2: 90}


def test_sparse_group_cache_keeps_its_groups_while_the_row_counts_stay():
    """A table swapped for another of the same shape changes nothing the groups hold (no address is cached): the policies and their recorded
    statistics survive, as they do from step to step."""
    plan = _three_table_plan()
    tables = [torch.zeros(50, 16), torch.zeros(70, 16), torch.zeros(90, 16)]
    first = ops._sparse_group_cache(plan, tables)
    assert ops._sparse_group_cache(plan, tables) is first
    tables[1] = torch.ones(70, 16)
    assert ops._sparse_group_cache(plan, tables) is first
    assert ops._sparse_group_cache(plan, tuple(tables)) is first          # the backward passes the node's tuple


@pytest.mark.parametrize("cfg,name", [("cf_deep_small.yaml", "subcategory"), ("cf_array_small.yaml", "item_id"),
                                       ("cf_array_small.yaml", "user_click_cats")])
def test_model_hands_the_replaced_parameter_to_the_launch(cfg, name, monkeypatch):
    """BaseModel._embed caches its table list per feature set.  With the launch itself replaced by a recorder (no GPU here): after the
    Parameter of a table that is neither first nor last is replaced, the next call passes the NEW Parameter, and the others unchanged."""
    from news_recsys_amd.model.sort.deep.model import Deep
    m = Deep(os.path.join(CONFIGS, cfg))
    names = m.user_feature_names | m.item_feature_names
    B = 4
    batch = {}
    for n in sorted(names):
        if n in m.array_feature_names:
            L = m.array_max_length[n]
            batch[n] = torch.ones(B, L, dtype=torch.int64)
            batch[f"{n}_mask"] = torch.ones(B, L)
        else:
            batch[n] = torch.ones(B, dtype=torch.int64)
    seen = []

    def record(plan, tables, inputs, weights, **kw):
        seen.append((plan, list(tables)))
        return torch.zeros(B, plan.out_width), None, None

    monkeypatch.setattr(ops, "embed_apply", record)
    m.get_embeddings_from_batch(batch, names)
    plan, before = seen[-1]
    table_names = []
    for s in plan.slots:
        tn = m._get_emb_feature_name(s.name)
        if tn not in table_names:
            table_names.append(tn)
    k = table_names.index(name)
    assert 0 < k < len(before) - 1, (k, table_names)
    assert all(t is m.embedding_tables[tn].weight for t, tn in zip(before, table_names))
    new = torch.nn.Parameter(torch.randn_like(before[k]))
    m.embedding_tables[name].weight = new
    m.get_embeddings_from_batch(batch, names)
    plan2, after = seen[-1]
    assert plan2 is plan
    assert after[k] is new
    assert all(a is b for i, (a, b) in enumerate(zip(after, before)) if i != k)
    # a replaced module (what sharding does) is followed too
    emb = torch.nn.Embedding(before[k].shape[0], before[k].shape[1], padding_idx=0)
    m.embedding_tables[name] = emb
    m.get_embeddings_from_batch(batch, names)
    assert seen[-1][1][k] is emb.weight
