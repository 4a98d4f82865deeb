"""CPU checks of the DIN ranker (news_recsys_amd/model/sort/din): the din_cfg block and its constructor-time errors, the
state_dict, the MLP's input width, the sharding refusals -- and every NRX_ERR_BAD_ARG / NRX_ERR_UNSUPPORTED refusal of nrx_din_pool_fwd /
nrx_din_pool_bwd, which are decided before any launch (no GPU is touched: the pointers are never followed)."""
import copy
import os

import pytest
import torch
import yaml

from news_recsys_amd import _lib
from news_recsys_amd.model.sort.din.model import DIN
from tests.conftest import CONFIGS

CFG = os.path.join(CONFIGS, "cf_din_small.yaml")


def _variant(tmp_path, edit):
    """Path of a copy of cf_din_small.yaml after edit(cfg dict)."""
    with open(CFG) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    edit(cfg)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_din_cfg_is_parsed():
    m = DIN(CFG)
    assert m.din_cfg == dict(history_feature_names=["user_history"], query_feature="item_id", scale=None)
    assert m._din_other == frozenset({"user_id", "user_click_cats", "item_id", "category"})


def test_din_cfg_defaults(tmp_path):
    """Without the block: the array features whose table a single-valued feature owns (user_history -> item_id; user_click_cats has its own
    table and stays on the mean pool), the query that owner."""
    m = DIN(_variant(tmp_path, lambda c: c.pop("din_cfg")))
    assert m.din_cfg == dict(history_feature_names=["user_history"], query_feature="item_id", scale=None)
    m = DIN(_variant(tmp_path, lambda c: c["din_cfg"].update(scale=0.25, query_feature=None)))
    assert m.din_cfg["scale"] == 0.25 and m.din_cfg["query_feature"] == "item_id"


def test_example_config_of_the_package_loads():
    import news_recsys_amd.model.sort.din as pkg
    with open(os.path.join(os.path.dirname(pkg.__file__), "train_cf_din.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["din_cfg"]["history_feature_names"] == ["user_history"] and cfg["din_cfg"]["query_feature"] == "item_id"
    assert cfg["embeddings"]["share_emb_table_features"] == {"user_history": "item_id"}


@pytest.mark.parametrize("edit, key", [
    (lambda c: c["din_cfg"].update(history_feature_names=["category"]), "din_cfg.history_feature_names"),         # not an array feature
    (lambda c: c["din_cfg"].update(history_feature_names=["nope"]), "din_cfg.history_feature_names"),
    (lambda c: c["din_cfg"].update(history_feature_names=[]), "din_cfg.history_feature_names"),
    (lambda c: c["din_cfg"].update(query_feature="user_click_cats"), "din_cfg.query_feature"),                    # not single-valued
    (lambda c: c["din_cfg"].update(query_feature="ctr"), "din_cfg.query_feature"),                                # dense
    (lambda c: c["din_cfg"].update(query_feature="nope"), "din_cfg.query_feature"),
    (lambda c: c["din_cfg"].update(query_feature="user_id"), "din_cfg"),                                          # dims 16 vs 32
    (lambda c: c["din_cfg"].update(history_feature_names=["user_click_cats"]), "din_cfg"),                        # dims 12 vs 32
    (lambda c: c["din_cfg"].update(history_feature_names=["user_click_cats"], query_feature=None), "din_cfg.query_feature"),   # no owner
])
def test_constructor_errors_name_the_key(tmp_path, edit, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        DIN(_variant(tmp_path, edit))


def test_dim_mismatch_message_names_both_features(tmp_path):
    with pytest.raises(ValueError, match=r"'user_id' has dim 16 .* 'user_history' has dim 32"):
        DIN(_variant(tmp_path, lambda c: c["din_cfg"].update(query_feature="user_id")))


def test_state_dict_keys_shapes_and_input_width():
    m = DIN(CFG)
    sd = m.state_dict()
    assert all(k.startswith("embedding_tables.") or k.startswith("score_fc.") for k in sd)
    tables = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("embedding_tables.")}
    assert tables == {"embedding_tables.category.weight": (18, 8), "embedding_tables.item_id.weight": (41, 32),
                      "embedding_tables.user_click_cats.weight": (18, 12), "embedding_tables.user_id.weight": (53, 16)}
    # the MLP reads cat([concat of the other features, pooled histories]): user 16 + 32 + 12, item 32 + 8
    assert m.user_input_dim + m.item_input_dim == 100
    first = m.score_fc.network.network[0]
    assert first.weight.shape == (128, 100)
    # no parameters beyond Deep's
    from news_recsys_amd.model.sort.deep.model import Deep
    d = Deep(os.path.join(CONFIGS, "cf_array_small.yaml"))
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_sharding_refusals_name_din_cfg():
    from news_recsys_amd.shard_step import shard_model_step_
    from news_recsys_amd.sharding import shard_model_
    m = DIN(CFG)
    with pytest.raises(NotImplementedError, match="din_cfg"):
        shard_model_(m, 0, 2)
    with pytest.raises(NotImplementedError, match="din_cfg"):
        shard_model_step_(m, 0, 2)


def test_forward_on_cpu_raises_like_every_model():
    m = DIN(CFG)
    batch = dict(user_id=torch.ones(2, dtype=torch.long), item_id=torch.ones(2, dtype=torch.long), category=torch.ones(2, dtype=torch.long),
                 user_click_cats=torch.ones(2, 5, dtype=torch.long), user_click_cats_mask=torch.ones(2, 5),
                 user_history=torch.ones(2, 7, dtype=torch.long), user_history_mask=torch.ones(2, 7))
    with pytest.raises(_lib.NrxError):
        m(batch)


# ---------------------------------------------------------------- the two entry points' refusals (decided before any launch)
P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"
OK = dict(table=P, rows=97, dim=16, flags=0, ids=P, index_bits=64, mask=None, query=P, q_ld=16, batch=3, bag_len=50, scale=0.25, out=P, out_ld=16,
          lse=P, status=None, g_out=P, g_out_ld=16, g_query=P, g_query_ld=16, g_rows=P)


def _fwd(**kw):
    a = dict(OK, **kw)
    return _lib.load().nrx_din_pool_fwd(a["table"], a["rows"], a["dim"], a["flags"], a["ids"], a["index_bits"], a["mask"], a["query"], a["q_ld"],
                                        a["batch"], a["bag_len"], a["scale"], a["out"], a["out_ld"], a["lse"], a["status"], None)


def _bwd(**kw):
    a = dict(OK, **kw)
    return _lib.load().nrx_din_pool_bwd(a["table"], a["rows"], a["dim"], a["flags"], a["ids"], a["index_bits"], a["mask"], a["query"], a["q_ld"],
                                        a["batch"], a["bag_len"], a["scale"], a["out"], a["out_ld"], a["lse"], a["g_out"], a["g_out_ld"],
                                        a["g_query"], a["g_query_ld"], a["g_rows"], None)


BAD_BOTH = [dict(table=None), dict(ids=None), dict(query=None), dict(out=None), dict(lse=None),
            dict(table=P + 4), dict(table=P + 4, flags=1), dict(query=P + 8), dict(out=P + 4), dict(ids=P + 4), dict(ids=P + 2, index_bits=32),
            dict(mask=P + 2), dict(lse=P + 1), dict(q_ld=18), dict(out_ld=18), dict(q_ld=12), dict(out_ld=12),
            dict(scale=float("inf")), dict(scale=float("nan")), dict(index_bits=16), dict(index_bits=0), dict(flags=2),
            dict(batch=-1), dict(bag_len=0), dict(dim=0), dict(rows=0)]
BAD_FWD = [dict(status=P + 2)]
BAD_BWD = [dict(g_out=None), dict(g_query=None), dict(g_rows=None), dict(g_out=P + 4), dict(g_query=P + 8), dict(g_rows=P + 4),
           dict(g_out_ld=18), dict(g_query_ld=18), dict(g_out_ld=12), dict(g_query_ld=12)]
UNSUPPORTED = [dict(dim=68, q_ld=68, out_ld=68, g_out_ld=68, g_query_ld=68), dict(dim=6, q_ld=8, out_ld=8, g_out_ld=8, g_query_ld=8),
               dict(dim=2, q_ld=4, out_ld=4, g_out_ld=4, g_query_ld=4), dict(bag_len=257), dict(rows=(1 << 30) + 1)]


@pytest.mark.parametrize("kw", BAD_BOTH + BAD_FWD, ids=str)
def test_fwd_bad_arguments(kw):
    assert _fwd(**kw) == _lib.NRX_ERR_BAD_ARG
    assert b"nrx_din_pool_fwd" in _lib.load().nrx_last_error()


@pytest.mark.parametrize("kw", BAD_BOTH + BAD_BWD, ids=str)
def test_bwd_bad_arguments(kw):
    assert _bwd(**kw) == _lib.NRX_ERR_BAD_ARG
    assert b"nrx_din_pool_bwd" in _lib.load().nrx_last_error()


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=str)
def test_unsupported_shapes(kw):
    assert _fwd(**kw) == _lib.NRX_ERR_UNSUPPORTED and b"supports" in _lib.load().nrx_last_error()
    assert _bwd(**kw) == _lib.NRX_ERR_UNSUPPORTED
    with pytest.raises(_lib.NrxError):
        _lib.check(_fwd(**kw), "nrx_din_pool_fwd")


def test_empty_batch_is_ok_and_touches_nothing():
    none = dict(batch=0, table=None, ids=None, query=None, out=None, lse=None, g_out=None, g_query=None, g_rows=None)
    assert _fwd(**none) == _lib.NRX_OK and _bwd(**none) == _lib.NRX_OK
    assert _lib.load().nrx_abi_version() == 3          # the additions are additive
