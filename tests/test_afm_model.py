"""CPU checks of the AFM ranker (news_recsys_amd/model/sort/afm): the afm_cfg block, its defaults and its constructor-time
errors, the state_dict with and without use_deep, the widths, the sharding refusals, and the C entry points of the attentional pooling
rejecting bad arguments before any launch.  No GPU is touched."""
import copy
import ctypes
import os

import pytest
import torch
import yaml

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.sort.afm.model import AFM
from tests.conftest import CONFIGS

CFG = os.path.join(CONFIGS, "cf_afm_small.yaml")


def _variant(tmp_path, edit):
    """Path of a copy of cf_afm_small.yaml after edit(cfg dict)."""
    with open(CFG) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    edit(cfg)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_afm_cfg_is_parsed():
    m = AFM(CFG)
    assert m.afm_cfg == dict(afm_feature_names=["category", "item_id", "user_history", "user_id"], attention_factor=5, use_deep=True)
    assert m.afm_dim == 16


def test_afm_cfg_defaults(tmp_path):
    """Without the block: every sparse / array feature of the model (the dense view_rate stays out), 16 attention units, the MLP on -- once
    subcat shares the dim."""
    def edit(c):
        c.pop("afm_cfg")
        c["embeddings"]["embedding_size"]["subcat"] = 16
    m = AFM(_variant(tmp_path, edit))
    assert m.afm_cfg == dict(afm_feature_names=["category", "item_id", "subcat", "user_history", "user_id"], attention_factor=16, use_deep=True)
    assert m.attention.w1.shape == (16, 16) and m.attention.b1.shape == (16,) and m.attention.w2.shape == (16,) and m.afm_out.weight.shape == (1, 16)


def test_example_config_of_the_package_loads():
    import news_recsys_amd.model.sort.afm as pkg
    path = os.path.join(os.path.dirname(pkg.__file__), "train_cf_afm.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    assert cfg["afm_cfg"] == dict(afm_feature_names=["user_id", "item_id", "user_history"], attention_factor=16, use_deep=True)
    assert "xdeepfm_cfg" not in cfg and "pnn_cfg" not in cfg
    m = AFM(path)
    assert m.afm_dim == 32 and m.attention.w1.shape == (16, 32)


@pytest.mark.parametrize("edit", [
    lambda c: c["afm_cfg"].update(afm_feature_names=["user_id", "nope"]),                 # not a feature of the model
    lambda c: c["afm_cfg"].update(afm_feature_names=["user_id", "view_rate"]),            # dense
    lambda c: c["afm_cfg"].update(afm_feature_names=["user_id"]),                         # fewer than 2 fields
    lambda c: c["afm_cfg"].update(afm_feature_names=[]),
    lambda c: c["afm_cfg"].update(afm_feature_names=["user_id", "subcat"]),               # dims 16 and 8
    lambda c: c.pop("afm_cfg"),                                                           # the default takes subcat (dim 8) in
], ids=["unknown", "dense", "one", "none", "dims", "default-dims"])
def test_field_errors_name_the_key(tmp_path, edit):
    with pytest.raises(ValueError, match=r"afm_cfg\.afm_feature_names"):
        AFM(_variant(tmp_path, edit))


def test_a_feature_without_a_table_is_refused(tmp_path):
    def edit(c):
        c["features"]["sparse_feature_names"].append("brand")
        c["features"]["item_feature_names"].append("brand")
        c["afm_cfg"]["afm_feature_names"].append("brand")
    try:
        AFM(_variant(tmp_path, edit))
    except ValueError as e:
        assert "afm_cfg.afm_feature_names" in str(e) and "no embedding table" in str(e)
    except KeyError:
        pass          # (the base model refuses a sparse feature without embedding sizes before the block is read)
    else:
        raise AssertionError("an AFM field without an embedding table was accepted")


@pytest.mark.parametrize("factor", [0, -1, 2.5, "16", True, [16]], ids=["zero", "negative", "float", "str", "bool", "list"])
def test_attention_factor_errors_name_the_key(tmp_path, factor):
    with pytest.raises(ValueError, match=r"afm_cfg\.attention_factor"):
        AFM(_variant(tmp_path, lambda c: c["afm_cfg"].update(attention_factor=factor)))


def test_use_deep_must_be_a_bool(tmp_path):
    with pytest.raises(ValueError, match=r"afm_cfg\.use_deep"):
        AFM(_variant(tmp_path, lambda c: c["afm_cfg"].update(use_deep="yes")))


def test_dim_mismatch_message_lists_the_dims(tmp_path):
    with pytest.raises(ValueError, match=r"'subcat': 8.*'user_id': 16"):
        AFM(_variant(tmp_path, lambda c: c["afm_cfg"].update(afm_feature_names=["user_id", "subcat"])))


def test_state_dict_keys_shapes_and_widths(tmp_path):
    torch.manual_seed(3)
    m = AFM(CFG)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    mine = {k: v for k, v in sd.items() if not (k.startswith("embedding_tables.") or k.startswith("score_fc."))}
    assert mine == {"bias": (1,), "attention.w1": (5, 16), "attention.b1": (5,), "attention.w2": (5,), "afm_out.weight": (1, 16)}
    # the MLP reads the concat alone: user 16 + 16 + 1, item 16 + 16 + 8 -- Deep's head, unchanged
    assert m.user_input_dim + m.item_input_dim == 73
    from news_recsys_amd.model.sort.deep.model import Deep
    d = {k: tuple(v.shape) for k, v in Deep(CFG).state_dict().items()}
    assert {k: v for k, v in sd.items() if k not in mine} == d
    # uniform in +-sqrt(3 / fan_in), fan_in = dim and A; b1 zeros; from torch's generator (the same seed, the same model)
    for w, fan in ((m.attention.w1, 16), (m.attention.w2, 5)):
        a = (3.0 / fan) ** 0.5
        assert 0.5 * a < float(w.detach().abs().max()) <= a
    assert not m.attention.b1.detach().any() and float(m.bias.detach()) == 0.0
    torch.manual_seed(3)
    again = AFM(CFG)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in m.state_dict().items())
    # without the MLP: no score_fc.* at all
    shallow = AFM(_variant(tmp_path, lambda c: c["afm_cfg"].update(use_deep=False)))
    keys = [k for k in shallow.state_dict() if not k.startswith("embedding_tables.")]
    assert sorted(keys) == ["afm_out.weight", "attention.b1", "attention.w1", "attention.w2", "bias"] and not hasattr(shallow, "score_fc")


def test_sharding_refusals_name_afm_cfg():
    from news_recsys_amd.shard_step import shard_model_step_
    from news_recsys_amd.sharding import shard_model_
    m = AFM(CFG)
    with pytest.raises(NotImplementedError, match="afm_cfg.*does not know that operator"):
        shard_model_(m, 0, 2)
    with pytest.raises(NotImplementedError, match="afm_cfg.*does not know that operator"):
        shard_model_step_(m, 0, 2)


def test_forward_on_cpu_raises_like_every_model():
    m = AFM(CFG)
    batch = dict(user_id=torch.ones(2, dtype=torch.long), item_id=torch.ones(2, dtype=torch.long), category=torch.ones(2, dtype=torch.long),
                 subcat=torch.ones(2, dtype=torch.long), view_rate=torch.ones(2), user_history=torch.ones(2, 7, dtype=torch.long),
                 user_history_mask=torch.ones(2, 7))
    with pytest.raises(_lib.NrxError):
        m(batch)


# ------------------------------------------------------------------------------------------------- the C entry points, without a GPU
def _off(a):
    return None if a["off"] is None else (ctypes.c_int32 * len(a["off"]))(*a["off"])


def _fwd(lib, **kw):
    a = dict(x=64, ld=16, off=[0, 4, 8], F=3, dim=4, W1=64, b1=64, w2=64, A=2, batch=2, out=64, out_ld=4, lse=64)
    a.update(kw)
    return lib.nrx_afm_fwd(a["x"], a["ld"], _off(a), a["F"], a["dim"], a["W1"], a["b1"], a["w2"], a["A"], a["batch"], a["out"], a["out_ld"], a["lse"], None)


def _bwd(lib, **kw):
    a = dict(x=64, ld=16, off=[0, 4, 8], F=3, dim=4, W1=64, b1=64, w2=64, A=2, batch=2, out=64, out_ld=4, lse=64, g_out=64, go_ld=4, g_x=64, gx_ld=16,
             g_W1=64, g_b1=64, g_w2=64, ws=64)
    a.update(kw)
    return lib.nrx_afm_bwd(a["x"], a["ld"], _off(a), a["F"], a["dim"], a["W1"], a["b1"], a["w2"], a["A"], a["batch"], a["out"], a["out_ld"], a["lse"],
                           a["g_out"], a["go_ld"], a["g_x"], a["gx_ld"], a["g_W1"], a["g_b1"], a["g_w2"], a["ws"], None)


SHARED = [
    (dict(x=None), b"null buffer (x)"), (dict(W1=None), b"null buffer (W1)"), (dict(b1=None), b"null buffer (b1)"), (dict(w2=None), b"null buffer (w2)"),
    (dict(out=None), b"null buffer (out)"), (dict(lse=None), b"null buffer (lse)"), (dict(off=None), b"null field_off"),
    (dict(x=68), b"misaligned x"), (dict(W1=66), b"misaligned W1"), (dict(b1=66), b"misaligned b1"), (dict(w2=66), b"misaligned w2"),
    (dict(out=66), b"misaligned out"), (dict(lse=66), b"misaligned lse"),
    (dict(ld=3), b"ld 3"), (dict(ld=18), b"ld 18"), (dict(out_ld=3), b"out_ld 3"),
    (dict(off=[0, 4, 14]), b"field_off[2]"), (dict(off=[0, 2, 8]), b"misaligned field"), (dict(off=[0, 4, 4]), b"overlap"), (dict(off=[0, -4, 8]), b"field_off[1]"),
    (dict(F=0), b"n_fields 0"), (dict(dim=0), b"dim 0"), (dict(A=0), b"A 0"), (dict(batch=-1), b"batch -1"),
]
_ids = lambda v: None if isinstance(v, bytes) else "-".join(f"{k}{x}" for k, x in v.items())  # noqa: E731


@pytest.mark.parametrize("kw, says", SHARED, ids=_ids)
def test_the_forward_entry_point_rejects_bad_arguments_without_a_gpu(kw, says):
    lib = _lib.load()
    assert _fwd(lib, **kw) == _lib.NRX_ERR_BAD_ARG
    msg = lib.nrx_last_error()
    assert msg.startswith(b"nrx_afm_fwd:") and says in msg, msg


@pytest.mark.parametrize("kw, says", SHARED + [
    (dict(g_out=None), b"null buffer (g_out)"), (dict(g_x=None), b"null buffer (g_x)"), (dict(g_W1=None), b"null buffer (g_W1)"),
    (dict(g_b1=None), b"null buffer (g_b1)"), (dict(g_w2=None), b"null buffer (g_w2)"), (dict(ws=None), b"null buffer (workspace)"),
    (dict(g_out=66), b"misaligned g_out"), (dict(g_x=66), b"misaligned g_x"), (dict(g_W1=66), b"misaligned g_W1"), (dict(g_b1=66), b"misaligned g_b1"),
    (dict(g_w2=66), b"misaligned g_w2"), (dict(ws=66), b"misaligned workspace"),
    (dict(go_ld=3), b"g_out_ld 3"), (dict(gx_ld=8), b"gx_ld 8 does not hold field 2"),
], ids=_ids)
def test_the_backward_entry_point_rejects_bad_arguments_without_a_gpu(kw, says):
    lib = _lib.load()
    assert _bwd(lib, **kw) == _lib.NRX_ERR_BAD_ARG
    msg = lib.nrx_last_error()
    assert msg.startswith(b"nrx_afm_bwd:") and says in msg, msg


def test_unsupported_shapes_and_empty_batches_launch_nothing_without_a_gpu():
    lib = _lib.load()
    assert _fwd(lib, A=65) == _lib.NRX_ERR_UNSUPPORTED and b"supports n_fields 2..64" in lib.nrx_last_error()
    assert _fwd(lib, off=[0], F=1) == _lib.NRX_ERR_UNSUPPORTED
    assert _fwd(lib, dim=6, ld=32, off=[0, 8, 16], out_ld=6) == _lib.NRX_ERR_UNSUPPORTED
    assert _bwd(lib, A=65) == _lib.NRX_ERR_UNSUPPORTED and _bwd(lib, off=[0], F=1) == _lib.NRX_ERR_UNSUPPORTED
    none = dict(x=None, W1=None, b1=None, w2=None, out=None, lse=None)
    assert _fwd(lib, batch=0, **none) == _lib.NRX_OK
    assert _bwd(lib, batch=0, g_out=None, g_x=None, g_W1=None, g_b1=None, g_w2=None, ws=None, **none) == _lib.NRX_OK
    assert [lib.nrx_afm_supported(*s) for s in ((2, 4, 1), (64, 64, 64), (1, 4, 1), (65, 4, 1), (2, 6, 1), (2, 68, 1), (2, 4, 0), (2, 4, 65))] \
        == [1, 1, 0, 0, 0, 0, 0, 0]
    assert all(bool(lib.nrx_afm_supported(F, D, A)) == ops.afm_supported(F, D, A)
               for F in (1, 2, 64, 65) for D in (0, 2, 4, 12, 64, 68) for A in (0, 1, 64, 65))
    # the slice is a function of the shape alone; the workspace holds one partial of A dim + 2 A floats per slice
    sl = lib.nrx_afm_wgrad_slice(26, 16, 16)
    assert sl >= 1 and lib.nrx_afm_bwd_workspace(sl, 26, 16, 5) == 4 * (5 * 16 + 10) and lib.nrx_afm_bwd_workspace(sl + 1, 26, 16, 5) == 2 * 4 * (5 * 16 + 10)
