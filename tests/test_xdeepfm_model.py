"""CPU checks of the xDeepFM ranker (news_recsys_amd/model/sort/xdeepfm): the xdeepfm_cfg block, its defaults and its
constructor-time errors, the state_dict, the widths, the sharding refusals, and the C entry points of the CIN rejecting bad arguments before any
launch.  No GPU is touched."""
import copy
import ctypes
import os

import pytest
import torch
import yaml

from news_recsys_amd import _lib, ops
from news_recsys_amd.model.sort.xdeepfm.model import xDeepFM
from tests.conftest import CONFIGS

CFG = os.path.join(CONFIGS, "cf_xdeepfm_small.yaml")


def _variant(tmp_path, edit):
    """Path of a copy of cf_xdeepfm_small.yaml after edit(cfg dict)."""
    with open(CFG) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    edit(cfg)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_xdeepfm_cfg_is_parsed():
    m = xDeepFM(CFG)
    assert m.xdeepfm_cfg == dict(cin_feature_names=["category", "item_id", "user_history", "user_id"], cin_layer_sizes=[6, 5])
    assert m.cin_dim == 16 and ops.cin_out_width(m.xdeepfm_cfg["cin_layer_sizes"]) == 11


def test_xdeepfm_cfg_defaults(tmp_path):
    """Without the block: every sparse / array feature of the model (the dense view_rate stays out), layers [32, 32] -- once subcat shares the dim."""
    def edit(c):
        c.pop("xdeepfm_cfg")
        c["embeddings"]["embedding_size"]["subcat"] = 16
    m = xDeepFM(_variant(tmp_path, edit))
    assert m.xdeepfm_cfg == dict(cin_feature_names=["category", "item_id", "subcat", "user_history", "user_id"], cin_layer_sizes=[32, 32])
    assert [tuple(w.shape) for w in m.cin.weights] == [(32, 5, 5), (32, 32, 5)] and m.cin_out.weight.shape == (1, 64)


def test_example_config_of_the_package_loads():
    import news_recsys_amd.model.sort.xdeepfm as pkg
    path = os.path.join(os.path.dirname(pkg.__file__), "train_cf_xdeepfm.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    assert cfg["xdeepfm_cfg"] == dict(cin_feature_names=["user_id", "item_id", "user_history"], cin_layer_sizes=[32, 32])
    assert "pnn_cfg" not in cfg and "din_cfg" not in cfg
    m = xDeepFM(path)
    assert m.cin_dim == 32 and [tuple(w.shape) for w in m.cin.weights] == [(32, 3, 3), (32, 32, 3)]


@pytest.mark.parametrize("edit", [
    lambda c: c["xdeepfm_cfg"].update(cin_feature_names=["user_id", "nope"]),                 # not a feature of the model
    lambda c: c["xdeepfm_cfg"].update(cin_feature_names=["user_id", "view_rate"]),            # dense
    lambda c: c["xdeepfm_cfg"].update(cin_feature_names=["user_id"]),                         # fewer than 2 fields
    lambda c: c["xdeepfm_cfg"].update(cin_feature_names=[]),
    lambda c: c["xdeepfm_cfg"].update(cin_feature_names=["user_id", "subcat"]),               # dims 16 and 8
    lambda c: c.pop("xdeepfm_cfg"),                                                           # the default takes subcat (dim 8) in
], ids=["unknown", "dense", "one", "none", "dims", "default-dims"])
def test_field_errors_name_the_key(tmp_path, edit):
    with pytest.raises(ValueError, match=r"xdeepfm_cfg\.cin_feature_names"):
        xDeepFM(_variant(tmp_path, edit))


def test_a_feature_without_a_table_is_refused(tmp_path):
    def edit(c):
        c["features"]["sparse_feature_names"].append("brand")
        c["features"]["item_feature_names"].append("brand")
        c["xdeepfm_cfg"]["cin_feature_names"].append("brand")
    try:
        xDeepFM(_variant(tmp_path, edit))
    except ValueError as e:
        assert "xdeepfm_cfg.cin_feature_names" in str(e) and "no embedding table" in str(e)
    except KeyError:
        pass          # (the base model refuses a sparse feature without embedding sizes before the block is read)
    else:
        raise AssertionError("a CIN field without an embedding table was accepted")


@pytest.mark.parametrize("sizes", [[], [4, 0], [4, -1], [2.5], "32", [True]], ids=["empty", "zero", "negative", "float", "str", "bool"])
def test_layer_size_errors_name_the_key(tmp_path, sizes):
    with pytest.raises(ValueError, match=r"xdeepfm_cfg\.cin_layer_sizes"):
        xDeepFM(_variant(tmp_path, lambda c: c["xdeepfm_cfg"].update(cin_layer_sizes=sizes)))


def test_dim_mismatch_message_lists_the_dims(tmp_path):
    with pytest.raises(ValueError, match=r"'subcat': 8.*'user_id': 16"):
        xDeepFM(_variant(tmp_path, lambda c: c["xdeepfm_cfg"].update(cin_feature_names=["user_id", "subcat"])))


def test_state_dict_keys_shapes_and_widths():
    torch.manual_seed(3)
    m = xDeepFM(CFG)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    mine = {k: v for k, v in sd.items() if not (k.startswith("embedding_tables.") or k.startswith("score_fc."))}
    assert mine == {"bias": (1,), "cin.weights.0": (6, 4, 4), "cin.weights.1": (5, 6, 4), "cin_out.weight": (1, 11)}
    # the MLP reads the concat alone: user 16 + 16 + 1, item 16 + 16 + 8 -- Deep's head, unchanged
    assert m.user_input_dim + m.item_input_dim == 73
    from news_recsys_amd.model.sort.deep.model import Deep
    d = {k: tuple(v.shape) for k, v in Deep(CFG).state_dict().items()}
    assert {k: v for k, v in sd.items() if k not in mine} == d
    # the CIN weights: uniform in +-sqrt(3 / fan_in), fan_in = H_(k-1) m; from torch's generator (the same seed, the same model)
    for w, fan in zip(m.cin.weights, (16, 24)):
        a = (3.0 / fan) ** 0.5
        assert 0.5 * a < float(w.detach().abs().max()) <= a
    torch.manual_seed(3)
    again = xDeepFM(CFG)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in m.state_dict().items())
    assert float(m.bias.detach()) == 0.0


def test_sharding_refusals_name_xdeepfm_cfg():
    from news_recsys_amd.shard_step import shard_model_step_
    from news_recsys_amd.sharding import shard_model_
    m = xDeepFM(CFG)
    with pytest.raises(NotImplementedError, match="xdeepfm_cfg.*does not know that operator"):
        shard_model_(m, 0, 2)
    with pytest.raises(NotImplementedError, match="xdeepfm_cfg.*does not know that operator"):
        shard_model_step_(m, 0, 2)


def test_forward_on_cpu_raises_like_every_model():
    m = xDeepFM(CFG)
    batch = dict(user_id=torch.ones(2, dtype=torch.long), item_id=torch.ones(2, dtype=torch.long), category=torch.ones(2, dtype=torch.long),
                 subcat=torch.ones(2, dtype=torch.long), view_rate=torch.ones(2), user_history=torch.ones(2, 7, dtype=torch.long),
                 user_history_mask=torch.ones(2, 7))
    with pytest.raises(_lib.NrxError):
        m(batch)


# ------------------------------------------------------------------------------------------------- the C entry points, without a GPU
def _fwd(lib, **kw):
    a = dict(x0=64, x0_ld=16, off=[0, 4, 8], m=3, dim=4, xprev=None, xprev_ld=0, Hp=3, W=64, H=2, batch=2, xk=64, xk_ld=8, p=64, p_ld=2)
    a.update(kw)
    off = None if a["off"] is None else (ctypes.c_int32 * len(a["off"]))(*a["off"])
    return lib.nrx_cin_layer_fwd(a["x0"], a["x0_ld"], off, a["m"], a["dim"], a["xprev"], a["xprev_ld"], a["Hp"], a["W"], a["H"], a["batch"], a["xk"],
                                 a["xk_ld"], a["p"], a["p_ld"], None)


def _bwd(lib, **kw):
    a = dict(x0=64, x0_ld=16, off=[0, 4, 8], m=3, dim=4, xprev=None, xprev_ld=0, Hp=3, W=64, H=2, batch=2, g_p=64, gp_ld=2, g_xk=64, gxk_ld=8,
             g_xprev=None, gxprev_ld=0, g_x0=64, gx0_ld=16, acc=0, g_W=64, ws=64)
    a.update(kw)
    off = None if a["off"] is None else (ctypes.c_int32 * len(a["off"]))(*a["off"])
    return lib.nrx_cin_layer_bwd(a["x0"], a["x0_ld"], off, a["m"], a["dim"], a["xprev"], a["xprev_ld"], a["Hp"], a["W"], a["H"], a["batch"], a["g_p"],
                                 a["gp_ld"], a["g_xk"], a["gxk_ld"], a["g_xprev"], a["gxprev_ld"], a["g_x0"], a["gx0_ld"], a["acc"], a["g_W"], a["ws"],
                                 None)


@pytest.mark.parametrize("kw, says", [
    (dict(x0=None), b"null buffer (x0 or W)"), (dict(W=None), b"null buffer (x0 or W)"), (dict(p=None), b"null buffer (p)"), (dict(off=None), b"null field_off"),
    (dict(x0=68), b"misaligned x0"), (dict(xk=68), b"misaligned xk"), (dict(p=66), b"misaligned p"), (dict(W=66), b"misaligned W"),
    (dict(x0_ld=3), b"x0_ld"), (dict(x0_ld=18), b"x0_ld"), (dict(xk_ld=4), b"xk row stride"), (dict(p_ld=1), b"p row stride"),
    (dict(off=[0, 4, 14]), b"field_off[2]"), (dict(off=[0, 2, 8]), b"misaligned field"), (dict(off=[0, 4, 4]), b"overlap"),
    (dict(Hp=2), b"xprev is null"), (dict(xprev=64, xprev_ld=8), b"xprev_ld"), (dict(xprev=68, xprev_ld=12), b"misaligned xprev"),
    (dict(m=0), b"bad argument (m 0"), (dict(H=0), b"H 0"), (dict(batch=-1), b"batch -1"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_the_forward_entry_point_rejects_bad_arguments_without_a_gpu(kw, says):
    lib = _lib.load()
    assert _fwd(lib, **kw) == _lib.NRX_ERR_BAD_ARG
    msg = lib.nrx_last_error()
    assert msg.startswith(b"nrx_cin_layer_fwd:") and says in msg, msg


@pytest.mark.parametrize("kw, says", [
    (dict(g_p=None), b"null buffer (g_p"), (dict(g_x0=None), b"null buffer (g_p"), (dict(g_W=None), b"null buffer (g_p"), (dict(ws=None), b"null buffer (g_p"),
    (dict(acc=2), b"accumulate_x0 2"), (dict(g_xprev=64, gxprev_ld=12), b"g_xprev must be null exactly when xprev is"),
    (dict(xprev=64, xprev_ld=12), b"g_xprev must be null exactly when xprev is"), (dict(gp_ld=1), b"g_p row stride"), (dict(gxk_ld=6), b"g_xk row stride"),
    (dict(g_xk=72), b"misaligned g_xk"), (dict(gx0_ld=8), b"gx0_ld 8 does not hold field 2"), (dict(gx0_ld=14), b"g_x0 row stride"),
    (dict(g_x0=68), b"misaligned g_x0"), (dict(g_W=66), b"misaligned g_W or workspace"), (dict(xprev=64, xprev_ld=12, g_xprev=64, gxprev_ld=8), b"g_xprev row stride"),
    (dict(off=[0, 4, 4]), b"overlap"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_the_backward_entry_point_rejects_bad_arguments_without_a_gpu(kw, says):
    lib = _lib.load()
    assert _bwd(lib, **kw) == _lib.NRX_ERR_BAD_ARG
    msg = lib.nrx_last_error()
    assert msg.startswith(b"nrx_cin_layer_bwd:") and says in msg, msg


def test_unsupported_shapes_and_empty_batches_launch_nothing_without_a_gpu():
    lib = _lib.load()
    assert _fwd(lib, H=65, xk_ld=260, p_ld=65) == _lib.NRX_ERR_UNSUPPORTED and b"supports m 2..64" in lib.nrx_last_error()
    assert _fwd(lib, off=[0], m=1, Hp=1) == _lib.NRX_ERR_UNSUPPORTED
    assert _bwd(lib, H=65, gp_ld=65, gxk_ld=260) == _lib.NRX_ERR_UNSUPPORTED
    assert _fwd(lib, batch=0, x0=None, W=None, p=None, xk=None) == _lib.NRX_OK and _bwd(lib, batch=0, g_p=None, g_x0=None, g_W=None, ws=None) == _lib.NRX_OK
    assert [lib.nrx_cin_supported(*s) for s in ((2, 1, 1, 4), (64, 64, 64, 64), (1, 1, 1, 4), (65, 1, 1, 4), (2, 65, 1, 4), (2, 1, 65, 4), (2, 1, 1, 6), (2, 1, 1, 68))] \
        == [1, 1, 0, 0, 0, 0, 0, 0]
    assert all(bool(lib.nrx_cin_supported(m, Hp, H, D)) == ops.cin_supported(m, Hp, H, D)
               for m in (1, 2, 64, 65) for Hp in (0, 1, 64, 65) for H in (0, 1, 64, 65) for D in (0, 2, 4, 12, 64, 68))
    sl = lib.nrx_cin_wgrad_slice(16)
    assert sl >= 1 and lib.nrx_cin_layer_bwd_workspace(sl, 3, 5, 2, 16) == 4 * 2 * 5 * 3 and lib.nrx_cin_layer_bwd_workspace(sl + 1, 3, 5, 2, 16) == 2 * 4 * 2 * 5 * 3
