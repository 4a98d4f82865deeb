"""CPU checks of the pairwise dot-product interaction's entry points (nrx_dot_interact_fwd / _bwd, include/nrx_embed.h): every
NRX_ERR_BAD_ARG / NRX_ERR_UNSUPPORTED refusal through ctypes -- decided before any launch, no GPU is touched: the device pointers are never
followed --, the empty batch, the symbols in header, library and binding, the ops' own refusals, and the host half of both entry points under
ASan + UBSan (a stand-alone driver with its own main)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from news_recsys_amd import _lib, ops
from tests.conftest import ROOT

P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"
OK = dict(x=P, ld=48, off=(0, 16, 32), dim=16, batch=3, flags=0, z=P + 0x8000, z_ld=3, g_z=P + 0x8000, gz_ld=3, g_x=P + 0x4000, gx_ld=48, accumulate=0)


def _off(offs, n=None):
    return None if offs is None else (ctypes.c_int32 * len(offs))(*offs)


def _fwd(**kw):
    a = dict(OK, **kw)
    n = a.get("n_fields", 0 if a["off"] is None else len(a["off"]))
    return _lib.load().nrx_dot_interact_fwd(a["x"], a["ld"], _off(a["off"]), n, a["dim"], a["batch"], a["flags"], a["z"], a["z_ld"], None)


def _bwd(**kw):
    a = dict(OK, **kw)
    n = a.get("n_fields", 0 if a["off"] is None else len(a["off"]))
    return _lib.load().nrx_dot_interact_bwd(a["x"], a["ld"], _off(a["off"]), n, a["dim"], a["batch"], a["flags"], a["g_z"], a["gz_ld"], a["g_x"],
                                            a["gx_ld"], a["accumulate"], None)


# (arguments, the word nrx_last_error() must hold)
BAD_BOTH = [(dict(x=None), "null buffer"), (dict(x=P + 4), "misaligned x"), (dict(x=P + 8), "misaligned x"),
            (dict(off=None, n_fields=3), "field_off"), (dict(off=(), n_fields=0), "n_fields"), (dict(n_fields=-1), "n_fields"),
            (dict(dim=0), "dim"), (dict(dim=-4), "dim"), (dict(batch=-1), "batch"), (dict(flags=2), "flags"), (dict(flags=3), "flags"),
            (dict(ld=46), "ld"), (dict(ld=12), "ld"), (dict(ld=44), "field_off[2]"),
            (dict(off=(0, 18, 32)), "field_off[1]"), (dict(off=(0, -16, 32), ld=64), "field_off[1]"), (dict(off=(0, 16, 36)), "field_off[2]"),
            (dict(off=(0, 16, 28)), "overlap"), (dict(off=(0, 16, 16)), "overlap"), (dict(off=(32, 0, 20)), "overlap")]
BAD_FWD = [(dict(z=None), "null buffer"), (dict(z=P + 0x8002), "misaligned z"), (dict(z_ld=2), "z_ld"), (dict(flags=1, z_ld=5), "z_ld"),
           (dict(ld=52, z=P + 4 * 44, z_ld=52), "overlaps field"), (dict(ld=52, z=P + 4 * 50, z_ld=52), "leaves")]
BAD_BWD = [(dict(g_z=None), "null buffer"), (dict(g_x=None), "null buffer"), (dict(g_z=P + 0x8001), "misaligned g_z"), (dict(g_x=P + 0x4002), "misaligned g_x"),
           (dict(gz_ld=2), "gz_ld"), (dict(flags=1, gz_ld=5), "gz_ld"), (dict(gx_ld=47), "gx_ld"), (dict(accumulate=2), "accumulate"),
           (dict(accumulate=-1), "accumulate"), (dict(g_z=P + 0x4000 + 4 * 40, gz_ld=52, gx_ld=52, accumulate=1), "overlaps field")]
UNSUPPORTED = [dict(off=(0,), z_ld=0, gz_ld=0), dict(off=tuple(4 * i for i in range(65)), dim=4, ld=260, z_ld=2080, gz_ld=2080, gx_ld=260),
               dict(off=(0, 8), dim=6, ld=16, z_ld=1, gz_ld=1, gx_ld=16), dict(off=(0, 4), dim=2, ld=8, z_ld=1, gz_ld=1, gx_ld=8),
               dict(off=(0, 68), dim=68, ld=136, z_ld=1, gz_ld=1, gx_ld=136)]


@pytest.mark.parametrize("kw, word", BAD_BOTH + BAD_FWD, ids=str)
def test_fwd_bad_arguments(kw, word):
    assert _fwd(**kw) == _lib.NRX_ERR_BAD_ARG
    err = _lib.load().nrx_last_error()
    assert b"nrx_dot_interact_fwd" in err and word.encode() in err, err


@pytest.mark.parametrize("kw, word", BAD_BOTH + BAD_BWD, ids=str)
def test_bwd_bad_arguments(kw, word):
    assert _bwd(**kw) == _lib.NRX_ERR_BAD_ARG
    err = _lib.load().nrx_last_error()
    assert b"nrx_dot_interact_bwd" in err and word.encode() in err, err


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=str)
def test_unsupported_shapes(kw):
    assert _fwd(**kw) == _lib.NRX_ERR_UNSUPPORTED and b"supports" in _lib.load().nrx_last_error()
    assert _bwd(**kw) == _lib.NRX_ERR_UNSUPPORTED and b"nrx_dot_interact_bwd" in _lib.load().nrx_last_error()
    with pytest.raises(_lib.NrxError):
        _lib.check(_fwd(**kw), "nrx_dot_interact_fwd")
    n, d = len(kw["off"]), kw.get("dim", 16)
    assert not ops.dot_interaction_supported(n, d)


def test_a_bad_argument_wins_over_an_unsupported_shape():
    assert _fwd(off=(0,), z=None, z_ld=0) == _lib.NRX_ERR_BAD_ARG
    assert _bwd(off=(0, 8), dim=6, ld=16, gz_ld=1, gx_ld=12) == _lib.NRX_ERR_BAD_ARG


def test_empty_batch_is_ok_and_touches_nothing():
    none = dict(batch=0, x=None, z=None, g_z=None, g_x=None)
    assert _fwd(**none) == _lib.NRX_OK and _bwd(**none) == _lib.NRX_OK
    assert _fwd(**dict(none, flags=1, z_ld=6)) == _lib.NRX_OK and _bwd(**dict(none, flags=1, gz_ld=6, accumulate=1)) == _lib.NRX_OK
    assert _fwd(**dict(none, z_ld=2)) == _lib.NRX_ERR_BAD_ARG          # ... but its shape is still checked
    assert _lib.load().nrx_abi_version() == 3                          # the additions are additive


def test_symbols_in_header_library_and_binding():
    txt = open(os.path.join(ROOT, "include", "nrx_embed.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nrx_dot_interact_fwd", "nrx_dot_interact_bwd"):
        assert re.search(r"^NRX_API\s+int\s+%s\s*\(" % name, txt, flags=re.M)
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nrx_dot_interact_fwd"][1]) == 10 and len(_lib.SIGNATURES["nrx_dot_interact_bwd"][1]) == 13
    assert re.search(r"^#define NRX_DOT_SELF 1\b", txt, flags=re.M) and _lib.NRX_DOT_SELF == 1


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    x = torch.zeros(2, 48)
    with pytest.raises(_lib.NrxError):
        ops.dot_interaction(x, 3, 16)
    with pytest.raises(_lib.NrxError):
        ops.dot_interaction_cat_(torch.zeros(2, 52), 48, 3, 16)
    assert isinstance(ops.dot_interaction_calls, int)
    with pytest.raises(ValueError, match="names no field"):
        ops.dot_interaction_math(x, [], 16)


# ---- the host half of the entry points under ASan + UBSan: a stand-alone driver with its own main, run directly
def test_dot_interact_host_validation_is_clean_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    if not os.path.exists(os.path.join(ROOT, "tests", "sanitize", "dot_interact.mk")):
        pytest.skip("tests/sanitize/ is not part of this tree (it does not travel to the GPU machines)")
    p = subprocess.run(["make", "-C", "tests/sanitize", "-f", "dot_interact.mk", "run"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert "nrx_dot_interact validation sanitize driver: OK" in out
