"""CPU-only: the four per-symbol Laplace / Cauchy entry points (cst_{ans,range}_{encode,decode}_family_batch) exist at every
layer, and they judge their arguments before they touch the device -- so their argument checks run here, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
ENTRY_POINTS = ["cst_ans_encode_family_batch", "cst_ans_decode_family_batch", "cst_range_encode_family_batch", "cst_range_decode_family_batch"]


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"cst_status\s+%s\s*\(\s*cst_coder_config\s+cfg\s*,\s*int32_t\s+family\s*," % name, text)
        assert m, f"{name}: not declared with `family` after `cfg`"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def _call(lib, name, family=None, lo=-100, hi=100, null=()):
    """one call with n_streams = 1, n_per_stream = 4 and HOST buffers behind every pointer: a call that passed its argument
    checks would go on to the device, so only calls that must fail them are made"""
    from constriction_amd import _native as N
    family = N.FAMILY_LAPLACE if family is None else family
    buf = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "a", "b", "words", "n_words", "state", "status", "n_words_out")}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    cfg = N.CoderConfig(32, 64, 24)
    if name == "cst_ans_encode_family_batch" or name == "cst_range_encode_family_batch":
        return getattr(lib, name)(cfg, family, lo, hi, p["symbols"], p["a"], p["b"], 1, 4, N.LAYOUT_STREAM_MAJOR, p["words"], 16, p["n_words"],
                                  p["state"], p["status"], N.FLAG_NONE, None)
    if name == "cst_ans_decode_family_batch":
        return lib.cst_ans_decode_family_batch(cfg, family, lo, hi, p["words"], None, 16, 16, p["n_words"], p["a"], p["b"], p["symbols"], 1, 4,
                                               N.LAYOUT_STREAM_MAJOR, p["state"], p["n_words_out"], p["status"], N.FLAG_NONE, None)
    return lib.cst_range_decode_family_batch(cfg, family, lo, hi, p["words"], None, 16, 16, p["n_words"], p["a"], p["b"], p["symbols"], 1, 4,
                                             N.LAYOUT_STREAM_MAJOR, p["state"], p["status"], N.FLAG_NONE, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    assert _call(lib, name, family=N.FAMILY_BINOMIAL) == bad
    assert _call(lib, name, family=0) == bad
    assert _call(lib, name, null=("symbols",)) == bad
    assert _call(lib, name, null=("words",)) == bad
    assert _call(lib, name, lo=5, hi=5) == bad
    assert _call(lib, name, lo=5, hi=4) == bad
    for other in ("a", "b", "n_words", "status"):
        assert _call(lib, name, null=(other,)) == bad
    assert _call(lib, name, family=N.FAMILY_CAUCHY, null=("status",)) == bad


def test_batched_exposes_the_named_functions():
    pytest.importorskip("torch")
    from constriction_amd import batched
    for coder in ("ans", "range"):
        for direction in ("encode", "decode"):
            assert callable(getattr(batched, f"{coder}_{direction}_family"))
            for family in ("laplace", "cauchy"):
                fn = getattr(batched, f"{coder}_{direction}_{family}")
                assert callable(fn) and fn.__name__ == f"{coder}_{direction}_{family}"
