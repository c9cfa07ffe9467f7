"""CPU-only: the two ragged per-symbol Gaussian entry points (cst_ans_{encode,decode}_gaussian_ragged) exist at every layer, and
they judge their arguments before they touch the device -- so their argument checks run here, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
ENTRY_POINTS = ["cst_ans_encode_gaussian_ragged", "cst_ans_decode_gaussian_ragged"]


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"cst_status\s+%s\s*\(\s*cst_coder_config\s+cfg\s*,\s*int32_t\s+min_symbol\s*,\s*int32_t\s+max_symbol\s*,([^;]*)\)\s*;" % name, text)
        assert m, f"{name}: not declared"
        for arg in ("d_symbols", "d_means", "d_stds", "d_sym_offsets", "n_streams", "d_order", "d_words", "d_word_offsets", "stride_words",
                    "d_n_words", "d_status", "stream"):
            assert re.search(r"\b%s\b" % arg, m.group(1)), f"{name}: no argument {arg}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert "words_capacity" in re.search(r"cst_ans_decode_gaussian_ragged\s*\(([^;]*)\)\s*;", text).group(1)
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def _call(lib, name, cfg=(32, 64, 24), lo=-100, hi=100, null=(), stride=0, n_streams=1):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_streams > 0 would go on to
    the device, so only calls that must fail them (or that have no streams) are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "means", "stds", "sym_offsets", "order", "words", "word_offsets", "n_words", "status")}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    c = N.CoderConfig(*cfg)
    if name == "cst_ans_encode_gaussian_ragged":
        return lib.cst_ans_encode_gaussian_ragged(c, lo, hi, p["symbols"], p["means"], p["stds"], p["sym_offsets"], n_streams, p["order"], p["words"],
                                                  p["word_offsets"], stride, p["n_words"], p["status"], None)
    return lib.cst_ans_decode_gaussian_ragged(c, lo, hi, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["means"], p["stds"], p["symbols"],
                                              p["sym_offsets"], n_streams, p["order"], p["status"], None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for pointer in ("symbols", "means", "stds", "sym_offsets", "words", "n_words", "status"):
        assert _call(lib, name, null=(pointer,)) == bad, pointer
    for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
        assert _call(lib, name, cfg=cfg) == bad, cfg
    assert _call(lib, name, lo=5, hi=5) == bad
    assert _call(lib, name, lo=5, hi=4) == bad
    assert _call(lib, name, null=("word_offsets",), stride=0) == bad
    # ... and the same refusals whatever the number of streams
    assert _call(lib, name, null=("status",), n_streams=0) == bad
    assert _call(lib, name, lo=5, hi=5, n_streams=0) == bad


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_no_streams_is_ok_without_a_launch(lib, name):
    from constriction_amd import _native as N
    assert _call(lib, name, n_streams=0) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("order",)) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("word_offsets",), stride=16) == N.CST_OK
    assert _call(lib, name, n_streams=0, cfg=(16, 32, 12), lo=-60, hi=60) == N.CST_OK


def test_batched_exposes_the_named_functions():
    pytest.importorskip("torch")
    import inspect
    from constriction_amd import batched
    enc, dec = batched.ans_encode_gaussian_ragged, batched.ans_decode_gaussian_ragged
    assert list(inspect.signature(enc).parameters) == ["symbols", "sym_offsets", "min_symbol", "max_symbol", "means", "stds", "config", "order"]
    assert list(inspect.signature(dec).parameters) == ["encoded", "sym_offsets", "min_symbol", "max_symbol", "means", "stds", "out", "order"]
    assert inspect.signature(enc).parameters["config"].default == (32, 64, 24)
    assert inspect.signature(enc).parameters["order"].default == "auto" and inspect.signature(dec).parameters["order"].default == "auto"
