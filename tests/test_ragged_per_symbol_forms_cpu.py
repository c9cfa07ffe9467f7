"""CPU-only: the six ragged per-symbol entry points beyond ANS x Gaussian (cst_range_{encode,decode}_gaussian_ragged and
cst_{ans,range}_{encode,decode}_family_ragged) exist at every layer, and they judge their arguments before they touch the device --
so their argument checks run here, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
GAUSSIAN = ["cst_range_encode_gaussian_ragged", "cst_range_decode_gaussian_ragged"]
FAMILY = ["cst_ans_encode_family_ragged", "cst_ans_decode_family_ragged", "cst_range_encode_family_ragged", "cst_range_decode_family_ragged"]
ENTRY_POINTS = GAUSSIAN + FAMILY
LAPLACE, CAUCHY = 1, 2


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        family = r"int32_t\s+family\s*,\s*" if name in FAMILY else ""
        m = re.search(r"cst_status\s+%s\s*\(\s*cst_coder_config\s+cfg\s*,\s*%sint32_t\s+min_symbol\s*,\s*int32_t\s+max_symbol\s*,([^;]*)\)\s*;"
                      % (name, family), text)
        assert m, f"{name}: not declared"
        params = ("d_a", "d_b") if name in FAMILY else ("d_means", "d_stds")
        for arg in ("d_symbols", *params, "d_sym_offsets", "n_streams", "d_order", "d_words", "d_word_offsets", "stride_words", "d_n_words",
                    "d_status", "stream"):
            assert re.search(r"\b%s\b" % arg, m.group(1)), f"{name}: no argument {arg}"
        assert ("words_capacity" in m.group(1)) == ("decode" in name), f"{name}: words_capacity belongs to the decoders"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
        # (the family calls take one int32 more than the Gaussian ones, right after the configuration)
        twin = _native.SIGNATURES["cst_ans_%s_gaussian_ragged" % ("encode" if "encode" in name else "decode")]
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is twin[0]
        assert argtypes == (twin[1][:1] + [ctypes.c_int32] + twin[1][1:] if name in FAMILY else twin[1])
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def _call(lib, name, cfg=(32, 64, 24), lo=-100, hi=100, null=(), stride=0, n_streams=1, family=LAPLACE):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_streams > 0 would go on to
    the device, so only calls that must fail them (or that have no streams) are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "a", "b", "sym_offsets", "order", "words", "word_offsets", "n_words", "status")}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    head = (N.CoderConfig(*cfg), family, lo, hi) if name in FAMILY else (N.CoderConfig(*cfg), lo, hi)
    if "encode" in name:
        return getattr(lib, name)(*head, p["symbols"], p["a"], p["b"], p["sym_offsets"], n_streams, p["order"], p["words"], p["word_offsets"],
                                  stride, p["n_words"], p["status"], None)
    return getattr(lib, name)(*head, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["a"], p["b"], p["symbols"], p["sym_offsets"],
                              n_streams, p["order"], p["status"], None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for pointer in ("symbols", "a", "b", "sym_offsets", "words", "n_words", "status"):
        assert _call(lib, name, null=(pointer,)) == bad, pointer
    for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
        assert _call(lib, name, cfg=cfg) == bad, cfg
    assert _call(lib, name, lo=5, hi=5) == bad
    assert _call(lib, name, lo=5, hi=4) == bad
    assert _call(lib, name, null=("word_offsets",), stride=0) == bad
    # ... and the same refusals whatever the number of streams
    assert _call(lib, name, null=("status",), n_streams=0) == bad
    assert _call(lib, name, lo=5, hi=5, n_streams=0) == bad
    for pointer in ("symbols", "a", "b", "sym_offsets", "words", "n_words"):
        assert _call(lib, name, null=(pointer,), n_streams=0) == bad, pointer
    assert _call(lib, name, cfg=(32, 64, 25), n_streams=0) == bad
    assert _call(lib, name, null=("word_offsets",), stride=0, n_streams=0) == bad


@pytest.mark.parametrize("name", FAMILY)
def test_only_laplace_and_cauchy_are_families(lib, name):
    """family = 0, CST_FAMILY_BINOMIAL (a family of the library, but not of these calls) and unknown values"""
    from constriction_amd import _native as N
    assert (N.FAMILY_LAPLACE, N.FAMILY_CAUCHY) == (LAPLACE, CAUCHY)
    for family in (0, 3, 4, -1, 1 << 20):
        assert _call(lib, name, family=family) == N.CST_ERR_INVALID_ARGUMENT, family
        assert _call(lib, name, family=family, n_streams=0) == N.CST_ERR_INVALID_ARGUMENT, family
    for family in (LAPLACE, CAUCHY):
        assert _call(lib, name, family=family, n_streams=0) == N.CST_OK


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_no_streams_is_ok_without_a_launch(lib, name):
    from constriction_amd import _native as N
    assert _call(lib, name, n_streams=0) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("order",)) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("word_offsets",), stride=16) == N.CST_OK
    assert _call(lib, name, n_streams=0, cfg=(16, 32, 12), lo=-60, hi=60) == N.CST_OK
    assert _call(lib, name, n_streams=0, family=CAUCHY) == N.CST_OK


def test_batched_exposes_the_named_functions():
    pytest.importorskip("torch")
    import inspect
    from constriction_amd import batched
    params = lambda fn: list(inspect.signature(fn).parameters)
    default = lambda fn, name: inspect.signature(fn).parameters[name].default
    enc, dec = batched.range_encode_gaussian_ragged, batched.range_decode_gaussian_ragged
    assert params(enc) == ["symbols", "sym_offsets", "min_symbol", "max_symbol", "means", "stds", "config", "order"]
    assert params(dec) == ["encoded", "sym_offsets", "min_symbol", "max_symbol", "means", "stds", "out", "order"]
    # ... and the existing pair keeps its signature
    assert params(batched.ans_encode_gaussian_ragged) == params(enc) and params(batched.ans_decode_gaussian_ragged) == params(dec)
    for coder in ("ans", "range"):
        enc, dec = getattr(batched, f"{coder}_encode_family_ragged"), getattr(batched, f"{coder}_decode_family_ragged")
        assert params(enc) == ["family", "symbols", "sym_offsets", "lo", "hi", "a", "b", "config", "order"]
        assert params(dec) == ["family", "encoded", "sym_offsets", "lo", "hi", "a", "b", "out", "order"]
    for fn in (batched.range_encode_gaussian_ragged, batched.ans_encode_family_ragged, batched.range_encode_family_ragged):
        assert default(fn, "config") == (32, 64, 24) and default(fn, "order") == "auto"
    for fn in (batched.range_decode_gaussian_ragged, batched.ans_decode_family_ragged, batched.range_decode_family_ragged):
        assert default(fn, "out") is None and default(fn, "order") == "auto"
    for coder in ("ans", "range"):
        for way in ("encode", "decode"):
            for family in ("laplace", "cauchy"):
                fn = getattr(batched, f"{coder}_{way}_{family}_ragged")
                assert callable(fn) and fn.__name__ == f"{coder}_{way}_{family}_ragged"


def test_a_ragged_batch_says_which_coder_wrote_it():
    pytest.importorskip("torch")
    import dataclasses
    from constriction_amd import batched
    fields = dataclasses.fields(batched.RaggedBatch)
    assert [f.name for f in fields] == ["words", "word_offsets", "n_words", "status", "config", "order", "jump", "coder"]
    assert fields[-1].default == "ans"
