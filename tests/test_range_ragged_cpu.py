"""CPU-only: the ragged range coder with a shared table (cst_range_{encode,decode}_ragged, cst_range_count_until) exists at every
layer, and it judges its arguments before it touches the device -- so the argument checks run here, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
ENCODE, DECODE, COUNT = "cst_range_encode_ragged", "cst_range_decode_ragged", "cst_range_count_until"
ENTRY_POINTS = [ENCODE, DECODE, COUNT]
# every call takes the arguments of its ANS twin with a schedule
TWIN = {ENCODE: "cst_ans_encode_ragged_ordered", DECODE: "cst_ans_decode_ragged_ordered", COUNT: "cst_ans_count_until_ordered"}
ARGS = {
    ENCODE: ["model", "cfg", "d_symbols", "d_sym_offsets", "n_streams", "d_order", "d_words", "d_word_offsets", "stride_words", "d_n_words",
             "d_status", "stream"],
    DECODE: ["model", "cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "d_symbols", "d_sym_offsets",
             "n_streams", "d_order", "d_status", "stream"],
    COUNT: ["model", "cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "n_streams", "d_order", "eof_symbol",
            "max_symbols", "d_lengths", "d_status", "stream"],
}


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"cst_status\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, f"{name}: not declared"
        declared = [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]
        assert declared == ARGS[name], f"{name}: {declared}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
        assert _native.SIGNATURES[name] == _native.SIGNATURES[TWIN[name]]
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def _call(lib, name, model=None, cfg=(32, 64, 24), null=(), stride=0, n_streams=1):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_streams > 0 would go on to the
    device, so only calls that must fail them (or that have no streams) are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "lengths")}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    c = N.CoderConfig(*cfg)
    if name == ENCODE:
        return lib.cst_range_encode_ragged(model, c, p["symbols"], p["sym_offsets"], n_streams, p["order"], p["words"], p["word_offsets"], stride,
                                           p["n_words"], p["status"], None)
    if name == DECODE:
        return lib.cst_range_decode_ragged(model, c, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["symbols"], p["sym_offsets"],
                                           n_streams, p["order"], p["status"], None)
    return lib.cst_range_count_until(model, c, p["words"], p["word_offsets"], stride, 64, p["n_words"], n_streams, p["order"], 3, 100,
                                     p["lengths"], p["status"], None)


REQUIRED = {ENCODE: ("sym_offsets", "words", "n_words", "status"), DECODE: ("sym_offsets", "n_words", "status"),
            COUNT: ("n_words", "lengths", "status")}


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_null_model_is_refused(lib, name):
    from constriction_amd import _native as N
    for n_streams in (0, 1, 1000):
        assert _call(lib, name, model=None, n_streams=n_streams) == N.CST_ERR_INVALID_ARGUMENT
        assert _call(lib, name, model=None, n_streams=n_streams, cfg=(16, 32, 12)) == N.CST_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    """No model can be made without a device, so every call here carries a NULL model: refused whatever else it holds -- NULL
    pointers, unsupported configurations, no slabs, no streams -- and refused FIRST: nothing behind the host pointers is read, nothing
    is launched.  (The same refusals with a real model: tests/test_gpu_range_ragged.py.)"""
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24), (32, 64, 24)):
        assert _call(lib, name, cfg=cfg) == bad and _call(lib, name, cfg=cfg, n_streams=0) == bad, cfg
    for pointer in REQUIRED[name]:
        assert _call(lib, name, null=(pointer,)) == bad and _call(lib, name, null=(pointer,), n_streams=0) == bad, pointer
    assert _call(lib, name, null=("word_offsets",), stride=0) == bad
    assert _call(lib, name, n_streams=1 << 32) == bad
    assert _call(lib, name, null=tuple(REQUIRED[name]) + ("order", "word_offsets", "symbols")) == bad


def test_batched_exposes_the_three_functions():
    pytest.importorskip("torch")
    import inspect
    from constriction_amd import batched
    params = lambda fn: list(inspect.signature(fn).parameters)
    default = lambda fn, name: inspect.signature(fn).parameters[name].default
    enc, dec, until = batched.range_encode_ragged, batched.range_decode_ragged, batched.range_decode_until
    assert params(enc) == ["symbols", "sym_offsets", "model", "config", "order"]
    assert default(enc, "config") == (32, 64, 24) and default(enc, "order") == "auto"
    assert params(dec) == ["encoded", "model", "sym_offsets", "out", "order"]
    assert default(dec, "out") is None and default(dec, "order") == "auto"
    assert params(until) == ["encoded", "model", "eof_symbol", "max_symbols"] and default(until, "max_symbols") is None
    # ... the ANS functions keep theirs
    assert params(batched.ans_encode_ragged) == ["symbols", "sym_offsets", "model", "config", "order", "jump_every"]
    assert params(batched.ans_decode_ragged) == params(dec) and params(batched.ans_decode_until) == params(until)


def test_the_range_decoders_refuse_an_ans_batch_first():
    """a RaggedBatch says which coder wrote it; the other coder's decoders refuse it before they look at anything else (CPU tensors,
    no model: anything else they did would fail differently)"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    ans = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, None, "ans")
    assert batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24)).coder == "ans"
    with pytest.raises(ValueError, match="'ans'"):
        batched.range_decode_ragged(ans, None, z(3, torch.int64))
    with pytest.raises(ValueError, match="'ans'"):
        batched.range_decode_until(ans, None, 5)
    rng = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, None, "range")
    with pytest.raises(ValueError, match="'range'"):
        batched.ans_decode_ragged(rng, None, z(3, torch.int64))
