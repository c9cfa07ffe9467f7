"""CPU-only: jump points for ragged range batches (cst_range_{encode,decode}_ragged_jump, cst_range_ragged_jump_scratch_bytes) exist at
every layer, and the calls judge their arguments before they touch the device -- so the argument checks run here, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
SCRATCH, ENCODE, DECODE = "cst_range_ragged_jump_scratch_bytes", "cst_range_encode_ragged_jump", "cst_range_decode_ragged_jump"
# the arguments of the ANS twins, with d_jump_state replaced by d_jump_lower, d_jump_range
TWIN = {SCRATCH: "cst_ragged_jump_scratch_bytes", ENCODE: "cst_ans_encode_ragged_jump", DECODE: "cst_ans_decode_ragged_jump"}
ARGS = {
    SCRATCH: ["n_chunks_total"],
    ENCODE: ["model", "cfg", "d_symbols", "d_sym_offsets", "n_streams", "d_order", "d_words", "d_word_offsets", "stride_words", "d_n_words",
             "jump_interval", "d_chunk_offsets", "d_jump_pos", "d_jump_lower", "d_jump_range", "d_status", "stream"],
    DECODE: ["model", "cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "d_symbols", "d_sym_offsets",
             "n_streams", "jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos", "d_jump_lower", "d_jump_range", "d_scratch",
             "d_status", "stream"],
}


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def _declared(text, name):
    m = re.search(r"(?:cst_status|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name}: not declared"
    return [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in (SCRATCH, ENCODE, DECODE):
        assert _declared(text, name) == ARGS[name], name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
        # ... and the ANS twin's declaration differs by exactly that one argument
        twin = _declared(text, TWIN[name])
        k = twin.index("d_jump_state") if "d_jump_state" in twin else None
        assert ARGS[name] == (twin if k is None else twin[:k] + ["d_jump_lower", "d_jump_range"] + twin[k + 1:])
        res, args = _native.SIGNATURES[name]
        twin_res, twin_args = _native.SIGNATURES[TWIN[name]]
        assert res == twin_res and len(args) == len(ARGS[name])
        assert list(args) == (list(twin_args) if k is None else list(twin_args[:k]) + [ctypes.c_void_p] + list(twin_args[k:]))
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5
    assert "No jump points (RangeEncoder::pos / RangeDecoder::seek)" not in HEADER.read_text()
    assert lib.cst_range_ragged_jump_scratch_bytes(0) > 0
    assert lib.cst_range_ragged_jump_scratch_bytes(1000) >= lib.cst_range_ragged_jump_scratch_bytes(0) + 28 * 1000


POINTERS = ("symbols", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "chunk_offsets", "jump_pos", "jump_lower",
            "jump_range", "scratch")


def _call(lib, name, model=None, cfg=(32, 64, 24), null=(), stride=0, n_streams=1, interval=64, n_chunks=8):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_streams > 0 would go on to the
    device, so only calls that must fail them are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in POINTERS}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    c = N.CoderConfig(*cfg)
    if name == ENCODE:
        return lib.cst_range_encode_ragged_jump(model, c, p["symbols"], p["sym_offsets"], n_streams, p["order"], p["words"], p["word_offsets"],
                                                stride, p["n_words"], interval, p["chunk_offsets"], p["jump_pos"], p["jump_lower"],
                                                p["jump_range"], p["status"], None)
    return lib.cst_range_decode_ragged_jump(model, c, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["symbols"], p["sym_offsets"],
                                            n_streams, interval, p["chunk_offsets"], n_chunks, p["jump_pos"], p["jump_lower"], p["jump_range"],
                                            p["scratch"], p["status"], None)


REQUIRED = {ENCODE: ("sym_offsets", "words", "n_words", "status", "chunk_offsets", "jump_pos", "jump_lower", "jump_range"),
            DECODE: ("sym_offsets", "n_words", "status", "chunk_offsets", "jump_pos", "jump_lower", "jump_range", "scratch")}


@pytest.mark.parametrize("name", [ENCODE, DECODE])
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    """No model can be made without a device, so every call here carries a NULL model: refused whatever else it holds, and refused
    FIRST -- nothing behind the host pointers is read, nothing is launched.  (The same refusals with a real model:
    tests/test_gpu_range_ragged_jump.py.)"""
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for n_streams in (0, 1, 1000):
        assert _call(lib, name, n_streams=n_streams) == bad
        assert _call(lib, name, n_streams=n_streams, cfg=(16, 32, 12)) == bad
    for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24), (32, 64, 24)):
        assert _call(lib, name, cfg=cfg) == bad and _call(lib, name, cfg=cfg, n_streams=0) == bad, cfg
    for n_streams in (0, 1):
        for interval in (0, 12, 1 << 31):
            assert _call(lib, name, interval=interval, n_streams=n_streams) == bad, (interval, n_streams)
        for pointer in REQUIRED[name]:
            assert _call(lib, name, null=(pointer,), n_streams=n_streams) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_streams=n_streams) == bad
        if name == DECODE:
            assert _call(lib, name, n_chunks=1 << 32, n_streams=n_streams) == bad
    assert _call(lib, name, null=POINTERS) == bad


def test_batched_exposes_the_function_and_the_table():
    pytest.importorskip("torch")
    import dataclasses
    import inspect
    from constriction_amd import batched
    sig = inspect.signature(batched.range_encode_ragged_jump)
    assert list(sig.parameters) == ["symbols", "sym_offsets", "model", "config", "order", "jump_every"]
    assert sig.parameters["config"].default == (32, 64, 24) and sig.parameters["order"].default == "auto"
    assert sig.parameters["jump_every"].default == "auto"
    assert [f.name for f in dataclasses.fields(batched.RangeRaggedJump)] == ["interval", "chunk_offsets", "pos", "lower", "range"]
    assert [f.name for f in dataclasses.fields(batched.RaggedJump)] == ["interval", "chunk_offsets", "pos", "state"]
    assert [f.name for f in dataclasses.fields(batched.RaggedBatch)] == ["words", "word_offsets", "n_words", "status", "config", "order", "jump",
                                                                        "coder"]
    # the plain functions keep their signatures
    assert list(inspect.signature(batched.range_encode_ragged).parameters) == ["symbols", "sym_offsets", "model", "config", "order"]
    assert list(inspect.signature(batched.range_decode_ragged).parameters) == ["encoded", "model", "sym_offsets", "out", "order"]


@pytest.mark.parametrize("jump_every", [-8, 12, "often"])
def test_jump_every_is_judged_first(jump_every):
    """CPU tensors and no model: anything else the function did would fail differently"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    with pytest.raises(ValueError, match="jump_every"):
        batched.range_encode_ragged_jump(torch.zeros(8, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), None, jump_every=jump_every)


def test_a_batch_is_still_built_positionally():
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    rng = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, None, "range")
    assert rng.coder == "range" and rng.jump is None and rng.order is None
    assert batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24)).coder == "ans"
    table = batched.RangeRaggedJump(64, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    rng.jump = table
    assert rng.jump.interval == 64 and rng.jump.lower.numel() == 4 and rng.jump.range.numel() == 4
    # a range batch -- with or without a table -- is refused by the ANS decoder before it looks at anything else
    with pytest.raises(ValueError, match="'range'"):
        batched.ans_decode_ragged(rng, None, z(3, torch.int64))
