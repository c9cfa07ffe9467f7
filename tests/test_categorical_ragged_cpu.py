"""CPU-only: the ragged per-symbol Categorical calls (cst_{ans,range}_{encode,decode}_categorical_ragged and their *_jump forms) exist
at every layer -- exported, declared, bound in _native.SIGNATURES, present in the Rust ffi, wrapped in constriction_amd.batched -- and
judge their arguments before they touch the device, so the refusals run here, without a GPU (the harness of
tests/test_persymbol_ragged_jump_cpu.py::test_invalid_arguments_are_refused_before_the_device: host buffers behind every pointer, and
only calls that must be refused, or that hold no stream, are made)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
FFI = ROOT / "bindings" / "rust" / "src" / "ffi.rs"
PLAIN = [f"cst_{coder}_{way}_categorical_ragged" for coder in ("ans", "range") for way in ("encode", "decode")]
JUMP = [name + "_jump" for name in PLAIN]
CALLS = PLAIN + JUMP


def table_args(name):
    return ["d_jump_state"] if "_ans_" in name else ["d_jump_lower", "d_jump_range"]


def expected_args(name):
    """the plain calls as the Gaussian ragged calls with (d_probs, prob_bytes, n_symbols, n_total) for the model; the jump calls add the
    interval and the table in the order of cst_*_gaussian_ragged_jump (the decoders without d_order)"""
    jump = name.endswith("_jump")
    if "_encode_" in name:
        args = ["cfg", "d_symbols", "d_probs", "prob_bytes", "n_symbols", "n_total", "d_sym_offsets", "n_streams", "d_order", "d_words",
                "d_word_offsets", "stride_words", "d_n_words"]
        if jump:
            args += ["jump_interval", "d_chunk_offsets", "d_jump_pos"] + table_args(name)
        return args + ["d_status", "stream"]
    args = ["cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "d_probs", "prob_bytes", "n_symbols", "n_total",
            "d_symbols", "d_sym_offsets", "n_streams"]
    if jump:
        return args + ["jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos"] + table_args(name) + ["d_scratch", "d_status", "stream"]
    return args + ["d_order", "d_status", "stream"]


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def _declared(text, name):
    m = re.search(r"cst_status\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name}: not declared"
    return [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]


def test_the_eight_entry_points_exist_at_every_layer(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = FFI.read_text()
    for name in CALLS:
        assert _declared(text, name) == expected_args(name), name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(expected_args(name)), name
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} is not in the Rust ffi"
    for name in JUMP:
        # the tail of the Gaussian form, from the sym_offsets on: argument for argument
        gaussian = _declared(text, name.replace("categorical", "gaussian"))
        mine = expected_args(name)
        assert mine[mine.index("d_sym_offsets"):] == gaussian[gaussian.index("d_sym_offsets"):], name
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


POINTERS = ("symbols", "probs", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "chunk_offsets", "jump_pos", "jump_a", "jump_b",
            "scratch")


def _call(lib, name, cfg=(32, 64, 24), null=(), prob_bytes=4, k=5, n_total=8, stride=0, n_streams=1, interval=64, n_chunks=8):
    from constriction_amd import _native as N
    buf = {key: np.zeros(64, dtype=np.float64) for key in POINTERS}
    p = {key: (None if key in null else ctypes.c_void_p(v.ctypes.data)) for key, v in buf.items()}
    c = N.CoderConfig(*cfg)
    table = (p["jump_pos"], p["jump_a"]) if "_ans_" in name else (p["jump_pos"], p["jump_a"], p["jump_b"])
    jump = name.endswith("_jump")
    if "_encode_" in name:
        tail = (interval, p["chunk_offsets"], *table) if jump else ()
        return getattr(lib, name)(c, p["symbols"], p["probs"], prob_bytes, k, n_total, p["sym_offsets"], n_streams, p["order"], p["words"],
                                  p["word_offsets"], stride, p["n_words"], *tail, p["status"], None)
    tail = (interval, p["chunk_offsets"], n_chunks, *table, p["scratch"]) if jump else (p["order"],)
    return getattr(lib, name)(c, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["probs"], prob_bytes, k, n_total, p["symbols"],
                              p["sym_offsets"], n_streams, *tail, p["status"], None)


def required(name):
    r = ["symbols", "probs", "sym_offsets", "words", "n_words", "status"]
    if name.endswith("_jump"):
        r += ["chunk_offsets", "jump_pos", "jump_a"] + (["jump_b"] if "_range_" in name else []) + (["scratch"] if "_decode_" in name else [])
    return r


@pytest.mark.parametrize("name", CALLS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad, model = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    for n_streams in (0, 1):
        for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
            assert _call(lib, name, cfg=cfg, n_streams=n_streams) == bad, cfg
        for pointer in required(name):
            assert _call(lib, name, null=(pointer,), n_streams=n_streams) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_streams=n_streams) == bad
        for prob_bytes in (0, 2, 3, 5, 16, -4):
            assert _call(lib, name, prob_bytes=prob_bytes, n_streams=n_streams) == bad, prob_bytes
        # K < 2, or no room for a nonzero probability each plus one: K >= 2^P - 1
        for cfg, k in (((32, 64, 24), 1), ((32, 64, 24), 0), ((32, 64, 24), -3), ((32, 64, 24), (1 << 24) - 1), ((16, 32, 12), 4095),
                       ((16, 32, 12), 5000), ((32, 64, 3), 7)):
            assert _call(lib, name, cfg=cfg, k=k, n_streams=n_streams) == model, (cfg, k)
        # ... an invalid argument is reported before a model that cannot be built
        assert _call(lib, name, k=1, prob_bytes=3, n_streams=n_streams) == bad
        assert _call(lib, name, k=1, null=("probs",), n_streams=n_streams) == bad
        if name.endswith("_jump"):
            for interval in (0, 8, 24, 100, 1 << 31, (1 << 31) + 16):
                assert _call(lib, name, interval=interval, n_streams=n_streams) == bad, (interval, n_streams)
            if "_decode_" in name:
                assert _call(lib, name, n_chunks=1 << 32, n_streams=n_streams) == bad
    for n_streams in (1 << 31, 1 << 32, 1 << 62):                       # more streams than a launch has blocks
        assert _call(lib, name, n_streams=n_streams) == bad, n_streams
    if "_encode_" in name:
        assert _call(lib, name, n_total=64 * ((1 << 31) - 1) + 1) == bad      # more rows than pass 1 has blocks of 64
    assert _call(lib, name, null=POINTERS) == bad


@pytest.mark.parametrize("name", CALLS)
def test_no_streams_is_ok_and_launches_nothing(lib, name):
    from constriction_amd import _native as N
    for cfg, k in (((32, 64, 24), 2), ((32, 64, 24), (1 << 24) - 2), ((32, 64, 12), 257), ((16, 32, 12), 4094), ((16, 32, 16), 65)):
        for prob_bytes in (4, 8):
            assert _call(lib, name, cfg=cfg, k=k, prob_bytes=prob_bytes, n_streams=0) == N.CST_OK, (cfg, k)
    assert _call(lib, name, n_streams=0, n_total=0, interval=(1 << 31) - 16, n_chunks=(1 << 32) - 1) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("order", "word_offsets"), stride=7) == N.CST_OK


NAMES = ["ans_encode_categorical_ragged", "ans_decode_categorical_ragged", "range_encode_categorical_ragged", "range_decode_categorical_ragged"]


def test_batched_exposes_the_four_names():
    pytest.importorskip("torch")
    import inspect
    from constriction_amd import batched
    for fn in NAMES:
        f = getattr(batched, fn)
        params = list(inspect.signature(f).parameters)
        if "_encode_" in fn:
            assert params == ["symbols", "sym_offsets", "probabilities", "config", "order", "jump_every"], fn
            assert f.__kwdefaults__ == {"jump_every": 0} and inspect.signature(f).parameters["config"].default == (32, 64, 24)
        else:
            assert params == ["encoded", "sym_offsets", "probabilities", "out", "order"], fn
        assert inspect.signature(f).parameters["order"].default == "auto"
    assert "DESIGN.md 4.21" in batched._encode_categorical_ragged.__doc__ and "measured" in batched._encode_categorical_ragged.__doc__


@pytest.mark.parametrize("jump_every", [-16, 8, 24, "often", 1 << 31])
@pytest.mark.parametrize("fn", [n for n in NAMES if "_encode_" in n])
def test_jump_every_is_judged_first(fn, jump_every):
    """CPU tensors: anything else the function did with them would fail differently"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    sym, off, probs = torch.zeros(8, dtype=torch.int32), torch.tensor([0, 3, 8]), torch.ones(8, 5)
    with pytest.raises(ValueError, match="jump_every"):
        getattr(batched, fn)(sym, off, probs, jump_every=jump_every)


def test_decoders_refuse_the_other_coders_batch_and_table():
    """judged before any tensor is looked at (CPU tensors: anything else would fail differently)"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    probs, off = torch.ones(8, 5), torch.tensor([0, 3, 8])
    of_range = batched.RangeRaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    of_ans = batched.RaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64))
    batch = lambda coder, table: batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None,
                                                     table, coder)
    with pytest.raises(ValueError, match="coder"):
        batched.ans_decode_categorical_ragged(batch("range", None), off, probs)
    with pytest.raises(ValueError, match="coder"):
        batched.range_decode_categorical_ragged(batch("ans", None), off, probs)
    with pytest.raises(ValueError, match="another coder"):
        batched.ans_decode_categorical_ragged(batch("ans", of_range), off, probs)
    with pytest.raises(ValueError, match="another coder"):
        batched.range_decode_categorical_ragged(batch("range", of_ans), off, probs)
