"""CPU-only: random access into ragged batches (cst_{ans,range}_decode_ragged_select, their scratch sizes, the two `batched` functions)
exists at every layer; the C calls judge their arguments before they touch the device, so the argument checks run here, without a GPU;
and the Python layer's piece count is the brute-force count of the chunks a range touches."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
ANS, RANGE = "cst_ans_decode_ragged_select", "cst_range_decode_ragged_select"
SCRATCH = {ANS: "cst_ragged_select_scratch_bytes", RANGE: "cst_range_ragged_select_scratch_bytes"}
BATCH = ["model", "cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "d_sym_offsets", "n_streams", "jump_interval",
         "d_chunk_offsets", "n_chunks_total", "d_jump_pos"]
QUERIES = ["d_query_stream", "d_query_first", "d_query_count", "n_queries", "d_piece_offsets", "n_pieces_total", "d_symbols_out", "d_out_offsets",
           "d_scratch", "d_status", "stream"]
ARGS = {ANS: BATCH + ["d_jump_state"] + QUERIES, RANGE: BATCH + ["d_jump_lower", "d_jump_range"] + QUERIES}
TABLE = {ANS: ("chunk_offsets", "jump_pos", "jump_state"), RANGE: ("chunk_offsets", "jump_pos", "jump_lower", "jump_range")}


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
    for name in (ANS, RANGE):
        assert _declared(text, name) == ARGS[name], name
        assert _declared(text, SCRATCH[name]) == ["n_pieces_total"]
        for symbol in (name, SCRATCH[name]):
            assert hasattr(lib, symbol), f"{symbol} is not exported"
            assert symbol in _native.SIGNATURES
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(ARGS[name])
        for arg, ctype in zip(ARGS[name], args):
            want = (_native.CoderConfig if arg == "cfg" else
                    ctypes.c_size_t if arg in ("stride_words", "words_capacity", "n_streams", "jump_interval", "n_chunks_total", "n_queries",
                                               "n_pieces_total") else ctypes.c_void_p)
            assert ctype == want, (name, arg)
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


@pytest.mark.parametrize("name", [ANS, RANGE])
def test_scratch_is_monotone_and_never_empty(lib, name):
    fn = getattr(lib, SCRATCH[name])
    sizes = [fn(n) for n in (0, 1, 2, 63, 64, 65, 1000, 1001, 1 << 20, (1 << 32) - 1)]
    assert sizes[0] > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # a piece's record is ten 32-bit words (two 64-bit and six 32-bit fields)
    assert fn(1000) >= fn(0) + 40 * 1000


POINTERS = ("words", "word_offsets", "n_words", "sym_offsets", "chunk_offsets", "jump_pos", "jump_state", "jump_lower", "jump_range", "query_stream",
            "query_first", "query_count", "piece_offsets", "symbols_out", "out_offsets", "scratch", "status")


def _call(lib, name, model=None, cfg=(32, 64, 24), null=(), stride=0, n_streams=1, interval=64, n_chunks=8, n_queries=1, n_pieces=8):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_queries > 0 would go on to the
    device, so only calls that must fail them are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in POINTERS}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    table = [p[k] for k in TABLE[name][1:]]
    return getattr(lib, name)(model, N.CoderConfig(*cfg), p["words"], p["word_offsets"], stride, 64, p["n_words"], p["sym_offsets"], n_streams,
                              interval, p["chunk_offsets"], n_chunks, *table, p["query_stream"], p["query_first"], p["query_count"], n_queries,
                              p["piece_offsets"], n_pieces, p["symbols_out"], p["out_offsets"], p["scratch"], p["status"], None)


@pytest.mark.parametrize("name", [ANS, RANGE])
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    """No model can be made without a device, so every call here carries a NULL model: refused whatever else it holds, and refused
    FIRST -- nothing behind the host pointers is read, nothing is launched.  (The same refusals with a real model:
    tests/test_gpu_ragged_select.py::test_refusals_with_a_model.)"""
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for n_streams in (0, 1, 1000):
        for n_queries in (0, 1, 1000):
            assert _call(lib, name, n_streams=n_streams, n_queries=n_queries) == bad
            assert _call(lib, name, n_streams=n_streams, n_queries=n_queries, cfg=(16, 32, 12)) == bad
    for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24), (32, 64, 24)):
        assert _call(lib, name, cfg=cfg) == bad and _call(lib, name, cfg=cfg, n_queries=0) == bad, cfg
    for n_queries in (0, 1):
        # every refusal of the plain decoders
        for pointer in ("sym_offsets", "n_words"):
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_queries=n_queries) == bad
        # an interval that is neither 0 nor a multiple of 8, or above 2^31 - 1
        for interval in (4, 12, 63, 1 << 31, (1 << 31) + 8):
            assert _call(lib, name, interval=interval, n_queries=n_queries) == bad, interval
        # a table given only in part: an interval without all of its arrays, arrays without an interval
        for pointer in TABLE[name]:
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
            assert _call(lib, name, interval=0, null=tuple(k for k in TABLE[name] if k != pointer), n_queries=n_queries) == bad, pointer
        assert _call(lib, name, interval=0, n_queries=n_queries) == bad
        assert _call(lib, name, interval=64, null=TABLE[name], n_queries=n_queries) == bad
        # exactly one of first / count
        assert _call(lib, name, null=("query_first",), n_queries=n_queries) == bad
        assert _call(lib, name, null=("query_count",), n_queries=n_queries) == bad
        assert _call(lib, name, n_pieces=1 << 32, n_queries=n_queries) == bad
        assert _call(lib, name, n_chunks=1 << 32, n_queries=n_queries) == bad
    for pointer in ("query_stream", "piece_offsets", "out_offsets", "scratch", "status"):
        assert _call(lib, name, null=(pointer,), n_queries=1) == bad, pointer
    assert _call(lib, name, null=POINTERS) == bad


def _brute_force_pieces(first, count, interval):
    """the chunks that hold at least one of the symbols first .. first + count - 1"""
    if interval == 0:
        return 1 if count > 0 else 0
    return len({k // interval for k in range(first, first + count)})


@pytest.mark.parametrize("interval", [0, 8, 24, 64, 256])
def test_piece_counts_are_the_chunks_a_range_touches(interval):
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    step = interval or 8
    firsts = sorted({c * step + r for c in (0, 1, 5) for r in (0, 1, step - 1)})
    counts = [0, 1, step - 1, step, step + 1, 3 * step]
    cases = [(f, n) for f in firsts for n in counts]
    # ranges that end exactly on a boundary, from every kind of start
    cases += [(f, e - f) for f in firsts for e in (step, 2 * step, 6 * step, 9 * step) if e > f]
    first = torch.tensor([f for f, _ in cases], dtype=torch.int64)
    count = torch.tensor([n for _, n in cases], dtype=torch.int64)
    got = batched._select_piece_counts(first, count, interval)
    assert got.dtype == torch.int64
    assert got.tolist() == [_brute_force_pieces(f, n, interval) for f, n in cases]
    # ... and the formula of the header, for the same cases
    if interval:
        assert got.tolist() == [0 if n == 0 else -(-(f % interval + n) // interval) for f, n in cases]


def test_batched_exposes_the_functions():
    pytest.importorskip("torch")
    from constriction_amd import batched
    for fn in (batched.ans_decode_ragged_select, batched.range_decode_ragged_select):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["encoded", "model", "sym_offsets", "streams", "first", "count", "out"]
        assert all(sig.parameters[k].default is None for k in ("first", "count", "out"))
    # the existing decoders keep their signatures
    assert list(inspect.signature(batched.ans_decode_ragged).parameters) == ["encoded", "model", "sym_offsets", "out", "order"]
    assert list(inspect.signature(batched.range_decode_ragged).parameters) == ["encoded", "model", "sym_offsets", "out", "order"]


def test_the_coders_refuse_each_others_batches():
    """judged first, on CPU tensors and without a model: anything else the functions did would fail differently"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    ans = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24))
    rng = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, None, "range")
    with pytest.raises(ValueError, match="'ans'"):
        batched.range_decode_ragged_select(ans, None, z(3, torch.int64), [0])
    with pytest.raises(ValueError, match="'range'"):
        batched.ans_decode_ragged_select(rng, None, z(3, torch.int64), [0])
