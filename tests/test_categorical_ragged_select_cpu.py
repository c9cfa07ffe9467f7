"""CPU-only: random access into ragged per-symbol Categorical batches (cst_{ans,range}_decode_categorical[_perfect]_ragged_select and the
four `batched` functions) exists at every layer -- header, library, ctypes prototypes, `batched`, the Rust crate -- and the C calls judge
their arguments before they touch the device, so the argument checks run here, without a GPU.  (On the device:
tests/test_gpu_categorical_ragged_select.py.)"""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
RUST = ROOT / "bindings" / "rust" / "src"
SCRATCH = "cst_persymbol_ragged_select_scratch_bytes"
NAMES = [f"cst_{coder}_decode_categorical_{perfect}ragged_select" for coder in ("ans", "range") for perfect in ("", "perfect_")]
WORDS = ["d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words"]
MODEL = ["d_probs", "prob_bytes", "n_symbols", "n_total"]
TABLE_HEAD = ["jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos"]
QUERIES = ["d_query_stream", "d_query_first", "d_query_count", "n_queries", "d_piece_offsets", "n_pieces_total", "d_symbols_out", "d_out_offsets",
           "d_scratch", "d_status", "stream"]
SIZES = ("stride_words", "words_capacity", "n_total", "max_piece_len", "n_streams", "jump_interval", "n_chunks_total", "n_queries", "n_pieces_total")
INTS = ("prob_bytes", "n_symbols")


def is_range(name):
    return name.startswith("cst_range")


def is_perfect(name):
    return "_perfect_" in name


def arguments(name):
    """the Gaussian select calls' list block by block: cfg alone, the words, the plain Categorical decoder's model arguments (the perfect
    pair: max_piece_len behind them), the streams, the table, the queries"""
    table = TABLE_HEAD + (["d_jump_lower", "d_jump_range"] if is_range(name) else ["d_jump_state"])
    return ["cfg"] + WORDS + MODEL + (["max_piece_len"] if is_perfect(name) else []) + ["d_sym_offsets", "n_streams"] + table + QUERIES


def table_pointers(name):
    return ("chunk_offsets", "jump_pos") + (("jump_lower", "jump_range") if is_range(name) else ("jump_state",))


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def _declared(text, name):
    m = re.search(r"(?:cst_status|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name}: not declared"
    return [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]


def test_header_library_and_prototypes_agree(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NAMES:
        assert _declared(text, name) == arguments(name), name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(arguments(name))
        for arg, ctype in zip(arguments(name), args):
            want = (_native.CoderConfig if arg == "cfg" else ctypes.c_size_t if arg in SIZES else ctypes.c_int32 if arg in INTS else ctypes.c_void_p)
            assert ctype == want, (name, arg)
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5
    # the header no longer says that the Categorical decoders have no select form
    assert "Categorical ragged decoders have no" not in re.sub(r"\s*\n \*\s*", " ", HEADER.read_text())


def test_rust_crate_declares_and_wraps_the_calls():
    ffi, wrappers = (RUST / "ffi.rs").read_text(), (RUST / "lib.rs").read_text()
    for name in NAMES:
        m = re.search(r"pub fn %s\(([^;]*?)\)\s*->\s*\w+;" % name, ffi)
        assert m, f"{name}: not declared in ffi.rs"
        assert [a.split(":")[0].strip() for a in m.group(1).split(",") if a.strip()] == arguments(name), name
        assert f"ffi::{name}(" in wrappers, f"{name}: no wrapper calls it"
    for wrapper in ("seek_and_decode_categorical_ragged", "seek_and_decode_categorical_perfect_ragged"):
        assert len(re.findall(r"pub unsafe fn %s<" % wrapper, wrappers)) == 2, wrapper          # BatchedAnsCoder and BatchedRangeDecoder


def test_the_scratch_holds_a_record_and_a_span_per_piece(lib):
    """all four calls take cst_persymbol_ragged_select_scratch_bytes: the perfect pair keeps a 32-bit span per piece behind the 92-byte
    records, inside what the function has always returned -- 96 n + 128, alignment slack of 15 bytes included"""
    fn = getattr(lib, SCRATCH)
    for n in (0, 1, 2, 63, 64, 65, 1000, 1001, 1 << 20, (1 << 32) - 1):
        assert fn(n) == 96 * n + 128
        assert fn(n) >= 15 + (92 + 4) * n
    assert lib.cst_ragged_select_scratch_bytes(1000) == 40 * 1000 + 128 == lib.cst_range_ragged_select_scratch_bytes(1000)


POINTERS = ("words", "word_offsets", "n_words", "probs", "sym_offsets", "chunk_offsets", "jump_pos", "jump_state", "jump_lower", "jump_range",
            "query_stream", "query_first", "query_count", "piece_offsets", "symbols_out", "out_offsets", "scratch", "status")


def _call(lib, name, cfg=(32, 64, 24), prob_bytes=4, k=8, null=(), stride=0, n_streams=1, interval=64, n_chunks=8, n_queries=1, n_pieces=8,
          max_piece=64):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_queries > 0 would go on to the
    device, so only calls that must fail them, or that carry no query, are made"""
    from constriction_amd import _native as N
    buf = {key: np.zeros(64, dtype=np.float64) for key in POINTERS}
    p = {key: (None if key in null else ctypes.c_void_p(v.ctypes.data)) for key, v in buf.items()}
    table = [p[key] for key in table_pointers(name)[1:]]
    bound = (max_piece,) if is_perfect(name) else ()
    return getattr(lib, name)(N.CoderConfig(*cfg), p["words"], p["word_offsets"], stride, 64, p["n_words"], p["probs"], prob_bytes, k, 8, *bound,
                              p["sym_offsets"], n_streams, interval, p["chunk_offsets"], n_chunks, *table, p["query_stream"], p["query_first"],
                              p["query_count"], n_queries, p["piece_offsets"], n_pieces, p["symbols_out"], p["out_offsets"], p["scratch"],
                              p["status"], None)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad, model, ok = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL, N.CST_OK
    table = table_pointers(name)
    no_table = dict(interval=0, null=table)
    for n_queries in (0, 1):
        # every refusal of the plain Categorical ragged decode call: its required pointers, the dtype, the preset
        for pointer in ("words", "n_words", "probs", "sym_offsets", "symbols_out", "status"):
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
            assert _call(lib, name, interval=0, null=table + (pointer,), n_queries=n_queries) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_queries=n_queries) == bad          # neither offsets nor a stride
        for prob_bytes in (0, 2, 3, 5, 16, -4):
            assert _call(lib, name, prob_bytes=prob_bytes, n_queries=n_queries) == bad, prob_bytes
        for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
            assert _call(lib, name, cfg=cfg, n_queries=n_queries) == bad, cfg
        assert _call(lib, name, n_streams=1 << 31, n_queries=n_queries) == bad
        # ... and its limits of K: the fast quantiser needs 2 <= K <= 2^P - 2, the perfect one 2 <= K <= min(2^P, 1024)
        for k in (1, 0, -1):
            assert _call(lib, name, k=k, n_queries=n_queries) == model, k
        if is_perfect(name):
            assert _call(lib, name, k=1025, n_queries=n_queries) == model
            assert _call(lib, name, cfg=(32, 64, 4), k=17, n_queries=n_queries) == model
            assert _call(lib, name, cfg=(32, 64, 4), k=16, n_queries=0) == ok
        else:
            assert _call(lib, name, cfg=(32, 64, 4), k=15, n_queries=n_queries) == model
            assert _call(lib, name, cfg=(32, 64, 4), k=14, n_queries=0) == ok
        # CST_ERR_INVALID_ARGUMENT comes before CST_ERR_MODEL, the query block's included
        assert _call(lib, name, k=1, null=("query_first",), n_queries=n_queries) == bad
        assert _call(lib, name, k=1, interval=24, n_queries=n_queries) == bad
        # an interval that is no multiple of 16 (the encoders' tiles), or above 2^31 - 1
        for interval in (4, 8, 24, 63, 1 << 31, (1 << 31) + 16):
            assert _call(lib, name, interval=interval, n_queries=n_queries) == bad, interval
        # a table given only in part: an interval without all of its arrays, arrays without an interval
        for pointer in table:
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
            assert _call(lib, name, interval=0, null=tuple(key for key in table if key != pointer), n_queries=n_queries) == bad, pointer
        assert _call(lib, name, interval=0, n_queries=n_queries) == bad
        assert _call(lib, name, interval=64, null=table, n_queries=n_queries) == bad
        assert _call(lib, name, n_chunks=1 << 32, n_queries=n_queries) == bad
        # exactly one of first / count
        assert _call(lib, name, null=("query_first",), n_queries=n_queries) == bad
        assert _call(lib, name, null=("query_count",), n_queries=n_queries) == bad
        assert _call(lib, name, n_pieces=1 << 32, n_queries=n_queries) == bad
        assert _call(lib, name, n_pieces=1 << 32, n_queries=n_queries, **no_table) == bad
    for pointer in ("query_stream", "piece_offsets", "out_offsets", "scratch"):
        assert _call(lib, name, null=(pointer,), n_queries=1) == bad, pointer
        assert _call(lib, name, k=1, null=(pointer,), n_queries=1) == bad, pointer
    # no queries: CST_OK and nothing is launched, with a table, without one, whole documents, and whatever hides behind the query pointers
    assert _call(lib, name, n_queries=0) == ok
    assert _call(lib, name, n_queries=0, prob_bytes=8) == ok
    assert _call(lib, name, n_queries=0, n_pieces=(1 << 32) - 1, n_chunks=(1 << 32) - 1, interval=(1 << 31) - 16) == ok
    assert _call(lib, name, n_queries=0, **no_table) == ok
    assert _call(lib, name, n_queries=0, interval=0, null=table + ("query_first", "query_count")) == ok
    assert _call(lib, name, n_queries=0, null=("query_stream", "piece_offsets", "out_offsets", "scratch", "query_first", "query_count")) == ok
    assert _call(lib, name, n_queries=0, n_streams=0) == ok
    assert _call(lib, name, n_queries=0, max_piece=0) == ok


def test_batched_exposes_the_functions():
    pytest.importorskip("torch")
    from constriction_amd import batched
    for coder in ("ans", "range"):
        for perfect in ("", "_perfect"):
            fn = getattr(batched, f"{coder}_decode_categorical{perfect}_ragged_select")
            plain = getattr(batched, f"{coder}_decode_categorical{perfect}_ragged")
            sig = inspect.signature(fn)
            assert list(sig.parameters) == ["encoded", "sym_offsets", "probabilities", "streams", "first", "count", "out"]
            assert all(sig.parameters[key].default is None for key in ("first", "count", "out"))
            # the model's arguments are the plain decoder's
            assert list(sig.parameters)[:-4] == list(inspect.signature(plain).parameters)[:-2]
    # the other select functions keep their signatures
    for fn in (batched.ans_decode_ragged_select, batched.range_decode_ragged_select):
        assert list(inspect.signature(fn).parameters) == ["encoded", "model", "sym_offsets", "streams", "first", "count", "out"]
    assert list(inspect.signature(batched.ans_decode_gaussian_ragged_select).parameters) == [
        "encoded", "sym_offsets", "min_symbol", "max_symbol", "means", "stds", "streams", "first", "count", "out"]


def test_batches_of_the_other_coder_are_refused():
    """judged first, on CPU tensors: the batch's coder, then the type of its jump table"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    ans_jump = batched.RaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64))
    range_jump = batched.RangeRaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    make = lambda coder, jump: batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, jump,
                                                   coder)
    args = (z(3, torch.int64), torch.zeros(0, 4, dtype=torch.float32), [0])
    for perfect in ("", "_perfect"):
        ans_fn, range_fn = (getattr(batched, f"{coder}_decode_categorical{perfect}_ragged_select") for coder in ("ans", "range"))
        with pytest.raises(ValueError, match="'ans'"):
            range_fn(make("ans", None), *args)
        with pytest.raises(ValueError, match="'range'"):
            ans_fn(make("range", None), *args)
        with pytest.raises(ValueError, match="jump points of another coder"):
            ans_fn(make("ans", range_jump), *args)
        with pytest.raises(ValueError, match="jump points of another coder"):
            range_fn(make("range", ans_jump), *args)
