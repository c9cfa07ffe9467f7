"""CPU-only: random access into ragged per-symbol batches (cst_{ans,range}_decode_{gaussian,family}_ragged_select, their scratch size,
the eight `batched` functions) exists at every layer, and the C calls judge their arguments before they touch the device, so the
argument checks run here, without a GPU.  (On the device: tests/test_gpu_persymbol_ragged_select.py.)"""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
SCRATCH = "cst_persymbol_ragged_select_scratch_bytes"
NAMES = [f"cst_{coder}_decode_{kind}_ragged_select" for coder in ("ans", "range") for kind in ("gaussian", "family")]
WORDS = ["d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words"]
TABLE_HEAD = ["jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos"]
QUERIES = ["d_query_stream", "d_query_first", "d_query_count", "n_queries", "d_piece_offsets", "n_pieces_total", "d_symbols_out", "d_out_offsets",
           "d_scratch", "d_status", "stream"]
SIZES = ("stride_words", "words_capacity", "n_streams", "jump_interval", "n_chunks_total", "n_queries", "n_pieces_total")
INTS = ("family", "min_symbol", "max_symbol")


def is_range(name):
    return name.startswith("cst_range")


def arguments(name):
    family = "family" in name
    model = ["cfg"] + (["family"] if family else []) + ["min_symbol", "max_symbol"]
    params = ["d_a", "d_b"] if family else ["d_means", "d_stds"]
    table = TABLE_HEAD + (["d_jump_lower", "d_jump_range"] if is_range(name) else ["d_jump_state"])
    return model + WORDS + params + ["d_sym_offsets", "n_streams"] + table + QUERIES


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


def test_header_declares_and_library_exports_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert _declared(text, SCRATCH) == ["n_pieces_total"]
    assert hasattr(lib, SCRATCH) and SCRATCH in _native.SIGNATURES
    for name in NAMES:
        assert _declared(text, name) == arguments(name), name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(arguments(name))
        for arg, ctype in zip(arguments(name), args):
            want = (_native.CoderConfig if arg == "cfg" else ctypes.c_size_t if arg in SIZES else ctypes.c_int32 if arg in INTS else ctypes.c_void_p)
            assert ctype == want, (name, arg)
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5
    # the header no longer says that the per-symbol coders have no select form
    assert "have no select form yet" not in HEADER.read_text()


def test_scratch_is_monotone_and_never_empty(lib):
    fn = getattr(lib, SCRATCH)
    sizes = [fn(n) for n in (0, 1, 2, 63, 64, 65, 1000, 1001, 1 << 20, (1 << 32) - 1)]
    assert sizes[0] > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # a piece's record: a range state (40 bytes), four 64-bit and five 32-bit fields
    assert fn(1000) >= fn(0) + 92 * 1000
    # the shared-table calls' scratch is what it was: 40 bytes per piece and 128
    assert lib.cst_ragged_select_scratch_bytes(1000) == 40 * 1000 + 128 == lib.cst_range_ragged_select_scratch_bytes(1000)


POINTERS = ("words", "word_offsets", "n_words", "a", "b", "sym_offsets", "chunk_offsets", "jump_pos", "jump_state", "jump_lower", "jump_range",
            "query_stream", "query_first", "query_count", "piece_offsets", "symbols_out", "out_offsets", "scratch", "status")


def _call(lib, name, cfg=(32, 64, 24), family=1, lo=-100, hi=100, null=(), stride=0, n_streams=1, interval=64, n_chunks=8, n_queries=1, n_pieces=8):
    """one call with HOST buffers behind every pointer: a call that passed its argument checks with n_queries > 0 would go on to the
    device, so only calls that must fail them, or that carry no query, are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in POINTERS}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    fam = (family,) if "family" in name else ()
    table = [p[k] for k in table_pointers(name)[1:]]
    return getattr(lib, name)(N.CoderConfig(*cfg), *fam, lo, hi, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["a"], p["b"],
                              p["sym_offsets"], n_streams, interval, p["chunk_offsets"], n_chunks, *table, p["query_stream"], p["query_first"],
                              p["query_count"], n_queries, p["piece_offsets"], n_pieces, p["symbols_out"], p["out_offsets"], p["scratch"],
                              p["status"], None)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad, ok = N.CST_ERR_INVALID_ARGUMENT, N.CST_OK
    table = table_pointers(name)
    no_table = dict(interval=0, null=table)
    for n_queries in (0, 1):
        # every refusal of the plain decode call: its required pointers, the preset, the support
        for pointer in ("words", "n_words", "a", "b", "sym_offsets", "symbols_out", "status"):
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
            assert _call(lib, name, interval=0, null=table + (pointer,), n_queries=n_queries) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_queries=n_queries) == bad          # neither offsets nor a stride
        for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
            assert _call(lib, name, cfg=cfg, n_queries=n_queries) == bad, cfg
        assert _call(lib, name, lo=5, hi=5, n_queries=n_queries) == bad and _call(lib, name, lo=5, hi=4, n_queries=n_queries) == bad
        assert _call(lib, name, cfg=(32, 64, 4), lo=0, hi=16, n_queries=n_queries) == N.CST_ERR_MODEL             # 17 symbols, 16 quantiles
        assert _call(lib, name, cfg=(16, 32, 12), lo=-3000, hi=3000, n_queries=n_queries, **no_table) == N.CST_ERR_MODEL
        # an interval that is no multiple of 16 (the encoders' tiles), or above 2^31 - 1
        for interval in (4, 8, 24, 63, 1 << 31, (1 << 31) + 16):
            assert _call(lib, name, interval=interval, n_queries=n_queries) == bad, interval
        # a table given only in part: an interval without all of its arrays, arrays without an interval
        for pointer in table:
            assert _call(lib, name, null=(pointer,), n_queries=n_queries) == bad, pointer
            assert _call(lib, name, interval=0, null=tuple(k for k in table if k != pointer), n_queries=n_queries) == bad, pointer
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
    if "family" in name:
        for family in (0, 3, -1):          # (the Gaussian has calls of its own)
            assert _call(lib, name, family=family) == bad and _call(lib, name, family=family, n_queries=0) == bad
    # no queries: CST_OK and nothing is launched, with a table, without one, whole documents, and whatever hides behind the query pointers
    assert _call(lib, name, n_queries=0) == ok
    assert _call(lib, name, n_queries=0, n_pieces=(1 << 32) - 1, n_chunks=(1 << 32) - 1, interval=(1 << 31) - 16) == ok
    assert _call(lib, name, n_queries=0, **no_table) == ok
    assert _call(lib, name, n_queries=0, interval=0, null=table + ("query_first", "query_count")) == ok
    assert _call(lib, name, n_queries=0, null=("query_stream", "piece_offsets", "out_offsets", "scratch", "query_first", "query_count")) == ok
    assert _call(lib, name, n_queries=0, n_streams=0) == ok


def test_batched_exposes_the_functions():
    pytest.importorskip("torch")
    from constriction_amd import batched
    tail = ["streams", "first", "count", "out"]
    for coder in ("ans", "range"):
        for family in ("gaussian", "laplace", "cauchy", "family"):
            fn = getattr(batched, f"{coder}_decode_{family}_ragged_select")
            plain = getattr(batched, f"{coder}_decode_{family}_ragged")
            assert callable(fn)
            if family in ("gaussian", "family"):
                sig = inspect.signature(fn)
                head = (["family"] if family == "family" else []) + ["encoded", "sym_offsets"]
                assert list(sig.parameters)[:len(head)] == head and list(sig.parameters)[-4:] == tail and len(sig.parameters) == len(head) + 8
                assert all(sig.parameters[k].default is None for k in ("first", "count", "out"))
                # the model's arguments are the plain decoder's
                assert list(sig.parameters)[:-4] == list(inspect.signature(plain).parameters)[:-2]
    # the shared-table calls keep their signatures
    for fn in (batched.ans_decode_ragged_select, batched.range_decode_ragged_select):
        assert list(inspect.signature(fn).parameters) == ["encoded", "model", "sym_offsets", "streams", "first", "count", "out"]


def test_batches_of_the_other_coder_are_refused():
    """judged first, on CPU tensors: the batch's coder, then the type of its jump table"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    ans_jump = batched.RaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64))
    range_jump = batched.RangeRaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    make = lambda coder, jump: batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, jump,
                                                   coder)
    args = (z(3, torch.int64), -10, 10, z(0, torch.float64), z(0, torch.float64), [0])
    for family in ("gaussian", "laplace", "cauchy"):
        ans_fn, range_fn = (getattr(batched, f"{coder}_decode_{family}_ragged_select") for coder in ("ans", "range"))
        with pytest.raises(ValueError, match="'ans'"):
            range_fn(make("ans", None), *args)
        with pytest.raises(ValueError, match="'range'"):
            ans_fn(make("range", None), *args)
        with pytest.raises(ValueError, match="jump points of another coder"):
            ans_fn(make("ans", range_jump), *args)
        with pytest.raises(ValueError, match="jump points of another coder"):
            range_fn(make("range", ans_jump), *args)
    with pytest.raises(ValueError, match="jump points of another coder"):
        batched.ans_decode_family_ragged_select("laplace", make("ans", range_jump), *args)
    # ... as in the shared-table calls, which share the query preparation
    with pytest.raises(ValueError, match="jump points of another coder"):
        batched.ans_decode_ragged_select(make("ans", range_jump), None, z(3, torch.int64), [0])
