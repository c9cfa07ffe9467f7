"""CPU-only: what random access into ragged indexed batches (csrc/cst_indexed_ragged.hip, batched.{ans,range}_decode_indexed_ragged_select;
DESIGN.md 4.31) decides before any device call -- the argument errors of the two cst_*_decode_indexed_ragged_select entry points, told
apart one by one, the ValueErrors of the Python layer -- and that the header, the ctypes binding, the built library and the Rust
declarations list the new names.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
NAMES = [f"cst_{c}_decode_indexed_ragged_select" for c in ("ans", "range")]


@pytest.fixture(scope="module")
def N():
    from constriction_amd import build, _native
    build.build_library()
    _native.load_library()
    return _native


def test_the_names_are_everywhere(N):
    header = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    wrappers = (ROOT / "bindings" / "rust" / "src" / "lib.rs").read_text()
    lib = N.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert "ffi::%s(" % name in wrappers, name
    # the argument lists: 11 of the model block, 5 of the table, 6 of the queries, 5 of the output -- the range call has one more
    # (d_jump_range); no new size function
    assert len(N.SIGNATURES[NAMES[0]][1]) == 27 and len(N.SIGNATURES[NAMES[1]][1]) == 28
    assert "seek_and_decode_indexed_ragged" in wrappers
    assert not any("indexed" in n and "scratch_bytes" in n for n in N.SIGNATURES)
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


class FakeTableSet(C.Structure):
    """the first fields of csrc/cst_indexed.hpp's cst_table_set: enough for table_set_alive and the precision check.  The refusals all
    come before anything else of it is read, and where the arguments pass n_queries is 0 and nothing is launched"""
    _fields_ = [("magic", C.c_uint32), ("precision", C.c_int32), ("rest", C.c_uint8 * 248)]


def live_looking(precision):
    return FakeTableSet(0x58495443, precision)


def calls(N, tables, cfg, n_streams=0, n_queries=0, index_bytes=1, stride=16, interval=16, n_chunks=4, n_pieces=4, table=True, **null):
    """both entry points with dummy non-NULL pointers (nothing is dereferenced before the checks pass; where they pass, n_queries is 0
    and nothing is launched); null=dict(idx=1, ...) names the pointers to hand in as NULL; table=False: no interval and no table array
    but those that `keep` names"""
    lib = N.load_library()
    buf = C.create_string_buffer(64)
    p = lambda name: None if null.get(name) else C.addressof(buf)
    t = None if tables is None else C.addressof(tables)
    woff = p("word_offsets") if null.get("use_word_offsets", True) else None
    keep = null.get("keep", ())
    tp = lambda name: p(name) if table or name in keep else None
    out = {}
    for coder in ("ans", "range"):
        table_w = [tp("jump_pos"), tp("jump_a")] + ([tp("jump_b")] if coder == "range" else [])
        out[coder] = getattr(lib, f"cst_{coder}_decode_indexed_ragged_select")(
            cfg, t, p("words"), woff, stride, 64, p("n_words"), p("idx"), index_bytes, p("sym_offsets"), n_streams,
            interval if table or "interval" in keep else 0, tp("chunk_offsets"), n_chunks, *table_w,
            p("query_stream"), p("query_first"), p("query_count"), n_queries, p("piece_offsets"), n_pieces, p("out"), p("out_offsets"),
            p("scratch"), p("status"), None)
    return out


def test_argument_errors_come_before_the_device_and_no_queries_is_ok(N):
    cfg = N.CoderConfig(32, 64, 12)
    bad, ok = N.CST_ERR_INVALID_ARGUMENT, N.CST_OK
    all_bad = lambda got: set(got.values()) == {bad}
    all_ok = lambda got: set(got.values()) == {ok}
    # a NULL handle, or one that is no live table set: refused, never followed (with queries to run: nothing may be launched)
    not_a_set = FakeTableSet(0, 12)
    for tables in (None, not_a_set):
        for n_queries in (0, 1):
            for table in (True, False):
                assert all_bad(calls(N, tables, cfg, n_queries=n_queries, table=table)), (tables, n_queries, table)
    # a handle that passes for live: n_queries == 0 is CST_OK, with and without a table, nothing launched ...
    live = live_looking(12)
    for table in (True, False):
        assert all_ok(calls(N, live, cfg, table=table)), table
        assert all_ok(calls(N, live, cfg, table=table, index_bytes=4))
        assert all_ok(calls(N, live, cfg, table=table, use_word_offsets=False, stride=16))        # slabs by stride
        assert all_ok(calls(N, live, cfg, table=table, n_streams=5))                               # (streams, but no queries)
        assert all_ok(calls(N, live, cfg, table=table, query_first=1, query_count=1))             # whole streams
        # (with no queries the query arrays, the output offsets and the scratch are not asked for)
        assert all_ok(calls(N, live, cfg, table=table, query_stream=1, piece_offsets=1, out_offsets=1, scratch=1))
        # ... and every single refusal of the plain decode is told apart from it (d_symbols_out in the place of d_symbols)
        for name in ("out", "idx", "sym_offsets", "words", "n_words", "status"):
            assert all_bad(calls(N, live, cfg, table=table, **{name: 1})), name
        for index_bytes in (0, 2, 3, 8, -1):
            assert all_bad(calls(N, live, cfg, table=table, index_bytes=index_bytes)), index_bytes
        for other in (N.CoderConfig(16, 32, 12), N.CoderConfig(32, 32, 12), N.CoderConfig(16, 64, 12)):
            assert all_bad(calls(N, live, other, table=table))
        for precision in (11, 13, 24):                                                             # not the set's
            assert all_bad(calls(N, live, N.CoderConfig(32, 64, precision), table=table)), precision
        assert all_bad(calls(N, live, cfg, table=table, use_word_offsets=False, stride=0))
        assert all_bad(calls(N, live, cfg, table=table, n_streams=2**32))
        assert all_ok(calls(N, live, cfg, table=table, n_streams=2**32 - 1))
        # the select calls' own
        assert all_bad(calls(N, live, cfg, table=table, n_pieces=2**32))
        assert all_ok(calls(N, live, cfg, table=table, n_pieces=2**32 - 1))
        assert all_bad(calls(N, live, cfg, table=table, query_first=1))                            # exactly one of the two
        assert all_bad(calls(N, live, cfg, table=table, query_count=1))
        for name in ("query_stream", "piece_offsets", "out_offsets", "scratch"):                   # with queries: each of the four
            assert all_bad(calls(N, live, cfg, table=table, n_queries=1, **{name: 1})), name
    # with a table: every refusal of the _jump decoders
    for interval in (8, 17, 24, 2**31, 2**31 + 16):
        assert all_bad(calls(N, live, cfg, interval=interval)), interval
    for interval in (16, 48, 2**31 - 16):
        assert all_ok(calls(N, live, cfg, interval=interval)), interval
    for name in ("chunk_offsets", "jump_pos", "jump_a"):
        assert all_bad(calls(N, live, cfg, **{name: 1})), name
    assert calls(N, live, cfg, jump_b=1) == {"ans": ok, "range": bad}                              # (the ANS table has no second array)
    assert all_bad(calls(N, live, cfg, n_chunks=2**32))
    assert all_ok(calls(N, live, cfg, n_chunks=2**32 - 1))
    # table arrays without an interval, one by one; an interval without arrays
    for name in ("chunk_offsets", "jump_pos", "jump_a"):
        assert all_bad(calls(N, live, cfg, table=False, keep=(name,))), name
    assert calls(N, live, cfg, table=False, keep=("jump_b",)) == {"ans": ok, "range": bad}         # (no such argument in the ANS call)
    assert all_bad(calls(N, live, cfg, table=False, keep=("interval",)))
    # without a table n_chunks_total says nothing
    assert all_ok(calls(N, live, cfg, table=False, n_chunks=2**32))
    # the table's refusals come first, as in every jump call: still INVALID_ARGUMENT with a handle that is none
    assert all_bad(calls(N, not_a_set, cfg, interval=8))


def cdfs_of(k, n, p):
    """k valid rows: row r gives symbol r % n all the weight the others leave"""
    rows = np.zeros((k, n + 1), dtype=np.uint32)
    for r in range(k):
        prob = np.ones(n, dtype=np.int64)
        prob[r % n] = (1 << p) - (n - 1)
        rows[r, 1:] = np.cumsum(prob)
    return rows


def test_python_layer_value_errors_need_no_device(N):
    torch = pytest.importorskip("torch")
    from constriction_amd import batched as B
    tables = B.TableSet(None, cdfs_of(4, 5, 12), 0, 12)              # no handle: the checks below come before it is used
    cfg = (32, 64, 12)
    idx = torch.zeros(24, dtype=torch.uint8)
    off = torch.tensor([0, 8, 24], dtype=torch.int64)
    words, n_words = torch.zeros(64, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    woff = torch.tensor([0, 32, 64], dtype=torch.int64)
    chunk_off, pos, u64 = torch.tensor([0, 1, 3], dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    for coder in ("ans", "range"):
        sel = getattr(B, f"{coder}_decode_indexed_ragged_select")
        batch = lambda coder, jump=None, config=cfg: B.RaggedBatch(words, woff, n_words, n_words, config, None, jump, coder)
        other = "range" if coder == "ans" else "ans"
        own_jump = B.RaggedJump(16, chunk_off, pos, u64) if coder == "ans" else B.RangeRaggedJump(16, chunk_off, pos, u64, u64)
        other_jump = B.RangeRaggedJump(16, chunk_off, pos, u64, u64) if coder == "ans" else B.RaggedJump(16, chunk_off, pos, u64)
        # the table set, the batch, its coder, its jump table, its configuration; then the indices (host memory here)
        with pytest.raises(ValueError, match="TableSet"):
            sel(batch(coder), idx, off, "not a table set", [0])
        with pytest.raises(ValueError, match="RaggedBatch"):
            sel((words, n_words), idx, off, tables, [0])
        with pytest.raises(ValueError, match="coder"):
            sel(batch(other), idx, off, tables, [0])
        with pytest.raises(ValueError, match="another coder"):
            sel(batch(coder, other_jump), idx, off, tables, [0])
        for config in ((32, 64, 16), (16, 32, 12), (32, 32, 12)):
            with pytest.raises(ValueError, match="precision of the table set"):
                sel(batch(coder, config=config), idx, off, tables, [0])
        for b in (batch(coder), batch(coder, own_jump)):
            with pytest.raises(ValueError, match="indices"):        # the right type, in host memory
                sel(b, idx, off, tables, [0], [0], [4])
            for bad_idx in (torch.zeros(24, dtype=torch.int64), torch.zeros(24, dtype=torch.int8), torch.zeros(24, dtype=torch.float32),
                            torch.zeros((3, 8), dtype=torch.uint8), np.zeros(24, np.uint8)):
                with pytest.raises(ValueError, match="indices"):
                    sel(b, bad_idx, off, tables, [0])
