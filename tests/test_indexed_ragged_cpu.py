"""CPU-only: what ragged indexed table coding (csrc/cst_indexed_ragged.hip, batched.{ans,range}_{encode,decode}_indexed_ragged; DESIGN.md
4.30) decides before any device call -- the argument errors of the eight cst_*_indexed_ragged[_jump] entry points, the ValueErrors of
the Python layer -- that the header, the ctypes binding and the Rust declarations list the new names, and that the oracle recipe for
jump tables (tests/persymbol_jump_oracle.py) holds for lists of TableModel.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from persymbol_jump_oracle import ans_table, range_table

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
NAMES = [f"cst_{c}_{d}_indexed_ragged{j}" for c in ("ans", "range") for d in ("encode", "decode") for j in ("", "_jump")]


@pytest.fixture(scope="module")
def N():
    from constriction_amd import build, _native
    build.build_library()
    _native.load_library()
    return _native


def test_the_names_are_everywhere(N):
    header = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    lib = N.load_library()
    assert len(NAMES) == 8
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


class FakeTableSet(C.Structure):
    """the first fields of csrc/cst_indexed.hpp's cst_table_set: enough for table_set_alive and the precision check.  With n_streams == 0
    nothing else of it is read, so the refusals can be told apart one by one without a device"""
    _fields_ = [("magic", C.c_uint32), ("precision", C.c_int32), ("rest", C.c_uint8 * 248)]


def live_looking(precision):
    return FakeTableSet(0x58495443, precision)


def calls(N, tables, cfg, n_streams=0, index_bytes=1, stride=16, interval=16, n_chunks=4, off=(), **null):
    """the eight entry points with dummy non-NULL pointers (nothing is dereferenced before the checks pass; where they pass, n_streams is
    0 and nothing is launched); null=dict(sym=1, ...) names the pointers to hand in as NULL; `off`: the entry points to leave out"""
    lib = N.load_library()
    buf = C.create_string_buffer(64)
    p = lambda name: None if null.get(name) else C.addressof(buf)
    t = None if tables is None else C.addressof(tables)
    woff = p("word_offsets") if null.get("use_word_offsets", True) else None
    out = {}
    for coder in ("ans", "range"):
        table_w = [p("jump_pos"), p("jump_a")] + ([p("jump_b")] if coder == "range" else [])
        out[f"{coder}_encode"] = lambda coder=coder: getattr(lib, f"cst_{coder}_encode_indexed_ragged")(
            cfg, t, p("sym"), p("idx"), index_bytes, p("sym_offsets"), n_streams, None, p("words"), woff, stride, p("n_words"), p("status"), None)
        out[f"{coder}_decode"] = lambda coder=coder: getattr(lib, f"cst_{coder}_decode_indexed_ragged")(
            cfg, t, p("words"), woff, stride, 64, p("n_words"), p("idx"), index_bytes, p("sym"), p("sym_offsets"), n_streams, None, p("status"), None)
        out[f"{coder}_encode_jump"] = lambda coder=coder, table_w=table_w: getattr(lib, f"cst_{coder}_encode_indexed_ragged_jump")(
            cfg, t, p("sym"), p("idx"), index_bytes, p("sym_offsets"), n_streams, None, p("words"), woff, stride, p("n_words"), interval,
            p("chunk_offsets"), *table_w, p("status"), None)
        out[f"{coder}_decode_jump"] = lambda coder=coder, table_w=table_w: getattr(lib, f"cst_{coder}_decode_indexed_ragged_jump")(
            cfg, t, p("words"), woff, stride, 64, p("n_words"), p("idx"), index_bytes, p("sym"), p("sym_offsets"), n_streams, interval,
            p("chunk_offsets"), n_chunks, *table_w, p("scratch"), p("status"), None)
    return {k: f() for k, f in out.items() if k not in off}


def test_argument_errors_come_before_the_device_and_no_streams_is_ok(N):
    cfg = N.CoderConfig(32, 64, 12)
    bad, ok = N.CST_ERR_INVALID_ARGUMENT, N.CST_OK
    all_bad = lambda got: set(got.values()) == {bad}
    # a NULL handle, or one that is no live table set: refused, never followed (with one stream to code: nothing may be launched)
    not_a_set = FakeTableSet(0, 12)
    for tables in (None, not_a_set):
        for n_streams in (0, 1):
            assert all_bad(calls(N, tables, cfg, n_streams=n_streams)), (tables, n_streams)
    # a handle that passes for live: n_streams == 0 is CST_OK for all eight, nothing launched ...
    live = live_looking(12)
    got = calls(N, live, cfg)
    assert len(got) == 8 and set(got.values()) == {ok}, got
    assert set(calls(N, live, cfg, index_bytes=4).values()) == {ok}
    assert set(calls(N, live, cfg, use_word_offsets=False, stride=16).values()) == {ok}        # slabs by stride
    # ... and every single refusal of the plain calls is told apart from it
    for name in ("sym", "idx", "sym_offsets", "words", "n_words", "status"):
        assert all_bad(calls(N, live, cfg, **{name: 1})), name
    for index_bytes in (0, 2, 3, 8, -1):
        assert all_bad(calls(N, live, cfg, index_bytes=index_bytes)), index_bytes
    for other in (N.CoderConfig(16, 32, 12), N.CoderConfig(32, 32, 12), N.CoderConfig(16, 64, 12)):
        assert all_bad(calls(N, live, other))
    for precision in (11, 13, 24):                                                              # not the set's
        assert all_bad(calls(N, live, N.CoderConfig(32, 64, precision))), precision
    assert all_bad(calls(N, live, cfg, use_word_offsets=False, stride=0))
    # the jump forms' own: every refusal of jump_table_bad, n_chunks_total > 2^32 - 1, a NULL scratch
    plain = ("ans_encode", "ans_decode", "range_encode", "range_decode")
    for interval in (0, 8, 17, 24, 2**31, 2**31 + 16):
        assert all_bad(calls(N, live, cfg, interval=interval, off=plain)), interval
    for interval in (16, 48, 2**31 - 16):
        assert set(calls(N, live, cfg, interval=interval, off=plain).values()) == {ok}, interval
    for name in ("chunk_offsets", "jump_pos", "jump_a"):
        assert all_bad(calls(N, live, cfg, off=plain, **{name: 1})), name
    got = calls(N, live, cfg, off=plain, jump_b=1)                                              # (the ANS table has no second array)
    assert got == {"ans_encode_jump": ok, "ans_decode_jump": ok, "range_encode_jump": bad, "range_decode_jump": bad}
    decoders = calls(N, live, cfg, n_chunks=2**32, off=plain)
    assert decoders["ans_decode_jump"] == bad and decoders["range_decode_jump"] == bad
    assert set(calls(N, live, cfg, n_chunks=2**32 - 1, off=plain).values()) == {ok}
    got = calls(N, live, cfg, off=plain, scratch=1)
    assert got == {"ans_encode_jump": ok, "ans_decode_jump": bad, "range_encode_jump": ok, "range_decode_jump": bad}
    # the table's refusals come first, as in every jump call: still INVALID_ARGUMENT with a handle that is none
    assert all_bad(calls(N, not_a_set, cfg, interval=8, off=plain))


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
    sym = torch.zeros(24, dtype=torch.int32)
    idx = torch.zeros(24, dtype=torch.uint8)
    off = torch.tensor([0, 8, 24], dtype=torch.int64)
    for coder in ("ans", "range"):
        enc, dec = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
        # jump_every is judged first: before the table set, the configuration and the tensors
        for jump_every in (8, 17, -16, "always", 2**31):
            with pytest.raises(ValueError, match="jump_every"):
                enc("no tensor", "no tensor", "no tensor", "no table set", (1, 2, 3), jump_every=jump_every)
        with pytest.raises(ValueError, match="TableSet"):
            enc(sym, idx, off, "not a table set", cfg)
        for config in ((16, 32, 12), (32, 64, 16), (32, 32, 12)):
            with pytest.raises(ValueError, match="config"):
                enc(sym, idx, off, tables, config)
        with pytest.raises(ValueError, match="config"):             # the default is (32, 64, 16): not this set's
            enc(sym, idx, off, tables)
        for bad_sym in (sym, sym.to(torch.int64), sym.reshape(3, 8), np.zeros(24, np.int32)):      # host memory at the least
            with pytest.raises(ValueError, match="symbols"):
                enc(bad_sym, idx, off, tables, cfg)
        # the index checks, on tensors that claim no device: dtype, shape, numel, device
        for bad_idx in (torch.zeros(23, dtype=torch.uint8), torch.zeros(25, dtype=torch.int32), torch.zeros((3, 8), dtype=torch.uint8),
                        torch.zeros(24, dtype=torch.int64), torch.zeros(24, dtype=torch.int8), torch.zeros(24, dtype=torch.float32),
                        np.zeros(24, np.uint8), idx):
            with pytest.raises(ValueError, match="indices"):
                B._indexed_ragged_args(24, torch.device("cpu"), bad_idx, tables, cfg)
        for bad_off in (off.to(torch.int32), off.reshape(1, 3), torch.zeros(0, dtype=torch.int64), [0, 8, 24], off):
            with pytest.raises(ValueError, match="sym_offsets"):
                B._indexed_ragged_offsets(bad_off, torch.device("cuda", 0))
        # decode: the table set, the batch, its coder, its jump table, its configuration; then the indices (host memory here)
        words, n_words = torch.zeros(64, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
        woff = torch.tensor([0, 32, 64], dtype=torch.int64)
        batch = lambda coder, jump=None, config=cfg: B.RaggedBatch(words, woff, n_words, n_words, config, None, jump, coder)
        other = "range" if coder == "ans" else "ans"
        chunk_off, pos, u64 = torch.tensor([0, 1, 3], dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
        own_jump = B.RaggedJump(16, chunk_off, pos, u64) if coder == "ans" else B.RangeRaggedJump(16, chunk_off, pos, u64, u64)
        other_jump = B.RangeRaggedJump(16, chunk_off, pos, u64, u64) if coder == "ans" else B.RaggedJump(16, chunk_off, pos, u64)
        with pytest.raises(ValueError, match="TableSet"):
            dec(batch(coder), idx, off, "not a table set")
        with pytest.raises(ValueError, match="RaggedBatch"):
            dec((words, n_words), idx, off, tables)
        with pytest.raises(ValueError, match="coder"):
            dec(batch(other), idx, off, tables)
        with pytest.raises(ValueError, match="another coder"):
            dec(batch(coder, other_jump), idx, off, tables)
        with pytest.raises(ValueError, match="precision of the table set"):
            dec(batch(coder, config=(32, 64, 16)), idx, off, tables)
        for b in (batch(coder), batch(coder, own_jump)):
            with pytest.raises(ValueError, match="indices"):
                dec(b, idx, off, tables)
            with pytest.raises(ValueError, match="indices"):
                dec(b, torch.zeros(24, dtype=torch.int64), off, tables)
    # the rectangular helper keeps its behaviour (tests/test_indexed_cpu.py pins it): flat indices are not a matrix's
    with pytest.raises(ValueError):
        B._indexed_args((3, 8), torch.device("cpu"), torch.zeros(24, dtype=torch.uint8), tables, cfg)


# ---- the oracle recipe of tests/test_gpu_indexed_ragged.py ----

def table_models(O, K, n, P, rng):
    """K tables over n symbols from needle-thin (one symbol holds 2^P - (n - 1)) to flat"""
    lo = -(n // 2)
    rows = []
    for k in range(K):
        w = np.ones(n, dtype=np.int64)
        rest = (1 << P) - n
        if k % 3 == 0:
            w[rng.integers(0, n)] += rest
        elif k % 3 == 1:
            w += rest // n
            w[rng.integers(0, n)] += rest - (rest // n) * n
        else:
            cut = np.sort(rng.integers(0, rest + 1, n - 1))
            w += np.diff(np.concatenate([[0], cut, [rest]]))
        rows.append(np.concatenate([[0], np.cumsum(w)]).astype(np.uint32))
    return lo, [O.TableModel(r, lo, P) for r in rows]


def range_seek_decode(words, pos, lower, rng_, models, P):
    """RangeDecoder::seek((pos, (lower, range))) + decode_symbols for W = 32, S = 64 (src/stream/queue.rs:911-926, 847-868, 968-1033),
    restated: the oracle's RangeDecoder has no seek"""
    M = (1 << 64) - 1
    point, read = 0, 0
    while pos < len(words) and read < 2:
        point = ((point << 32) | int(words[pos])) & M
        pos, read = pos + 1, read + 1
    if 0 < read < 2:
        point = (point << 32) & M
    out = []
    for m in models:
        scale = rng_ >> P
        q = ((point - lower) & M) // scale
        assert q < (1 << P)
        s, l, p = m.quantile(q)
        out.append(int(s))
        lower = (lower + scale * l) & M
        rng_ = scale * p
        if rng_ < (1 << 32):
            lower, rng_ = (lower << 32) & M, (rng_ << 32) & M
            point = (point << 32) & M
            if pos < len(words):
                point |= int(words[pos])
                pos += 1
    return out


@pytest.mark.parametrize("P", [8, 16, 24])
@pytest.mark.parametrize("every", [16, 48])
def test_chunkwise_oracle_equals_one_shot_for_table_model_lists(P, every):
    """tests/test_persymbol_ragged_jump_cpu.py::test_chunkwise_oracle_equals_one_shot with [TableModel(cdfs[k]) for k in indices]: the
    words of chunk-wise coding are the one-shot words, and seek + decode from EVERY table entry returns the chunk, for both coders"""
    from oracle import oracle as O
    cfg = (32, 64, P)
    rng = np.random.default_rng(every + P)
    K, n = 7, 16
    lo, tm = table_models(O, K, n, P, rng)
    for length in (1, 15, 16, 17, 49, 96, 700):
        idx = rng.integers(0, K, length)
        sym = (rng.integers(0, n, length) + lo).astype(np.int32)
        models = [tm[k] for k in idx]
        one = O.AnsCoder()
        one.encode_reverse(sym, models, P)
        words, table = ans_table(O, cfg, sym, models, every)
        assert words.tolist() == one.get_compressed().tolist()
        assert len(table) == -(-length // every) and table[0] == one.pos()
        for j, (pos, state) in enumerate(table):
            c = O.AnsCoder(words)
            c.seek(pos, state)
            assert c.decode(models[j * every: (j + 1) * every], P=P).tolist() == sym[j * every: (j + 1) * every].tolist()
        rone = O.RangeEncoder()
        rone.encode(sym, models, P)
        rwords, rtable = range_table(O, cfg, sym, models, every)
        assert rwords.tolist() == rone.get_compressed().tolist()
        assert len(rtable) == -(-length // every) and rtable[0] == (0, 0, (1 << 64) - 1)
        assert all(rtable[j][0] <= rtable[j + 1][0] <= len(rwords) for j in range(len(rtable) - 1))
        assert O.RangeDecoder(rwords).decode(models, P=P).tolist() == sym.tolist()
        for j, (pos, lower, rng_) in enumerate(rtable):
            assert range_seek_decode(rwords, pos, lower, rng_, models[j * every: (j + 1) * every], P) == sym[j * every: (j + 1) * every].tolist()
