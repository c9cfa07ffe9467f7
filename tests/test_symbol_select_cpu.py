"""CPU-only: the host side of the Exp-Golomb jump calls and of the two symbol-code select calls (cst_exp_golomb_{encode,decode}_ragged_jump,
cst_{huffman,exp_golomb}_decode_ragged_select) -- every argument error, which must be reported before a device is touched (there is
none here) -- the Exp-Golomb jump table's two formulas from the plain-Python restatement in tests/exp_golomb_ref.py, and the Python
layer's own argument checks."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import exp_golomb_ref as R

ROOT = Path(__file__).resolve().parent.parent
DOC = json.loads((ROOT / "tests" / "golden" / "exp_golomb_vectors.json").read_text())["doc_example"]
STACK, QUEUE = 0, 1
OK, INVALID = 0, -1     # CST_OK, CST_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native, build
    build.build_library()
    assert _native.CST_ERR_INVALID_ARGUMENT == INVALID and _native.CST_OK == OK
    return _native.load_library()


@pytest.fixture(scope="module")
def handles():
    """(something that passes for a codebook as far as the argument checks look -- its tag and an alphabet of 4 -- , something that does
    not, a host buffer to stand for every device pointer: no check may follow any of them)"""
    book = np.zeros(32, dtype=np.uint32)
    book[0], book[1] = 0x48554646, 4
    return book, np.zeros(32, dtype=np.uint32), np.zeros(64, dtype=np.uint64)


def _encode_jump_args(book, p):
    return dict(semantics=STACK, d_symbols=p, symbol_bytes=4, d_sym_offsets=p, n_streams=3, d_words=p, d_word_offsets=p, stride_words=0,
                d_n_words=p, d_n_bits=p, jump_interval=32, d_chunk_offsets=p, d_jump_bits=p, d_status=p, stream=None)


def _decode_jump_args(book, p):
    return dict(semantics=QUEUE, d_words=p, d_word_offsets=p, stride_words=0, words_capacity=64, d_n_words=p, d_symbols=p, symbol_bytes=2,
                d_sym_offsets=p, n_streams=3, jump_interval=64, d_chunk_offsets=p, n_chunks_total=5, d_jump_bits=p, d_status=p, stream=None)


def _select_args(book, p):
    return dict(semantics=QUEUE, d_words=p, d_word_offsets=p, stride_words=0, words_capacity=64, d_n_words=p, d_sym_offsets=p, n_streams=3,
                jump_interval=64, d_chunk_offsets=p, n_chunks_total=5, d_jump_bits=p, d_query_stream=p, d_query_first=p, d_query_count=p,
                n_queries=2, d_piece_offsets=p, n_pieces_total=4, d_symbols_out=p, symbol_bytes=4, d_out_offsets=p, d_scratch=p, d_status=p,
                stream=None)


def _huffman_select_args(book, p):
    return dict(codebook=book, **_select_args(book, p))


# name -> (arguments, pointers that must never be NULL, symbol widths that are none)
CALLS = {"cst_exp_golomb_encode_ragged_jump": (_encode_jump_args, ["d_symbols", "d_sym_offsets", "d_words", "d_n_words", "d_status",
                                                                   "d_chunk_offsets", "d_jump_bits"], (0, 3, 8)),
         "cst_exp_golomb_decode_ragged_jump": (_decode_jump_args, ["d_words", "d_n_words", "d_symbols", "d_sym_offsets", "d_status",
                                                                   "d_chunk_offsets", "d_jump_bits"], (0, 3, 8)),
         "cst_exp_golomb_decode_ragged_select": (_select_args, ["d_words", "d_n_words", "d_sym_offsets"], (0, 3, 8)),
         "cst_huffman_decode_ragged_select": (_huffman_select_args, ["codebook", "d_words", "d_n_words", "d_sym_offsets"], (0, 2, 8))}
SELECT = [n for n in CALLS if n.endswith("_select")]


def _call(lib, name, args):
    def raw(v):
        return v.ctypes.data if isinstance(v, np.ndarray) else v
    return getattr(lib, name)(*[raw(v) for v in args.values()])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_argument_errors_come_before_any_device_call(lib, handles, name):
    book, not_a_book, p = handles
    make, must_not_be_null, bad_widths = CALLS[name]
    for arg in must_not_be_null:
        assert _call(lib, name, {**make(book, p), arg: None}) == INVALID, (name, arg)
    for width in bad_widths:
        assert _call(lib, name, {**make(book, p), "symbol_bytes": width}) == INVALID, width
    for semantics in (2, -1):
        assert _call(lib, name, {**make(book, p), "semantics": semantics}) == INVALID
    if "codebook" in make(book, p):
        assert _call(lib, name, {**make(book, p), "codebook": not_a_book}) == INVALID
        big = book.copy()
        big[1] = 257                                 # uint8 symbols need a small alphabet
        assert _call(lib, name, {**make(big, p), "symbol_bytes": 1}) == INVALID
    intervals = (33, 16, 1 << 31) if name in SELECT else (0, 33, 16, 1 << 31)
    for interval in intervals:
        assert _call(lib, name, {**make(book, p), "jump_interval": interval}) == INVALID, interval


@pytest.mark.parametrize("name", SELECT)
def test_select_argument_errors(lib, handles, name):
    book, _, p = handles
    make = CALLS[name][0]
    # a table given in part: an interval without its arrays, arrays without an interval, one array of the two
    for change in ({"d_chunk_offsets": None}, {"d_jump_bits": None}, {"jump_interval": 0}, {"d_chunk_offsets": None, "d_jump_bits": None},
                   {"jump_interval": 0, "d_chunk_offsets": None}, {"jump_interval": 0, "d_jump_bits": None}):
        assert _call(lib, name, {**make(book, p), **change}) == INVALID, change
    assert _call(lib, name, {**make(book, p), "n_chunks_total": 1 << 32}) == INVALID
    assert _call(lib, name, {**make(book, p), "n_pieces_total": 1 << 32}) == INVALID
    assert _call(lib, name, {**make(book, p), "d_query_first": None}) == INVALID
    assert _call(lib, name, {**make(book, p), "d_query_count": None}) == INVALID
    for arg in ("d_query_stream", "d_piece_offsets", "d_symbols_out", "d_out_offsets", "d_scratch", "d_status"):
        assert _call(lib, name, {**make(book, p), arg: None}) == INVALID, arg
    # no queries: nothing to do, with or without a table and whatever the query pointers are -- but the batch is still judged
    none = {"n_queries": 0, "d_query_stream": None, "d_piece_offsets": None, "d_symbols_out": None, "d_out_offsets": None, "d_scratch": None,
            "d_status": None, "d_query_first": None, "d_query_count": None}
    assert _call(lib, name, {**make(book, p), **none}) == OK
    assert _call(lib, name, {**make(book, p), **none, "jump_interval": 0, "d_chunk_offsets": None, "d_jump_bits": None}) == OK
    assert _call(lib, name, {**make(book, p), **none, "jump_interval": 48}) == INVALID
    assert _call(lib, name, {**make(book, p), **none, "d_words": None}) == INVALID


def test_signatures_are_registered():
    from constriction_amd import _native as N
    for name in CALLS:
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == len(CALLS[name][0](None, None))


def jump_table(message, interval, semantics, B):
    """the table's two formulas: queue the bits of message[: j I], stack the bits of message[j I :]"""
    chunks = -(-len(message) // interval)
    if semantics == "queue":
        return [len(R.queue_bits(message[: j * interval], B)) for j in range(chunks)]
    return [len(R.stack_bits(message[j * interval:], B)) for j in range(chunks)]


MESSAGES = [(DOC["symbols"], DOC["bits"]), ([0, 2 ** 17 - 2, 2 ** 17 - 1, 2 ** 32 - 1], 32), ([0, 254, 255, 7], 8), ([65535, 65534, 0, 1, 2], 16)]


@pytest.mark.parametrize("interval", [1, 2, 3, 32])
@pytest.mark.parametrize("message,B", MESSAGES)
def test_table_formulas(lib, message, B, interval):
    assert hasattr(lib, "cst_exp_golomb_encode_ragged_jump")           # the call that writes the table these formulas describe
    chunks = [message[i: i + interval] for i in range(0, len(message), interval)]
    chunk_bits = [sum(len(R.prefix_codeword(x, B)) for x in c) for c in chunks]
    for semantics, enc in (("queue", R.queue_encode), ("stack", R.stack_encode)):
        words, n_bits = enc(message, B)
        assert sum(chunk_bits) == n_bits
        table = jump_table(message, interval, semantics, B)
        if semantics == "queue":
            assert table == [sum(chunk_bits[:j]) for j in range(len(chunks))] and table[0] == 0          # the prefix bit sums
        else:
            assert table == [sum(chunk_bits[j:]) for j in range(len(chunks))] and table[0] == n_bits     # the suffix bit sums; the seal
        # a reader that starts at entry j finds chunk j's symbols there: upwards in a queue, downwards in a stack
        bits = R._bits(words)
        for j, c in enumerate(chunks):
            stream = bits[table[j]:] if semantics == "queue" else bits[: table[j]][::-1]
            pos = 0
            for x in c:
                sym, pos = R.decode_symbol(stream, pos, B)
                assert sym == x
            assert pos == chunk_bits[j]


def test_doc_example_is_the_golden_one():
    words, n_bits = R.queue_encode(DOC["symbols"], DOC["bits"])
    assert R._bits(words) == DOC["queue_bit_string"] and n_bits == sum(len(R.prefix_codeword(x)) for x in DOC["symbols"]) == 16


# ---- the Python layer: every check below raises before any device call ----

def host_batch(B, coder, jump=None):
    z32, z64 = torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    return B.RaggedBatch(z32, z64, z32[:2], z32[:2], ("queue", torch.int32), coder=coder, jump=jump)


def test_python_argument_checks():
    from constriction_amd import batched as B
    sym, offsets = torch.zeros(8, dtype=torch.int32), torch.tensor([0, 4, 8])
    for bad in (33, 16, -32, 1 << 31, "sometimes"):
        with pytest.raises(ValueError, match="jump_every"):
            B.exp_golomb_encode_ragged(sym, offsets, "queue", jump_every=bad)
    ans_jump = B.RaggedJump(32, offsets, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
    # the wrong coder
    for coder in ("ans", "range", "huffman"):
        with pytest.raises(ValueError, match="'exp_golomb' decoder"):
            B.exp_golomb_decode_ragged_select(host_batch(B, coder), offsets, [0])
    for coder in ("ans", "range", "exp_golomb"):
        with pytest.raises(ValueError, match="'huffman' decoder"):
            B.huffman_decode_ragged_select(host_batch(B, coder), None, offsets, [0])
    for coder in ("huffman", "exp_golomb"):
        with pytest.raises(ValueError, match="'ans' decoder"):
            B.ans_decode_ragged_select(host_batch(B, coder), None, offsets, [0])
        with pytest.raises(ValueError, match="'range' decoder"):
            B.range_decode_ragged_select(host_batch(B, coder), None, offsets, [0])
    # the wrong jump type
    with pytest.raises(ValueError, match="jump points of another coder"):
        B.exp_golomb_decode_ragged_select(host_batch(B, "exp_golomb", ans_jump), offsets, [0])
    with pytest.raises(ValueError, match="jump points of another coder"):
        B.huffman_decode_ragged_select(host_batch(B, "huffman", ans_jump), None, offsets, [0])
