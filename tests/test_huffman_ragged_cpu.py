"""CPU-only: the host side of the ragged Huffman entry points (cst_huffman_count_bits, cst_huffman_{encode,decode}_ragged and their
_jump forms) -- every argument error, which must be reported before a device is touched (there is none here) -- and the jump
table's two formulas on the reference's doc example, from the plain-Python restatement in tests/huffman_ref.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import huffman_ref as R

ROOT = Path(__file__).resolve().parent.parent
DOC = json.loads((ROOT / "tests" / "golden" / "huffman_vectors.json").read_text())["doc_examples"]
STACK, QUEUE = 0, 1
INVALID = -1     # CST_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native, build
    build.build_library()
    assert _native.CST_ERR_INVALID_ARGUMENT == INVALID
    return _native.load_library()


@pytest.fixture(scope="module")
def handles():
    """(something that passes for a codebook as far as the argument checks look -- its tag and an alphabet of 4 -- , something that does
    not, a host buffer to stand for every device pointer: no check may follow any of them)"""
    book = np.zeros(32, dtype=np.uint32)
    book[0], book[1] = 0x48554646, 4
    return book, np.zeros(32, dtype=np.uint32), np.zeros(64, dtype=np.uint64)


def _count_args(book, p):
    return dict(codebook=book, d_symbols=p, symbol_bytes=4, d_sym_offsets=p, n_streams=3, n_per_stream=0, d_n_bits=p, stream=None)


def _encode_args(book, p):
    return dict(codebook=book, semantics=STACK, d_symbols=p, symbol_bytes=4, d_sym_offsets=p, n_streams=3, d_words=p, d_word_offsets=p,
                stride_words=0, d_n_words=p, d_n_bits=p, d_status=p, stream=None)


def _decode_args(book, p):
    return dict(codebook=book, semantics=QUEUE, d_words=p, d_word_offsets=p, stride_words=0, words_capacity=64, d_n_words=p, d_symbols=p,
                symbol_bytes=4, d_sym_offsets=p, n_streams=3, d_status=p, stream=None)


def _encode_jump_args(book, p):
    a = _encode_args(book, p)
    status, stream = a.pop("d_status"), a.pop("stream")
    a.update(jump_interval=32, d_chunk_offsets=p, d_jump_bits=p, d_status=status, stream=stream)
    return a


def _decode_jump_args(book, p):
    a = _decode_args(book, p)
    status, stream = a.pop("d_status"), a.pop("stream")
    a.update(jump_interval=64, d_chunk_offsets=p, n_chunks_total=5, d_jump_bits=p, d_status=status, stream=stream)
    return a


CALLS = {"cst_huffman_count_bits": (_count_args, ["codebook", "d_n_bits"]),
         "cst_huffman_encode_ragged": (_encode_args, ["codebook", "d_symbols", "d_sym_offsets", "d_words", "d_n_words", "d_status"]),
         "cst_huffman_decode_ragged": (_decode_args, ["codebook", "d_words", "d_n_words", "d_symbols", "d_sym_offsets", "d_status"]),
         "cst_huffman_encode_ragged_jump": (_encode_jump_args, ["codebook", "d_symbols", "d_sym_offsets", "d_words", "d_n_words", "d_status",
                                                                "d_chunk_offsets", "d_jump_bits"]),
         "cst_huffman_decode_ragged_jump": (_decode_jump_args, ["codebook", "d_words", "d_n_words", "d_symbols", "d_sym_offsets", "d_status",
                                                                "d_chunk_offsets", "d_jump_bits"])}


def _call(lib, name, args):
    def raw(v):
        return v.ctypes.data if isinstance(v, np.ndarray) else v
    return getattr(lib, name)(*[raw(v) for v in args.values()])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_argument_errors_come_before_any_device_call(lib, handles, name):
    book, not_a_book, p = handles
    make, must_not_be_null = CALLS[name]
    for arg in must_not_be_null:
        assert _call(lib, name, {**make(book, p), arg: None}) == INVALID, (name, arg)
    assert _call(lib, name, {**make(book, p), "symbol_bytes": 2}) == INVALID
    assert _call(lib, name, {**make(book, p), "symbol_bytes": 0}) == INVALID
    assert _call(lib, name, {**make(book, p), "codebook": not_a_book}) == INVALID
    if "semantics" in make(book, p):
        assert _call(lib, name, {**make(book, p), "semantics": 2}) == INVALID
        assert _call(lib, name, {**make(book, p), "semantics": -1}) == INVALID
    if "jump_interval" in make(book, p):
        for interval in (0, 33, 16, 1 << 31):
            assert _call(lib, name, {**make(book, p), "jump_interval": interval}) == INVALID, interval
    if name == "cst_huffman_count_bits":        # no symbols at all is fine only for a matrix without columns
        assert _call(lib, name, {**make(book, p), "d_symbols": None}) == INVALID
        assert _call(lib, name, {**make(book, p), "d_symbols": None, "d_sym_offsets": None, "n_per_stream": 5}) == INVALID


def test_uint8_symbols_need_a_small_alphabet(lib, handles):
    book, _, p = handles
    big = book.copy()
    big[1] = 257
    for name in ("cst_huffman_decode_ragged", "cst_huffman_decode_ragged_jump"):
        assert _call(lib, name, {**CALLS[name][0](big, p), "symbol_bytes": 1}) == INVALID


def test_signatures_are_registered():
    from constriction_amd import _native as N
    for name in CALLS:
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == len(CALLS[name][0](None, None))


def jump_table(codes, message, interval, semantics):
    """the table's two formulas: queue the bits of message[: j I], stack the bits of message[j I :]"""
    chunks = -(-len(message) // interval)
    if semantics == "queue":
        return [len("".join(codes[x] for x in message[: j * interval])) for j in range(chunks)]
    return [len("".join(codes[x] for x in message[j * interval:])) for j in range(chunks)]


@pytest.mark.parametrize("interval", [1, 4, 5, 19, 32])
def test_table_formulas_on_the_doc_example(lib, interval):
    assert hasattr(lib, "cst_huffman_encode_ragged_jump")              # the call that writes the table these formulas describe
    nodes = R.tree(np.array(DOC["probabilities"], dtype=np.float32), True)
    msg = DOC["message"]
    prefix, suffix = R.prefix_codewords(nodes), R.suffix_codewords(nodes)
    chunks = [msg[i: i + interval] for i in range(0, len(msg), interval)]
    for semantics, codes, enc, want in (("queue", prefix, R.queue_encode, DOC["queue"]), ("stack", suffix, R.stack_encode, DOC["stack_encoded_in_reverse"])):
        words, bitrate = enc(nodes, msg)
        assert words == want["words"] and bitrate == want["bitrate"]
        chunk_bits = [sum(len(codes[x]) for x in c) for c in chunks]
        assert sum(chunk_bits) == want["bitrate"]                      # the chunk-wise sums reproduce the bitrate
        table = jump_table(codes, msg, interval, semantics)
        if semantics == "queue":
            assert table == [sum(chunk_bits[:j]) for j in range(len(chunks))] and table[0] == 0
        else:
            assert table == [sum(chunk_bits[j:]) for j in range(len(chunks))] and table[0] == want["bitrate"]
        # a reader that starts at entry j finds chunk j's symbols there: upwards in a queue, downwards in a stack
        bits = "".join(format(w, "032b")[::-1] for w in words)
        for j, c in enumerate(chunks):
            stream = bits[table[j]:] if semantics == "queue" else bits[: table[j]][::-1]
            got, pos = [], 0
            ch, n = R.children(nodes), len(DOC["probabilities"])
            for _ in c:
                v = 2 * n - 2
                while v >= n:
                    v = ch[v - n][int(stream[pos])]
                    pos += 1
                got.append(v)
            assert got == c and pos == chunk_bits[j]
