"""GPU: `constriction_amd.symbol.exp_golomb.ExpGolomb` in the coders of `constriction_amd.symbol`, against the reference's doc example
(tests/golden/exp_golomb_vectors.json) and bit-level models of the containers built on tests/exp_golomb_ref.py and
tests/huffman_ref.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import exp_golomb_ref as R
import huffman_ref as H

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "exp_golomb_vectors.json").read_text())
DOC = GOLDEN["doc_example"]


@pytest.fixture(scope="module")
def S():
    from constriction_amd import symbol
    return symbol


def test_doc_example_queue(S):
    code = S.exp_golomb.ExpGolomb()
    encoder = S.QueueEncoder()
    for x in DOC["symbols"]:
        encoder.encode_symbol(x, code)
    compressed, bitrate = encoder.get_compressed_and_bitrate()
    assert compressed.dtype == np.uint32 and compressed.tolist() == [20740] and bitrate == 16
    assert R.read_bits(compressed.tolist(), "queue") == DOC["queue_bit_string"]
    decoder = encoder.get_decoder()
    assert [decoder.decode_symbol(code) for _ in range(4)] == DOC["symbols"]
    with pytest.raises(ValueError):                             # the zero padding is no codeword
        decoder.decode_symbol(code)


def test_doc_example_stack(S):
    code = S.exp_golomb.ExpGolomb(bits=32)
    coder = S.StackCoder()
    for x in reversed(DOC["symbols"]):
        coder.encode_symbol(x, code)
    compressed, bitrate = coder.get_compressed_and_bitrate()
    assert compressed.tolist() == [73866] and bitrate == 16
    assert [coder.decode_symbol(code) for _ in range(4)] == DOC["symbols"]
    assert coder.get_compressed_and_bitrate()[1] == 0
    with pytest.raises(ValueError):
        coder.decode_symbol(code)


def test_stack_resumed_from_words(S):
    code = S.exp_golomb.ExpGolomb()
    message = [3, 7, 0, 1, 0xFFFFFFFF, 100000, 0xFFFFFFFE, 0]
    words, bits = R.stack_encode(message)
    coder = S.StackCoder(np.array(words, dtype=np.uint32))
    assert coder.get_compressed_and_bitrate()[1] == bits
    assert [coder.decode_symbol(code) for _ in message[:5]] == message[:5]
    coder.encode_symbol(12345, code)
    assert coder.decode_symbol(code) == 12345
    assert [coder.decode_symbol(code) for _ in message[5:]] == message[5:]
    words, bits = coder.get_compressed_and_bitrate()
    assert (words.tolist(), bits) == ([1], 0)


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_every_width(S, bits):
    code = S.exp_golomb.ExpGolomb(bits)
    top = (1 << bits) - 1
    message = [0, top, 1, top - 1, top >> 1, (top >> 1) + 1, 2, top]
    q, s = S.QueueEncoder(), S.StackCoder()
    for x in message:
        q.encode_symbol(x, code)
    for x in reversed(message):
        s.encode_symbol(x, code)
    words, n_bits = q.get_compressed_and_bitrate()
    assert (words.tolist(), n_bits) == R.queue_encode(message, bits)
    decoder = S.QueueDecoder(words)
    assert [decoder.decode_symbol(code) for _ in message] == message
    words, n_bits = s.get_compressed_and_bitrate()
    assert (words.tolist(), n_bits) == R.stack_encode(message, bits)
    assert [s.decode_symbol(code) for _ in message] == message


def test_codebooks_alternate_on_one_container(S):
    rng = np.random.default_rng(8)
    p = rng.dirichlet(np.ones(19) * 0.5)
    enc, dec = S.huffman.EncoderHuffmanTree(p), S.huffman.DecoderHuffmanTree(p)
    nodes = H.tree(p, False)
    h_prefix, h_suffix = H.prefix_codewords(nodes), H.suffix_codewords(nodes)
    code = S.exp_golomb.ExpGolomb()
    # runs of one kind and single switches; (kind, symbol)
    kinds = [int(k) for k in rng.integers(0, 2, 60)]
    kinds[10:20] = [0] * 10
    kinds[30:38] = [1] * 8
    message = [(k, int(rng.integers(0, 19)) if k == 0 else int(rng.choice([0, 1, 5, 70000, 0xFFFFFFFF, 0x7FFFFFFF]))) for k in kinds]
    queue, stack = S.QueueEncoder(), S.StackCoder()
    for k, x in message:
        queue.encode_symbol(x, enc if k == 0 else code)
    for k, x in reversed(message):
        stack.encode_symbol(x, enc if k == 0 else code)
    q_bits = "".join(h_prefix[x] if k == 0 else R.prefix_codeword(x) for k, x in message)
    s_bits = "".join(h_suffix[x] if k == 0 else R.suffix_codeword(x) for k, x in reversed(message))
    words, n_bits = queue.get_compressed_and_bitrate()
    assert (words.tolist(), n_bits) == (R._words(q_bits), len(q_bits))
    decoder = queue.get_decoder()
    assert [decoder.decode_symbol(dec if k == 0 else code) for k, _ in message] == [x for _, x in message]
    words, n_bits = stack.get_compressed_and_bitrate()
    assert (words.tolist(), n_bits) == (R._words(s_bits + "1"), len(s_bits))
    assert [stack.decode_symbol(dec if k == 0 else code) for k, _ in message] == [x for _, x in message]
    assert stack.get_compressed_and_bitrate()[1] == 0


def test_error_types(S):
    code8, code = S.exp_golomb.ExpGolomb(8), S.exp_golomb.ExpGolomb()
    for c in (S.StackCoder(), S.QueueEncoder()):
        c.encode_symbol(2, code8)
        with pytest.raises(OverflowError):
            c.encode_symbol(256, code8)
        with pytest.raises(OverflowError):
            c.encode_symbol(1 << 32, code)
        with pytest.raises(OverflowError):
            c.encode_symbol(-1, code)
        with pytest.raises(TypeError):
            c.encode_symbol(1.5, code)
        with pytest.raises(TypeError):
            c.encode_symbol(1, "exp_golomb")
        assert c.get_compressed_and_bitrate()[1] == 3            # "011": nothing else was appended
    with pytest.raises(TypeError):
        S.StackCoder().decode_symbol(None)
    with pytest.raises(TypeError):
        S.QueueDecoder(np.array([1], dtype=np.uint32)).decode_symbol(3)
    # invalid codewords: ValueError, and the container stays where it was
    q = S.QueueDecoder(np.array([1 << 9, 0], dtype=np.uint32))      # nine zeros, then a one: too long for u8, symbol 511 for u32
    with pytest.raises(ValueError):
        q.decode_symbol(code8)
    assert q.decode_symbol(code) == 511
    with pytest.raises(ValueError):                                  # the bits run out in the zero run
        q.decode_symbol(code)
    s = S.StackCoder()
    with pytest.raises(ValueError):
        s.decode_symbol(code)
    s = S.StackCoder(np.array([0b1000000000_1], dtype=np.uint32))   # read from the seal down: nine zeros, then a one, then nothing
    with pytest.raises(ValueError):
        s.decode_symbol(code)
    assert s.get_compressed_and_bitrate()[0].tolist() == [0b1000000000_1]
