"""GPU: constriction_amd.symbol, the drop-in for the reference's constriction.symbol (src/pybindings/symbol/), against the doc
vectors and a bit-level model of the reference's containers built on tests/huffman_ref.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import huffman_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DOC = json.loads((ROOT / "tests" / "golden" / "huffman_vectors.json").read_text())["doc_examples"]


@pytest.fixture(scope="module")
def S():
    from constriction_amd import symbol
    return symbol


def doc_trees(S):
    p = np.array(DOC["probabilities"], dtype=np.float32)
    return S.huffman.EncoderHuffmanTree(p), S.huffman.DecoderHuffmanTree(p)


def test_doc_example_queue(S, capsys):
    enc, dec = doc_trees(S)
    encoder = S.QueueEncoder()
    for x in DOC["message"]:
        encoder.encode_symbol(x, enc)
    compressed, bitrate = encoder.get_compressed()
    assert compressed.dtype == np.uint32 and compressed.tolist() == DOC["queue"]["words"] and bitrate == 48
    assert "QueueEncoder.get_compressed` has been renamed" in capsys.readouterr().out
    encoder.get_compressed()
    assert capsys.readouterr().out == ""                       # once per process
    decoder = S.QueueDecoder(compressed)
    assert [decoder.decode_symbol(dec) for _ in DOC["message"]] == DOC["message"]
    decoder2 = encoder.get_decoder()
    assert [decoder2.decode_symbol(dec) for _ in DOC["message"]] == DOC["message"]


def test_doc_example_stack(S, capsys):
    enc, dec = doc_trees(S)
    coder = S.StackCoder()
    for x in reversed(DOC["message"]):
        coder.encode_symbol(x, enc)
    compressed, bitrate = coder.get_compressed()
    assert compressed.tolist() == DOC["stack_encoded_in_reverse"]["words"] and bitrate == 48
    assert "StackCoder.get_compressed` has been renamed" in capsys.readouterr().out
    assert [coder.decode_symbol(dec) for _ in DOC["message"]] == DOC["message"]
    with pytest.raises(ValueError, match="Ran out of bits in compressed data."):
        coder.decode_symbol(dec)


def test_stack_from_compressed_finds_the_seal_at_the_highest_bit(S):
    # the reference's from_compressed takes the LOWEST set bit of 129455 for the seal and resumes from the wrong state
    # (src/symbol/mod.rs:478-497); the drop-in takes the highest, where the writer put it
    _, dec = doc_trees(S)
    coder = S.StackCoder(np.array(DOC["stack_encoded_in_reverse"]["words"], dtype=np.uint32))
    assert [coder.decode_symbol(dec) for _ in DOC["message"]] == DOC["message"]
    assert coder.get_compressed_and_bitrate()[1] == 0


def test_get_compressed_in_the_middle_changes_nothing(S):
    enc, _ = doc_trees(S)
    a, b = S.StackCoder(), S.StackCoder()
    qa, qb = S.QueueEncoder(), S.QueueEncoder()
    for i, x in enumerate(DOC["message"] * 3):
        for c in (a, b, qa, qb):
            c.encode_symbol(x, enc)
        if i % 5 == 2:
            a.get_compressed_and_bitrate()
            qa.get_compressed_and_bitrate()
    for x, y in ((a, b), (qa, qb)):
        wx, bx = x.get_compressed_and_bitrate()
        wy, by = y.get_compressed_and_bitrate()
        assert wx.tolist() == wy.tolist() and bx == by


class BitStack:
    """the reference's StackCoder at bit level"""

    def __init__(self, nodes):
        self.nodes, self.bits = nodes, []
        self.codes, self.ch, self.n = R.suffix_codewords(nodes), R.children(nodes), (len(nodes) + 1) // 2

    def encode(self, x):
        self.bits += list(self.codes[x])

    def decode(self):
        v = 2 * self.n - 2
        while v >= self.n:
            if not self.bits:
                return None
            v = self.ch[v - self.n][int(self.bits.pop())]
        return v

    def compressed(self):
        return R._words("".join(self.bits) + "1"), len(self.bits)


@pytest.mark.parametrize("f32", [False, True])
def test_bits_back_interleaving(S, f32):
    rng = np.random.default_rng(int(f32))
    p = rng.dirichlet(np.ones(37) * 0.4)
    p = p.astype(np.float32) if f32 else p
    enc, dec = S.huffman.EncoderHuffmanTree(p), S.huffman.DecoderHuffmanTree(p)
    model = BitStack(R.tree(p, f32))
    coder = S.StackCoder()
    for step in range(400):
        op = rng.integers(0, 3)
        if op < 2:
            x = int(rng.integers(0, 37))
            coder.encode_symbol(x, enc)
            model.encode(x)
        else:
            want = model.decode()
            if want is None:
                with pytest.raises(ValueError):
                    coder.decode_symbol(dec)
                model.bits = []
            else:
                assert coder.decode_symbol(dec) == want, step
        if step % 37 == 0:
            words, bits = coder.get_compressed_and_bitrate()
            assert (words.tolist(), bits) == model.compressed(), step
    words, bits = coder.get_compressed_and_bitrate()
    assert (words.tolist(), bits) == model.compressed()


def test_long_codewords_in_the_dropin(S):
    p = np.array([2.0 ** -i for i in range(1, 120)] + [2.0 ** -119])
    enc, dec = S.huffman.EncoderHuffmanTree(p), S.huffman.DecoderHuffmanTree(p)
    msg = [119, 0, 5, 118, 60, 119, 1]
    for make in (S.StackCoder, S.QueueEncoder):
        c = make()
        for x in (reversed(msg) if make is S.StackCoder else msg):
            c.encode_symbol(x, enc)
        words, bits = c.get_compressed_and_bitrate()
        nodes = R.tree(p, False)
        want = R.stack_encode(nodes, msg) if make is S.StackCoder else R.queue_encode(nodes, msg)
        assert (words.tolist(), bits) == want
        d = c if make is S.StackCoder else S.QueueDecoder(words)
        assert [d.decode_symbol(dec) for _ in msg] == msg


def test_errors(S):
    enc, dec = doc_trees(S)
    for c in (S.StackCoder(), S.QueueEncoder()):
        c.encode_symbol(1, enc)
        with pytest.raises(KeyError):
            c.encode_symbol(4, enc)
        with pytest.raises(OverflowError):
            c.encode_symbol(-1, enc)
        assert c.get_compressed_and_bitrate()[1] == 3            # "111": nothing else was appended
    with pytest.raises(ValueError, match="must not end in a zero word"):
        S.StackCoder(np.array([5, 0], dtype=np.uint32))
    with pytest.raises(TypeError):
        S.StackCoder(np.array([5, 1], dtype=np.int64))
    with pytest.raises(FloatingPointError):
        S.huffman.EncoderHuffmanTree(np.array([0.5, np.nan]))
    with pytest.raises(FloatingPointError):
        S.huffman.DecoderHuffmanTree(np.array([0.5, np.nan], dtype=np.float32))
    with pytest.raises(ValueError):
        S.huffman.EncoderHuffmanTree(np.array([0.5, -0.5]))
    q = S.QueueDecoder(np.array([], dtype=np.uint32))
    with pytest.raises(ValueError, match="Ran out of bits in compressed data."):
        q.decode_symbol(dec)
    q = S.QueueDecoder(np.array([0xFFFFFFFF], dtype=np.uint32))      # symbol 1 is "111" -- ten of them, then 2 bits
    assert [q.decode_symbol(dec) for _ in range(10)] == [1] * 10
    with pytest.raises(ValueError):
        q.decode_symbol(dec)
    s = S.StackCoder()
    with pytest.raises(ValueError):
        s.decode_symbol(dec)
    one = S.huffman.DecoderHuffmanTree(np.array([1.0]))
    assert S.StackCoder().decode_symbol(one) == 0               # a one-symbol alphabet reads no bits
