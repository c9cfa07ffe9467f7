"""`constriction.symbol.huffman`, computed on the MI355X: the reference's Huffman codebooks
(src/pybindings/symbol/huffman.rs).  Both trees come from the same construction (src/symbol/huffman.rs:62-116, 200-230);
each object holds the device codebook the coders of `constriction_amd.symbol` launch with."""
from __future__ import annotations

from ..batched import HuffmanCodebook


class _Tree:
    def __init__(self, probabilities):
        # float32 probabilities add in float32, float64 in float64; NaN -> FloatingPointError (pybindings/mod.rs:245-250)
        self._cb = HuffmanCodebook.from_probabilities(probabilities)

    def num_symbols(self) -> int:
        return self._cb.n_symbols


class EncoderHuffmanTree(_Tree):
    """A Huffman tree for encoding: `EncoderHuffmanTree(probabilities)`, probabilities a rank-1 float32 / float64 array over the
    symbols 0 .. len(probabilities) - 1 (nonnegative and finite; only their ratios matter)."""


class DecoderHuffmanTree(_Tree):
    """A Huffman tree for decoding, built from the same probabilities as its EncoderHuffmanTree."""
