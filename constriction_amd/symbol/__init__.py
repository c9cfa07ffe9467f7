"""`constriction.symbol`, computed on the MI355X: `StackCoder`, `QueueEncoder`, `QueueDecoder`, the `huffman` codebooks and the
`exp_golomb` code.

Mirror of src/pybindings/symbol/mod.rs (same constructors, method names, return dtypes and error types).  Each object keeps
the reference's bit container on the host -- whole u32 words plus the partial word and its bit count (src/symbol/mod.rs:
StackCoder / QueueEncoder / QueueDecoder) -- and all coding runs in the batched kernels (csrc/cst_huffman.hip) as one-stream
launches that continue from that container (`d_cont`); an `exp_golomb.ExpGolomb` codebook runs the kernels of
csrc/cst_exp_golomb.hip on the same container, and the two kinds may alternate.  Consecutive `encode_symbol` calls are buffered and coded in one launch
when the container is observed (`get_compressed*`, `decode_symbol`, `get_decoder`) or the codebook changes; every
`decode_symbol` is one device round trip.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from ..batched import _ptr, _stream_ptr
from . import exp_golomb, huffman  # noqa: F401
from .exp_golomb import ExpGolomb
from .huffman import DecoderHuffmanTree, EncoderHuffmanTree

_OUT_OF_DATA = "Ran out of bits in compressed data."
_INVALID_CODEWORD = "Invalid codeword for Exp-Golomb code."
_EG_DTYPES = {1: (np.uint8, np.uint8), 2: (np.uint16, np.int16), 4: (np.uint32, np.int32)}     # symbol_bytes -> (unsigned, tensor type)


def _as_words(compressed) -> np.ndarray:
    words = np.asarray(compressed)
    if words.ndim != 1 or words.dtype != np.uint32:
        raise TypeError("compressed must be a rank-1 numpy array with dtype uint32")
    return np.array(words, dtype=np.uint32)


def _check_symbol(symbol, codebook) -> int:
    if not isinstance(codebook, (EncoderHuffmanTree, ExpGolomb)):
        raise TypeError("codebook must be a constriction_amd.symbol.huffman.EncoderHuffmanTree or an exp_golomb.ExpGolomb")
    if isinstance(symbol, (bool, np.bool_)) or not isinstance(symbol, (int, np.integer)):
        raise TypeError(f"symbol must be an unsigned integer, not {type(symbol).__name__}")
    symbol = int(symbol)
    if symbol < 0:
        raise OverflowError("can't convert negative int to unsigned")
    if isinstance(codebook, ExpGolomb):
        if symbol >= codebook.num_symbols():
            raise OverflowError(f"symbol does not fit an unsigned integer of {codebook.bits} bits")
        return symbol
    if symbol >= codebook.num_symbols():
        raise KeyError("Tried to encode symbol that has zero probability under entropy model.")   # ImpossibleSymbol
    return symbol


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _encode(codebook, semantics, symbols, partial, nbits):
    """one launch: the buffered symbols (already in kernel order) after the partial word -> (completed words, partial, nbits)"""
    dev = _device()
    k = len(symbols)
    eg = isinstance(codebook, exp_golomb._Code)
    if eg:
        unsigned, signed = _EG_DTYPES[codebook.symbol_bytes]
        sym = torch.from_numpy(np.array(symbols, dtype=unsigned).view(signed)).to(dev).view(1, k)
    else:
        sym = torch.tensor(symbols, dtype=torch.int32).to(dev).view(1, k)
    stride = codebook.max_words(k, "stack" if semantics == N.HUFFMAN_STACK else "queue")
    words = torch.empty(stride, dtype=torch.int32, device=dev)
    n_words = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    cont = torch.tensor([partial | (nbits << 32)], dtype=torch.int64).to(dev)
    if eg:
        N.check(N.lib().cst_exp_golomb_encode_batch(semantics, _ptr(sym), codebook.symbol_bytes, 1, k, _ptr(words), stride, _ptr(n_words),
                                                    None, _ptr(cont), _ptr(status), _stream_ptr()), "cst_exp_golomb_encode_batch")
    else:
        N.check(N.lib().cst_huffman_encode_batch(codebook._h, semantics, _ptr(sym), 4, 1, k, _ptr(words), stride, _ptr(n_words), None,
                                                 _ptr(cont), _ptr(status), _stream_ptr()), "cst_huffman_encode_batch")
    st = int(status.cpu()[0])
    if st != N.STREAM_OK:
        raise RuntimeError(f"symbol encoder: stream status {st}")   # (symbols were range-checked at encode_symbol)
    c = int(cont.cpu()[0])
    return words[: int(n_words.cpu()[0])].cpu().numpy().view(np.uint32), c & 0xFFFFFFFF, c >> 32


def _decode(codebook, semantics, words: np.ndarray, cont: int):
    """one launch, one symbol -> (status, symbol, cont, words left / begun)"""
    dev = _device()
    dw = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev) if words.size else None
    n_words = torch.tensor([words.size], dtype=torch.int32).to(dev)
    c = torch.tensor([cont], dtype=torch.int64).to(dev)
    out = torch.empty(1, dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    if isinstance(codebook, exp_golomb._Code):
        # (an int32 output for every width: a u8 / u16 symbol is written as such into its first bytes, the rest is cleared)
        out.zero_()
        N.check(N.lib().cst_exp_golomb_decode_batch(semantics, _ptr(dw), None, words.size, words.size, _ptr(n_words), _ptr(out),
                                                    codebook.symbol_bytes, 1, 1, _ptr(c), _ptr(n_out), _ptr(status), _stream_ptr()),
                "cst_exp_golomb_decode_batch")
        return int(status.cpu()[0]), int(out.cpu()[0]) & 0xFFFFFFFF, int(c.cpu()[0]), int(n_out.cpu()[0])
    N.check(N.lib().cst_huffman_decode_batch(codebook._h, semantics, _ptr(dw), None, words.size, words.size, _ptr(n_words), _ptr(out),
                                             4, 1, 1, _ptr(c), _ptr(n_out), _ptr(status), _stream_ptr()), "cst_huffman_decode_batch")
    return int(status.cpu()[0]), int(out.cpu()[0]), int(c.cpu()[0]), int(n_out.cpu()[0])


def _check_decoder_codebook(codebook):
    if not isinstance(codebook, (DecoderHuffmanTree, ExpGolomb)):
        raise TypeError("codebook must be a constriction_amd.symbol.huffman.DecoderHuffmanTree or an exp_golomb.ExpGolomb")
    return codebook._cb


def _check_decoded(st):
    if st == N.STREAM_OUT_OF_DATA:
        raise ValueError(_OUT_OF_DATA)
    if st != N.STREAM_OK:
        raise RuntimeError(f"Huffman decoder: stream status {st}")


class _Container:
    """whole words + the partial word (nbits < 32 bits) + encodes not yet launched"""

    def __init__(self, semantics):
        self._semantics = semantics
        self._words = np.zeros(0, dtype=np.uint32)
        self._partial = 0
        self._nbits = 0
        self._pending = []
        self._pending_cb = None

    def _encode_symbol(self, symbol, codebook):
        symbol = _check_symbol(symbol, codebook)
        if self._pending and self._pending_cb is not codebook._cb:
            self._flush()
        self._pending.append(symbol)
        self._pending_cb = codebook._cb

    def _flush(self):
        if not self._pending:
            return
        syms = self._pending[::-1] if self._semantics == N.HUFFMAN_STACK else self._pending   # the stack kernel reads rows back to front
        new, self._partial, self._nbits = _encode(self._pending_cb, self._semantics, syms, self._partial, self._nbits)
        self._words = np.concatenate([self._words, new])
        self._pending, self._pending_cb = [], None

    def _bitrate(self) -> int:
        return 32 * int(self._words.size) + self._nbits


class StackCoder(_Container):
    """`constriction.symbol.StackCoder(compressed=None)`: last in, first out; encodes and decodes may interleave (bits-back)."""

    def __init__(self, compressed=None):
        super().__init__(N.HUFFMAN_STACK)
        if compressed is not None:
            words = _as_words(compressed)
            if words.size:
                last = int(words[-1])
                if last == 0:
                    raise ValueError("Compressed data for a stack must not end in a zero word.")
                # the seal is the HIGHEST set bit of the last word, where the writer puts it (the reference looks for the lowest,
                # src/symbol/mod.rs:478-497)
                self._nbits = last.bit_length() - 1
                self._partial = last ^ (1 << self._nbits)
                words = words[:-1]
            self._words = words

    def encode_symbol(self, symbol, codebook):
        self._encode_symbol(symbol, codebook)

    def decode_symbol(self, codebook) -> int:
        cb = _check_decoder_codebook(codebook)
        self._flush()
        # only the top of the stack can hold the next codeword: ship the words that cover the longest codeword below the partial
        # word (cst_huffman_max_words of one symbol bounds it)
        base = max(0, self._words.size - cb.max_words(1, "stack"))
        st, sym, cont, n_left = _decode(cb, N.HUFFMAN_STACK, self._words[base:], self._partial | (self._nbits << 32))
        if isinstance(cb, exp_golomb._Code) and st == N.STREAM_INVALID_DATA:
            raise ValueError(_INVALID_CODEWORD)      # (the container stays as it was: DESIGN.md 7)
        self._words = self._words[: base + n_left]
        self._partial, self._nbits = cont & 0xFFFFFFFF, cont >> 32
        _check_decoded(st)
        return sym

    def get_compressed_and_bitrate(self):
        self._flush()
        # sealed by one bit `1` above the written bits, the partial word pushed (src/symbol/mod.rs:264-283)
        sealed = np.concatenate([self._words, np.array([self._partial | (1 << self._nbits)], dtype=np.uint32)])
        return sealed, self._bitrate()

    _warned = False

    def get_compressed(self):
        if not StackCoder._warned:
            StackCoder._warned = True
            print("WARNING: `StackCoder.get_compressed` has been renamed to\n"
                  "         `StackCoder.get_compressed_and_bitrate` to avoid confusion.")
        return self.get_compressed_and_bitrate()


class QueueEncoder(_Container):
    """`constriction.symbol.QueueEncoder()`: first in, first out."""

    def __init__(self):
        super().__init__(N.HUFFMAN_QUEUE)

    def encode_symbol(self, symbol, codebook):
        self._encode_symbol(symbol, codebook)

    def get_compressed_and_bitrate(self):
        self._flush()
        tail = [self._partial] if self._nbits else []       # no seal; the partial word, if any (src/symbol/mod.rs:297-315)
        return np.concatenate([self._words, np.array(tail, dtype=np.uint32)]), self._bitrate()

    _warned = False

    def get_compressed(self):
        if not QueueEncoder._warned:
            QueueEncoder._warned = True
            print("WARNING: `QueueEncoder.get_compressed` has been renamed to\n"
                  "         `QueueEncoder.get_compressed_and_bitrate` to avoid confusion.")
        return self.get_compressed_and_bitrate()

    def get_decoder(self) -> "QueueDecoder":
        return QueueDecoder(self.get_compressed_and_bitrate()[0])


class QueueDecoder:
    """`constriction.symbol.QueueDecoder(compressed)`: reads the words front to back, each from bit 0 upwards."""

    def __init__(self, compressed):
        self._words = _as_words(compressed)
        self._pos = 0          # bits read

    def decode_symbol(self, codebook) -> int:
        cb = _check_decoder_codebook(codebook)
        first = self._pos // 32
        window = self._words[first: first + cb.max_words(1, "queue")]      # covers the longest codeword from any bit offset
        st, sym, cont, _ = _decode(cb, N.HUFFMAN_QUEUE, window, self._pos - 32 * first)
        if isinstance(cb, exp_golomb._Code) and st == N.STREAM_INVALID_DATA:
            raise ValueError(_INVALID_CODEWORD)      # (the read position stays where it was: DESIGN.md 7)
        if st == N.STREAM_OUT_OF_DATA:
            self._pos = 32 * int(self._words.size)
        _check_decoded(st)
        self._pos = 32 * first + cont
        return sym


__all__ = ["StackCoder", "QueueEncoder", "QueueDecoder", "huffman", "exp_golomb"]
