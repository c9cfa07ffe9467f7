"""Batched Huffman symbol codes (re-exported by `constriction_amd.batched`): one bit container per stream, one codebook shared by
the batch, coded by the kernels of csrc/cst_huffman.hip and, for streams of different lengths, csrc/cst_huffman_ragged.hip
(include/constriction_amd.h, "Huffman symbol codes").

A stack batch row s holds what the reference's `StackCoder` holds after `encode_symbol` of symbols[s] last to first and
`get_compressed_and_bitrate()` (src/pybindings/symbol/mod.rs:207-221); it decodes to symbols[s] in order, the convention of
`ans_encode`.  A queue batch row holds `QueueEncoder` after `encode_symbol` of symbols[s] first to last."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .batched import RAGGED_JUMP_EVERY, EncodedBatch, RaggedBatch, _ptr, _require_coder, _require_cuda, _stream_ptr

_SEMANTICS = {"stack": N.HUFFMAN_STACK, "queue": N.HUFFMAN_QUEUE}
_SYMBOL_BYTES = {torch.int32: 4, torch.uint8: 1}


def _semantics(semantics) -> int:
    if semantics not in _SEMANTICS:
        raise ValueError(f"semantics must be 'stack' or 'queue', not {semantics!r}")
    return _SEMANTICS[semantics]


def huffman_tree(probabilities) -> np.ndarray:
    """The reference's tree (src/symbol/huffman.rs:62-116) as its encoder representation, nodes[2n - 1] (uint64: parent << 1 |
    bit, 0 at the root).  float32 probabilities are added in float32, float64 in float64, as the reference does.
    NaN raises FloatingPointError (src/pybindings/mod.rs:245-250); negative or infinite values, which the reference documents as
    invalid (src/pybindings/symbol/huffman.rs:35-45) without checking them, raise ValueError."""
    if isinstance(probabilities, torch.Tensor):
        probabilities = probabilities.detach().cpu().numpy()
    p = np.asarray(probabilities)
    if p.ndim != 1 or p.dtype not in (np.float32, np.float64):
        raise TypeError("probabilities must be a rank-1 array of dtype float32 or float64")
    if p.size == 0:
        raise ValueError("a Huffman tree needs at least one symbol")
    if np.isnan(p).any():
        raise FloatingPointError("Floating point value is not a number (NaN).")
    wide = np.ascontiguousarray(p, dtype=np.float64)
    nodes = np.zeros(2 * p.size - 1, dtype=np.uint64)
    st = N.load_library().cst_huffman_tree(wide.ctypes.data, p.size, int(p.dtype == np.float32), nodes.ctypes.data)
    if st == N.CST_ERR_MODEL:
        raise ValueError("probabilities must be nonnegative and finite")
    N.check(st, "cst_huffman_tree")
    return nodes


class HuffmanCodebook:
    """Device codebook (cst_huffman_codebook_create) shared by every stream of a batch: the encoder's codewords in both bit orders
    and the decoder's table, from one tree."""

    def __init__(self, nodes: np.ndarray):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        n = (nodes.size + 1) // 2
        if nodes.ndim != 1 or nodes.size != 2 * n - 1 or n < 1:
            raise ValueError("nodes must hold 2n - 1 entries")
        if n > N.HUFFMAN_MAX_SYMBOLS:
            raise ValueError(f"Huffman codebooks take at most {N.HUFFMAN_MAX_SYMBOLS} symbols")
        L = N.lib()
        h = C.c_void_p()
        N.check(L.cst_huffman_codebook_create(nodes.ctypes.data, n, _stream_ptr(), C.byref(h)), "cst_huffman_codebook_create")
        self._h = h
        self.nodes = nodes
        self.n_symbols = n

    @classmethod
    def from_probabilities(cls, probabilities) -> "HuffmanCodebook":
        """float32 or float64 probabilities (the dtype selects the type the tree adds in)"""
        return cls(huffman_tree(probabilities))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.load_library().cst_huffman_codebook_destroy(h)
            except Exception:
                pass

    def max_words(self, n_per_stream: int, semantics="stack") -> int:
        """slab stride that holds any stream of n_per_stream symbols (cst_huffman_max_words)"""
        return N.load_library().cst_huffman_max_words(self._h, n_per_stream, _semantics(semantics))


@dataclass
class HuffmanBatch(EncodedBatch):
    """Slabs of a batched Huffman encode: stream s is words[s, :n_words[s]], bitrate n_bits[s] (the written bits without a
    stack's seal).  `stream(s)` is `get_compressed_and_bitrate()[0]` of the reference's coder for row s; `batched.compact`
    packs the slabs."""
    n_bits: Optional[torch.Tensor] = None
    semantics: str = "stack"


def _symbols_arg(symbols: torch.Tensor):
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    if symbols.dtype not in _SYMBOL_BYTES:
        raise TypeError("Huffman symbols are int32 or uint8")
    if symbols.dim() != 2:
        raise ValueError("symbols must be a [n_streams, n_per_stream] matrix (stream-major)")
    return symbols.contiguous(), _SYMBOL_BYTES[symbols.dtype]


def huffman_encode(symbols: torch.Tensor, codebook: HuffmanCodebook, semantics="stack", stride: Optional[int] = None,
                   out: Optional[HuffmanBatch] = None) -> HuffmanBatch:
    """Row s of the int32 / uint8 matrix `symbols` into its own stack (`StackCoder`, rows consumed last to first, sealed) or
    queue (`QueueEncoder`).  A symbol outside 0..n-1 leaves its stream with status IMPOSSIBLE_SYMBOL and 0 words, a slab that is
    too small (`stride` below `codebook.max_words`) with CAPACITY.  `out` (a HuffmanBatch of an earlier call with as many streams)
    is reused as it is: its slab stride holds, and `stride` is ignored, as for `ans_encode`."""
    sem = _semantics(semantics)
    symbols, sb = _symbols_arg(symbols)
    n_streams, n_per = symbols.shape
    dev = symbols.device
    if out is None:
        stride = stride if stride is not None else codebook.max_words(n_per, semantics)
        out = HuffmanBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev),
                           config=None, n_bits=torch.empty(n_streams, dtype=torch.int64, device=dev), semantics=semantics)
    else:
        if out.words.dim() != 2 or out.words.shape[0] != n_streams or out.n_words.numel() != n_streams or \
                out.status.numel() != n_streams or out.n_bits is None or out.n_bits.numel() != n_streams:
            raise ValueError("out must be a HuffmanBatch with one row per stream")
        for t, dt, name in ((out.words, torch.int32, "out.words"), (out.n_words, torch.int32, "out.n_words"),
                            (out.status, torch.int32, "out.status"), (out.n_bits, torch.int64, "out.n_bits")):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous device tensor of dtype {dt}")
        out.semantics = semantics
    N.check(N.lib().cst_huffman_encode_batch(codebook._h, sem, _ptr(symbols), sb, n_streams, n_per, _ptr(out.words),
                                             out.words.shape[1], _ptr(out.n_words), _ptr(out.n_bits), None, _ptr(out.status),
                                             _stream_ptr()), "cst_huffman_encode_batch")
    return out


def huffman_decode(encoded, codebook: HuffmanCodebook, n_per_stream: int, semantics=None, offsets: Optional[torch.Tensor] = None,
                   dtype=torch.int32):
    """n_per_stream symbols of every stream -> (symbols [n_streams, n_per_stream] of `dtype` (int32 or uint8), status int32).

    `encoded` is a HuffmanBatch (its semantics unless given) or (words, n_words): slabs [n_streams, stride], or with `offsets`
    (int64 [n_streams + 1], `batched.compact`) the packed words.  A stack stream without its seal reports INVALID_DATA, a
    stream that runs out of bits OUT_OF_DATA (its symbols from there on read 0)."""
    if isinstance(encoded, HuffmanBatch):
        words, n_words = encoded.words, encoded.n_words
        semantics = semantics or encoded.semantics
    else:
        words, n_words = encoded
    if semantics is None:
        raise ValueError("semantics ('stack' or 'queue') is needed for plain words")
    sem = _semantics(semantics)
    if dtype not in _SYMBOL_BYTES:
        raise TypeError("Huffman symbols are int32 or uint8")
    words = _require_cuda(words, torch.int32, "words")
    n_words = _require_cuda(n_words, torch.int32, "n_words")
    if offsets is not None:
        offsets = _require_cuda(offsets, torch.int64, "offsets")
        if offsets.numel() < n_words.numel():
            raise ValueError("offsets needs one entry per stream")
    elif words.dim() != 2 or words.shape[0] < n_words.numel():
        raise ValueError("slab words must be a [n_streams, stride] matrix (or give offsets for packed words)")
    stride = 0 if offsets is not None else words.shape[1]
    n_streams = n_words.numel()
    dev = words.device
    out = torch.empty((n_streams, n_per_stream), dtype=dtype, device=dev)
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    N.check(N.lib().cst_huffman_decode_batch(codebook._h, sem, _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words),
                                             _ptr(out), _SYMBOL_BYTES[dtype], n_streams, n_per_stream, None, None, _ptr(status),
                                             _stream_ptr()), "cst_huffman_decode_batch")
    return out, status


# ---------------------------------------------------------------------------------------------------------------------
# streams of different lengths: one container per document, all of them in one launch (csrc/cst_huffman_ragged.hip)
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class BitJump:
    """Jump points of a ragged Huffman batch: chunk j of stream s (symbols j * interval .. of it) starts at bit bits[chunk_offsets[s] + j]
    of the stream's container -- a queue is read from there upwards, a stack from there downwards.  A bit index is all a prefix
    code needs: there is no coder state."""
    interval: int
    chunk_offsets: torch.Tensor   # int64 [n_streams + 1]: exclusive prefix sum of ceil(length / interval)
    bits: torch.Tensor            # int64 [>= total chunks] (what lies behind chunk_offsets[-1] entries is not written or read)


def _never_null(t: torch.Tensor):
    """the address of `t`, or of a small buffer on its device if it has no elements (the ABI refuses NULL)"""
    return _ptr(t) if t.numel() else _ptr(torch.empty(4, dtype=torch.int32, device=t.device))


def _flat_symbols(symbols: torch.Tensor, sym_offsets: torch.Tensor):
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    if symbols.dtype not in _SYMBOL_BYTES:
        raise TypeError("Huffman symbols are int32 or uint8")
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if symbols.dim() != 1 or n_streams < 0:
        raise ValueError("symbols must be flat and sym_offsets hold n_streams + 1 entries")
    return symbols.contiguous(), _SYMBOL_BYTES[symbols.dtype], sym_offsets, n_streams


def huffman_count_bits(symbols: torch.Tensor, codebook: HuffmanCodebook, sym_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exact bits of every stream under `codebook` (int64 [n_streams], without a stack's seal): rows of a matrix, or with
    `sym_offsets` (int64 [n_streams + 1]) the ranges of flat `symbols`.  A symbol outside the alphabet counts 0 bits: the encoder
    is what reports it."""
    if sym_offsets is None:
        symbols, sb = _symbols_arg(symbols)
        n_streams, n_per = symbols.shape
    else:
        symbols, sb, sym_offsets, n_streams = _flat_symbols(symbols, sym_offsets)
        n_per = 0
    n_bits = torch.empty(n_streams, dtype=torch.int64, device=symbols.device)
    N.check(N.lib().cst_huffman_count_bits(codebook._h, _never_null(symbols), sb, _ptr(sym_offsets), n_streams, n_per, _ptr(n_bits),
                                           _stream_ptr()), "cst_huffman_count_bits")
    return n_bits


def _jump_every(jump_every) -> object:
    """the `jump_every` argument, judged before any tensor is looked at: "auto", or an int that is 0 or a positive multiple of 32"""
    if isinstance(jump_every, str):
        if jump_every != "auto":
            raise ValueError("jump_every: 'auto', 0 or a multiple of 32")
        return "auto"
    jump_every = int(jump_every or 0)
    if jump_every < 0 or jump_every % 32 != 0 or jump_every > 0x7fffffff:
        raise ValueError("jump_every: 'auto', 0 or a multiple of 32")
    return jump_every


def huffman_encode_ragged(symbols: torch.Tensor, sym_offsets: torch.Tensor, codebook: HuffmanCodebook, semantics="stack",
                          jump_every=0) -> RaggedBatch:
    """One container per stream, streams of different lengths (`symbols` flat, int32 or uint8; stream s =
    symbols[sym_offsets[s]:sym_offsets[s+1]]) in one launch.  The slabs are exact: a count pass sizes each to its stream's bits (and
    a stack's seal), rounded up to 16 bytes.  Returns a RaggedBatch with coder="huffman" (the ANS, range and Exp-Golomb decoders
    refuse it), config = (semantics, symbol dtype) and the bit counts as `.n_bits`; `stream(s)` is what `huffman_encode` gives for
    that stream as a one-row batch.  A stream with a symbol outside 0..n-1 reports IMPOSSIBLE_SYMBOL and has 0 words.

    jump_every: 0 (default) -- no jump points.  A positive multiple of 32: the encoder also notes the container's bit length at
    every jump_every symbols of every stream (the words are unchanged) and the batch carries the table as `.jump` (a BitJump);
    huffman_decode_ragged then decodes all chunks side by side, and a launch lasts jump_every symbols instead of its longest
    stream.  "auto": RAGGED_JUMP_EVERY where the streams average more than RAGGED_JUMP_EVERY symbols, else 0 -- the range coder's
    rule, measured for these kernels on 100 000 documents: at 20 .. 2000 symbols per document the table makes the
    decode 4 times faster for 2-7 % of encode time; at 200 symbols per document the round trip is a wash, and "auto" leaves it out."""
    sem = _semantics(semantics)
    jump_every = _jump_every(jump_every)
    symbols, sb, sym_offsets, n_streams = _flat_symbols(symbols, sym_offsets)
    dev = symbols.device
    bits = huffman_count_bits(symbols, codebook, sym_offsets)
    slabs = ((bits + ((sem == N.HUFFMAN_STACK) + 31)) // 32 + 3) // 4 * 4
    word_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(slabs, 0, out=word_offsets[1:])
    total = int(word_offsets[-1].item()) if n_streams else 0
    out = RaggedBatch(torch.empty(max(total, 4), dtype=torch.int32, device=dev), word_offsets,
                      torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev),
                      (semantics, symbols.dtype), coder="huffman")
    out.n_bits = torch.empty(n_streams, dtype=torch.int64, device=dev)
    if jump_every == "auto":
        jump_every = RAGGED_JUMP_EVERY if symbols.numel() > n_streams * RAGGED_JUMP_EVERY else 0
    if not jump_every:
        N.check(N.lib().cst_huffman_encode_ragged(codebook._h, sem, _never_null(symbols), sb, _ptr(sym_offsets), n_streams, _ptr(out.words),
                                                  _ptr(word_offsets), 0, _ptr(out.n_words), _ptr(out.n_bits), _ptr(out.status),
                                                  _stream_ptr()), "cst_huffman_encode_ragged")
        return out
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    chunk_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum((lengths + (jump_every - 1)) // jump_every, 0, out=chunk_offsets[1:])
    n_chunks = max(symbols.numel() // jump_every + n_streams, 1)      # (an upper bound: no read-back)
    out.jump = BitJump(jump_every, chunk_offsets, torch.empty(n_chunks, dtype=torch.int64, device=dev))
    N.check(N.lib().cst_huffman_encode_ragged_jump(codebook._h, sem, _never_null(symbols), sb, _ptr(sym_offsets), n_streams, _ptr(out.words),
                                                   _ptr(word_offsets), 0, _ptr(out.n_words), _ptr(out.n_bits), jump_every,
                                                   _ptr(chunk_offsets), _ptr(out.jump.bits), _ptr(out.status), _stream_ptr()),
            "cst_huffman_encode_ragged_jump")
    return out


def huffman_decode_ragged(encoded: RaggedBatch, codebook: HuffmanCodebook, sym_offsets: torch.Tensor, out: Optional[torch.Tensor] = None):
    """Stream s yields sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:], in the dtype the batch was encoded from (or
    that of `out`).  Returns (symbols flat, status per stream).  A batch with jump points (`jump_every` of the encoder) is decoded
    chunk by chunk, all chunks side by side; a stream's status is then the largest of its chunks' (OUT_OF_DATA before INVALID_DATA),
    and a chunk that fails reads 0 from the failure to its own end while the other chunks keep their symbols."""
    _require_coder(encoded, "huffman")
    semantics, dtype = encoded.config
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if n_streams != encoded.n_words.numel():
        raise ValueError("sym_offsets must hold one entry per stream of the batch, and one more")
    dev = encoded.words.device
    total = int(sym_offsets[-1].item()) if n_streams > 0 else 0
    if out is None:
        out = torch.empty(total, dtype=dtype, device=dev)
    elif not out.is_cuda or not out.is_contiguous() or out.numel() < total or out.dtype not in _SYMBOL_BYTES:
        raise ValueError("out must be a contiguous int32 or uint8 device tensor with room for every symbol")
    status = torch.empty(max(n_streams, 0), dtype=torch.int32, device=dev)
    jump = encoded.jump
    if jump is None:
        N.check(N.lib().cst_huffman_decode_ragged(codebook._h, _semantics(semantics), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                  encoded.words.numel(), _ptr(encoded.n_words), _never_null(out), _SYMBOL_BYTES[out.dtype],
                                                  _ptr(sym_offsets), n_streams, _ptr(status), _stream_ptr()), "cst_huffman_decode_ragged")
        return out, status
    if not isinstance(jump, BitJump):
        raise ValueError("the batch's jump points are not those of a Huffman batch")
    if jump.chunk_offsets.numel() != n_streams + 1:
        raise ValueError("the jump table must describe every stream of the batch")
    N.check(N.lib().cst_huffman_decode_ragged_jump(codebook._h, _semantics(semantics), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                   encoded.words.numel(), _ptr(encoded.n_words), _never_null(out), _SYMBOL_BYTES[out.dtype],
                                                   _ptr(sym_offsets), n_streams, jump.interval, _ptr(jump.chunk_offsets),
                                                   jump.bits.numel(), _ptr(jump.bits), _ptr(status), _stream_ptr()),
            "cst_huffman_decode_ragged_jump")
    return out, status


def huffman_decode_ragged_select(encoded: RaggedBatch, codebook: HuffmanCodebook, sym_offsets: torch.Tensor, streams, first=None, count=None,
                                 out: Optional[torch.Tensor] = None):
    """Random access into a ragged Huffman batch: query q decodes symbols [first[q], first[q] + count[q]) of document streams[q], and
    nothing else is decoded -- the queries and the three results (symbols flat, out_offsets int64 [n_queries + 1], status int32
    [n_queries]) of `batched.ans_decode_ragged_select`.  The symbols come in the dtype the batch was encoded from, or in that of `out`
    (int32 or uint8).  With jump points (`encoded.jump`, a BitJump) every query seeks to the bit index in front of `first`, decodes and
    drops first % interval symbols, and every chunk it touches runs on a lane of its own; without them a query starts where its
    document starts and drops `first` symbols.  A query the device refuses (no such document, a range beyond its document, a table
    entry beyond its stream's bits, a stack without its seal) reports INVALID_DATA and writes nothing; otherwise a query's status is
    the worst of its pieces' (OUT_OF_DATA before INVALID_DATA), and a piece that fails reads 0 from the failure to its own end."""
    from .batched import _symbol_decode_ragged_select
    return _symbol_decode_ragged_select("huffman", encoded, sym_offsets, streams, first, count, out, _SYMBOL_BYTES,
                                        "cst_huffman_decode_ragged_select", lambda: (codebook._h,))
