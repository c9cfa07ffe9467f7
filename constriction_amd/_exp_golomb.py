"""Batched Exponential-Golomb symbol codes (re-exported by `constriction_amd.batched`): one bit container per stream and no codebook
at all, coded by the kernels of csrc/cst_exp_golomb.hip (include/constriction_amd.h, "Exponential-Golomb symbol codes").

The code is the reference's `ExpGolomb<N>` (src/symbol/exp_golomb.rs) for N = u8 (uint8 tensors), u16 (the bit pattern of int16) or
u32 (the bit pattern of int32: -1 is u32::MAX); the containers are those of the Huffman calls.  A stack batch row s holds what the
reference's `StackCoder` holds after `encode_iid_symbols_reverse(symbols[s])`, sealed; it decodes to symbols[s] in order.  A queue
batch row holds `QueueEncoder` after `encode_iid_symbols(symbols[s])`."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N
from ._huffman import BitJump, HuffmanBatch, _jump_every, _semantics
from .batched import RAGGED_JUMP_EVERY, RaggedBatch, _ptr, _require_coder, _require_cuda, _stream_ptr

_SYMBOL_BYTES = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}


def _symbol_bytes(dtype) -> int:
    if dtype not in _SYMBOL_BYTES:
        raise TypeError("Exp-Golomb symbols are uint8, int16 (the bits of u16) or int32 (the bits of u32)")
    return _SYMBOL_BYTES[dtype]


def exp_golomb_max_words(n_per_stream: int, dtype=torch.int32, semantics="stack") -> int:
    """slab stride that holds any stream of n_per_stream symbols of `dtype` (cst_exp_golomb_max_words)"""
    return N.load_library().cst_exp_golomb_max_words(n_per_stream, _symbol_bytes(dtype), _semantics(semantics))


def exp_golomb_count_bits(symbols: torch.Tensor, sym_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exact bits of every stream (int64 [n_streams], without a stack's seal): rows of a matrix, or with `sym_offsets` (int64
    [n_streams + 1]) the ranges of flat `symbols`."""
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    sb = _symbol_bytes(symbols.dtype)
    symbols = symbols.contiguous()
    if sym_offsets is None:
        if symbols.dim() != 2:
            raise ValueError("symbols must be a [n_streams, n_per_stream] matrix (or flat, with sym_offsets)")
        n_streams, n_per = symbols.shape
    else:
        sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
        n_streams, n_per = sym_offsets.numel() - 1, 0
        if symbols.dim() != 1 or n_streams < 0:
            raise ValueError("symbols must be flat and sym_offsets hold n_streams + 1 entries")
    n_bits = torch.empty(n_streams, dtype=torch.int64, device=symbols.device)
    N.check(N.lib().cst_exp_golomb_count_bits(_never_null(symbols), sb, _ptr(sym_offsets), n_streams, n_per, _ptr(n_bits), _stream_ptr()),
            "cst_exp_golomb_count_bits")
    return n_bits


def _never_null(t: torch.Tensor):
    """the address of `t`, or of a small buffer on its device if it has no elements (the ABI refuses NULL)"""
    return _ptr(t) if t.numel() else _ptr(torch.empty(4, dtype=torch.int32, device=t.device))


def exp_golomb_encode(symbols: torch.Tensor, semantics="stack", stride="exact", out: Optional[HuffmanBatch] = None) -> HuffmanBatch:
    """Row s of the uint8 / int16 / int32 matrix `symbols` into its own stack (rows consumed last to first, sealed) or queue.

    stride: "exact" (default) counts every row's bits first and reads back their maximum: the slabs are as long as the longest stream,
    rounded up to 16 bytes; "max" takes `exp_golomb_max_words` (2 B + 1 bits per symbol: no read-back, ~13x the words small symbols
    need); an integer is taken as given, and a stream that does not fit reports CAPACITY with 0 words.  Every value has a codeword:
    there is no other failure.  `out` (a batch of an earlier call with as many streams) is reused as it is and `stride` ignored."""
    sem = _semantics(semantics)
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    sb = _symbol_bytes(symbols.dtype)
    if symbols.dim() != 2:
        raise ValueError("symbols must be a [n_streams, n_per_stream] matrix (stream-major)")
    symbols = symbols.contiguous()
    n_streams, n_per = symbols.shape
    dev = symbols.device
    if out is None:
        if isinstance(stride, str):
            if stride == "max":
                stride = exp_golomb_max_words(n_per, symbols.dtype, semantics)
            elif stride == "exact":
                bits = int(exp_golomb_count_bits(symbols).max().item()) if n_streams else 0
                stride = ((bits + (sem == N.SYMBOL_STACK) + 31) // 32 + 3) // 4 * 4
            else:
                raise ValueError('stride: "exact", "max" or a number of words')
        stride = int(stride)
        out = HuffmanBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev),
                           config=None, n_bits=torch.empty(n_streams, dtype=torch.int64, device=dev), semantics=semantics)
    else:
        if out.words.dim() != 2 or out.words.shape[0] != n_streams or out.n_words.numel() != n_streams or \
                out.status.numel() != n_streams or out.n_bits is None or out.n_bits.numel() != n_streams:
            raise ValueError("out must be a batch with one row per stream")
        for t, dt, name in ((out.words, torch.int32, "out.words"), (out.n_words, torch.int32, "out.n_words"),
                            (out.status, torch.int32, "out.status"), (out.n_bits, torch.int64, "out.n_bits")):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous device tensor of dtype {dt}")
        out.semantics = semantics
    N.check(N.lib().cst_exp_golomb_encode_batch(sem, _ptr(symbols), sb, n_streams, n_per, _ptr(out.words), out.words.shape[1],
                                                _ptr(out.n_words), _ptr(out.n_bits), None, _ptr(out.status), _stream_ptr()),
            "cst_exp_golomb_encode_batch")
    return out


def exp_golomb_decode(encoded, n_per_stream: int, semantics=None, offsets: Optional[torch.Tensor] = None, dtype=torch.int32):
    """n_per_stream symbols of every stream -> (symbols [n_streams, n_per_stream] of `dtype`, status int32).

    `encoded` is the batch of `exp_golomb_encode` (its semantics unless given) or (words, n_words): slabs [n_streams, stride], or with
    `offsets` (int64 [n_streams + 1], `batched.compact`) the packed words.  An invalid codeword -- the bits run out, a zero run
    longer than the type has bits -- or a stack without its seal reports INVALID_DATA; the symbols from there on read 0."""
    if isinstance(encoded, HuffmanBatch):
        words, n_words = encoded.words, encoded.n_words
        semantics = semantics or encoded.semantics
    else:
        words, n_words = encoded
    if semantics is None:
        raise ValueError("semantics ('stack' or 'queue') is needed for plain words")
    sem = _semantics(semantics)
    sb = _symbol_bytes(dtype)
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
    N.check(N.lib().cst_exp_golomb_decode_batch(sem, _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words), _ptr(out), sb,
                                                n_streams, n_per_stream, None, None, _ptr(status), _stream_ptr()),
            "cst_exp_golomb_decode_batch")
    return out, status


def exp_golomb_encode_ragged(symbols: torch.Tensor, sym_offsets: torch.Tensor, semantics="stack", jump_every=0) -> RaggedBatch:
    """One container per stream, streams of different lengths (`symbols` flat, stream s = symbols[sym_offsets[s]:sym_offsets[s+1]]) in
    one launch.  The slabs are exact: a count pass sizes each to its stream's bits (and a stack's seal), rounded up to 16 bytes.
    Returns a RaggedBatch with coder="exp_golomb" (the ANS and range decoders refuse it), config = (semantics, symbol dtype) and the
    bit counts as `.n_bits`.

    jump_every: 0 (default) -- no jump points.  A positive multiple of 32: the encoder also notes the container's bit length at
    every jump_every symbols of every stream (the words are unchanged) and the batch carries the table as `.jump` (a BitJump);
    exp_golomb_decode_ragged then decodes all chunks side by side, and exp_golomb_decode_ragged_select reads parts of documents.
    "auto": RAGGED_JUMP_EVERY where the streams average more than RAGGED_JUMP_EVERY symbols, else 0 -- the Huffman coder's rule,
    which the measurement on 100 000 documents supports for this coder too: at 20 .. 2000 symbols per document the
    table makes the decode 4.1-4.5 times faster for -1 .. +10 % of the encode call; at 200 symbols per document, one chunk each, the
    decode gains 0.04 ms and the encode call loses 0.03 ms, a wash, and "auto" leaves the table out."""
    sem = _semantics(semantics)
    jump_every = _jump_every(jump_every)
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    sb = _symbol_bytes(symbols.dtype)
    symbols = symbols.contiguous()
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if symbols.dim() != 1 or n_streams < 0:
        raise ValueError("symbols must be flat and sym_offsets hold n_streams + 1 entries")
    dev = symbols.device
    bits = exp_golomb_count_bits(symbols, sym_offsets)
    slabs = ((bits + ((sem == N.SYMBOL_STACK) + 31)) // 32 + 3) // 4 * 4
    word_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(slabs, 0, out=word_offsets[1:])
    total = int(word_offsets[-1].item()) if n_streams else 0
    out = RaggedBatch(torch.empty(max(total, 4), dtype=torch.int32, device=dev), word_offsets,
                      torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev),
                      (semantics, symbols.dtype), coder="exp_golomb")
    out.n_bits = torch.empty(n_streams, dtype=torch.int64, device=dev)
    if jump_every == "auto":
        jump_every = RAGGED_JUMP_EVERY if symbols.numel() > n_streams * RAGGED_JUMP_EVERY else 0
    if not jump_every:
        N.check(N.lib().cst_exp_golomb_encode_ragged(sem, _never_null(symbols), sb, _ptr(sym_offsets), n_streams, _ptr(out.words),
                                                     _ptr(word_offsets), 0, _ptr(out.n_words), _ptr(out.n_bits), _ptr(out.status),
                                                     _stream_ptr()), "cst_exp_golomb_encode_ragged")
        return out
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    chunk_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum((lengths + (jump_every - 1)) // jump_every, 0, out=chunk_offsets[1:])
    n_chunks = max(symbols.numel() // jump_every + n_streams, 1)      # (an upper bound: no read-back)
    out.jump = BitJump(jump_every, chunk_offsets, torch.empty(n_chunks, dtype=torch.int64, device=dev))
    N.check(N.lib().cst_exp_golomb_encode_ragged_jump(sem, _never_null(symbols), sb, _ptr(sym_offsets), n_streams, _ptr(out.words),
                                                      _ptr(word_offsets), 0, _ptr(out.n_words), _ptr(out.n_bits), jump_every,
                                                      _ptr(chunk_offsets), _ptr(out.jump.bits), _ptr(out.status), _stream_ptr()),
            "cst_exp_golomb_encode_ragged_jump")
    return out


def exp_golomb_decode_ragged(encoded: RaggedBatch, sym_offsets: torch.Tensor, out: Optional[torch.Tensor] = None):
    """Stream s yields sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:], in the dtype the batch was encoded from (or
    that of `out`).  Returns (symbols flat, status per stream).  A batch with jump points (`jump_every` of the encoder) is decoded
    chunk by chunk, all chunks side by side; a stream's status is then the largest of its chunks', and a chunk that fails reads 0
    from the failure to its own end while the other chunks keep their symbols."""
    _require_coder(encoded, "exp_golomb")
    semantics, dtype = encoded.config
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if n_streams != encoded.n_words.numel():
        raise ValueError("sym_offsets must hold one entry per stream of the batch, and one more")
    dev = encoded.words.device
    total = int(sym_offsets[-1].item()) if n_streams > 0 else 0
    if out is None:
        out = torch.empty(total, dtype=dtype, device=dev)
    elif not out.is_cuda or not out.is_contiguous() or out.numel() < total:
        raise ValueError("out must be a contiguous device tensor with room for every symbol")
    status = torch.empty(max(n_streams, 0), dtype=torch.int32, device=dev)
    jump = encoded.jump
    if jump is None:
        N.check(N.lib().cst_exp_golomb_decode_ragged(_semantics(semantics), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                     encoded.words.numel(), _ptr(encoded.n_words), _never_null(out), _symbol_bytes(out.dtype),
                                                     _ptr(sym_offsets), n_streams, _ptr(status), _stream_ptr()), "cst_exp_golomb_decode_ragged")
        return out, status
    if not isinstance(jump, BitJump):
        raise ValueError("the batch's jump points are not those of an Exp-Golomb batch")
    if jump.chunk_offsets.numel() != n_streams + 1:
        raise ValueError("the jump table must describe every stream of the batch")
    N.check(N.lib().cst_exp_golomb_decode_ragged_jump(_semantics(semantics), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                      encoded.words.numel(), _ptr(encoded.n_words), _never_null(out), _symbol_bytes(out.dtype),
                                                      _ptr(sym_offsets), n_streams, jump.interval, _ptr(jump.chunk_offsets),
                                                      jump.bits.numel(), _ptr(jump.bits), _ptr(status), _stream_ptr()),
            "cst_exp_golomb_decode_ragged_jump")
    return out, status


def exp_golomb_decode_ragged_select(encoded: RaggedBatch, sym_offsets: torch.Tensor, streams, first=None, count=None,
                                    out: Optional[torch.Tensor] = None):
    """`batched.huffman_decode_ragged_select` for an Exp-Golomb batch: the same queries and the same three results (symbols flat in the
    batch's dtype or that of `out`, out_offsets, status per query).  A piece that fails reports INVALID_DATA."""
    from .batched import _symbol_decode_ragged_select
    return _symbol_decode_ragged_select("exp_golomb", encoded, sym_offsets, streams, first, count, out, _SYMBOL_BYTES,
                                        "cst_exp_golomb_decode_ragged_select", tuple)
