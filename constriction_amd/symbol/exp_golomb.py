"""Exponential-Golomb codes for the coders of `constriction_amd.symbol`: the reference's `ExpGolomb<N>` (src/symbol/exp_golomb.rs).

The reference exposes this codebook to Rust only, so the constructor is this package's own: `ExpGolomb(bits=32)` is `ExpGolomb::<u32>`,
`bits=16` and `bits=8` the narrower types.  There is nothing to build: the object only names the symbol type.  One object serves
`encode_symbol` and `decode_symbol` alike."""
from __future__ import annotations

from .. import _native as N


class _Code:
    """what the coders launch with: the symbol width (one shared object per width, so that equal codebooks share a launch)"""

    def __init__(self, symbol_bytes: int):
        self.symbol_bytes = symbol_bytes

    def max_words(self, n_per_stream: int, semantics="stack") -> int:
        sem = N.SYMBOL_STACK if semantics == "stack" else N.SYMBOL_QUEUE
        return N.load_library().cst_exp_golomb_max_words(n_per_stream, self.symbol_bytes, sem)


_CODES = {8: _Code(1), 16: _Code(2), 32: _Code(4)}


class ExpGolomb:
    """`ExpGolomb(bits=32)`: the code of the unsigned integers below 2**bits (bits 8, 16 or 32).  Symbol x codes as floor(log2(x + 1))
    zeros followed by x + 1 in binary; 2**bits - 1 wraps as in the reference (bits zeros, a one, bits zeros)."""

    def __init__(self, bits: int = 32):
        if isinstance(bits, bool) or not isinstance(bits, int):
            raise TypeError("bits must be 8, 16 or 32")
        if bits not in _CODES:
            raise ValueError("bits must be 8, 16 or 32")
        self.bits = bits
        self._cb = _CODES[bits]

    def num_symbols(self) -> int:
        return 1 << self.bits

    def __repr__(self):
        return f"ExpGolomb(bits={self.bits})"
