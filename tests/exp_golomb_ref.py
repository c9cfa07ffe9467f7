"""Test helper: a bit-by-bit plain-Python restatement of the reference's Exponential-Golomb symbol code, written from the rules of
src/symbol/exp_golomb.rs and the bit containers of src/symbol/mod.rs, for the tests to compare the library against.  Slow and simple
on purpose: bits are '0' / '1' characters in the order they are written or read.

ExpGolomb<N>, N unsigned of B bits: m = symbol + 1 (wrapping), len = floor(log2 m); the codeword is len zeros followed by the len + 1
bits of m, most significant first.  symbol = N::MAX wraps to m == 0 and codes as B zeros, a one, B zeros."""


def prefix_codeword(symbol, B=32):
    assert 0 <= symbol < (1 << B)
    m = (symbol + 1) & ((1 << B) - 1)
    if m == 0:
        return "0" * B + "1" + "0" * B
    length = m.bit_length() - 1
    return "0" * length + format(m, "b")


def suffix_codeword(symbol, B=32):
    """what a stack writes: the prefix order reversed"""
    return prefix_codeword(symbol, B)[::-1]


def _words(bits):
    """bits in write order -> u32 words, each filled from bit 0 upwards, the last one zero-padded"""
    words = []
    for k in range(0, len(bits), 32):
        words.append(sum(1 << i for i, b in enumerate(bits[k: k + 32]) if b == "1"))
    return words


def _bits(words):
    """u32 words -> their bits from bit 0 of the first word upwards"""
    return "".join("1" if (w >> i) & 1 else "0" for w in words for i in range(32))


def queue_bits(message, B=32):
    return "".join(prefix_codeword(x, B) for x in message)


def stack_bits(message, B=32):
    """encode_symbol(x) for x in reversed(message): row s of a batch then decodes to message in order"""
    return "".join(suffix_codeword(x, B) for x in reversed(message))


def queue_encode(message, B=32):
    """-> (words, n_bits): no seal, the last partial word zero-padded"""
    bits = queue_bits(message, B)
    return _words(bits), len(bits)


def stack_encode(message, B=32):
    """-> (words, n_bits): one seal bit above the last written bit; n_bits does not count it"""
    bits = stack_bits(message, B)
    return _words(bits + "1"), len(bits)


def decode_symbol(bits, pos, B=32):
    """One codeword from bits[pos:] in read order -> (symbol, new pos), or (None, pos) for an invalid codeword: the bits run out in
    the zero run, the run is longer than B, the bits run out within the len value bits, or len == B with value bits not all zero."""
    start, length = pos, 0
    while True:
        if pos >= len(bits):
            return None, start
        bit = bits[pos]
        pos += 1
        if bit == "1":
            break
        length += 1
    if length > B:
        return None, start
    m = 1
    for _ in range(length):
        if pos >= len(bits):
            return None, start
        m = ((m << 1) | int(bits[pos])) & ((1 << B) - 1)
        pos += 1
    if length == B and m != 0:
        return None, start
    return (m - 1) & ((1 << B) - 1), pos


def read_bits(words, semantics):
    """the bits of a container in read order, or None for a stack without a seal (no words, or a zero last word).  A stack is found by
    the highest set bit of its last word and read from there downwards."""
    if semantics == "queue":
        return _bits(words)
    if not words or words[-1] == 0:
        return None
    bits = _bits(words)
    top = 32 * (len(words) - 1) + words[-1].bit_length() - 1
    return bits[:top][::-1]


def decode(words, count, semantics, B=32):
    """-> (symbols, ok, bits left unread): `count` symbols; after an invalid codeword the rest reads 0 and ok is False"""
    bits = read_bits(words, semantics)
    if bits is None:
        return [0] * count, False, 0
    out, pos, ok = [], 0, True
    for _ in range(count):
        sym = None
        if ok:
            sym, pos = decode_symbol(bits, pos, B)
            ok = sym is not None
        out.append(sym if ok else 0)
    return out, ok, len(bits) - pos
