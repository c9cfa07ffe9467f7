"""Test helper: a plain-Python restatement of the reference's Huffman symbol codes, written from the rules of
src/symbol/huffman.rs and src/symbol/mod.rs (tree construction, codeword orders, bit containers), for the tests to compare the
library against.  Slow and simple on purpose."""
import heapq

import numpy as np


def tree(probabilities, f32):
    """nodes[2n - 1]: pop the two smallest (p, index), ties on the index, first popped = bit 0; sums in f32 or f64"""
    n = len(probabilities)
    heap = [(float(np.float32(p)) if f32 else float(p), i) for i, p in enumerate(probabilities)]
    heapq.heapify(heap)
    nodes = [0] * (2 * n - 1)
    nxt = n
    while len(heap) >= 2:
        p0, i0 = heapq.heappop(heap)
        p1, i1 = heapq.heappop(heap)
        s = float(np.float32(p0) + np.float32(p1)) if f32 else p0 + p1
        heapq.heappush(heap, (s, nxt))
        nodes[i0] = nxt << 1
        nodes[i1] = (nxt << 1) | 1
        nxt += 1
    return nodes


def suffix_codewords(nodes):
    """per symbol the bits leaf to root (what a stack writes), as '0' / '1' strings"""
    n = (len(nodes) + 1) // 2
    out = []
    for s in range(n):
        bits, v = [], s
        while nodes[v] != 0:
            bits.append("1" if nodes[v] & 1 else "0")
            v = nodes[v] >> 1
        out.append("".join(bits))
    return out


def prefix_codewords(nodes):
    return [c[::-1] for c in suffix_codewords(nodes)]


def _words(bits):
    """bits in write order -> u32 words, each filled from bit 0 upwards"""
    if not bits:
        return []
    value = int(bits[::-1], 2)
    return [(value >> (32 * k)) & 0xFFFFFFFF for k in range((len(bits) + 31) // 32)]


def queue_encode(nodes, message, codes=None):
    codes = codes or prefix_codewords(nodes)
    bits = "".join(codes[x] for x in message)
    return _words(bits), len(bits)


def stack_encode(nodes, message, codes=None):
    """StackCoder: encode_symbol(x) for x in reversed(message), then get_compressed_and_bitrate()"""
    codes = codes or suffix_codewords(nodes)
    bits = "".join(codes[x] for x in reversed(message))
    return _words(bits + "1"), len(bits)


def children(nodes):
    n = (len(nodes) + 1) // 2
    ch = [[None, None] for _ in range(n - 1)]
    for i in range(len(nodes) - 1):
        ch[(nodes[i] >> 1) - n][nodes[i] & 1] = i
    return ch


def decode(nodes, words, count, semantics):
    """-> (symbols, out_of_data); a stack is found by the highest set bit of its last word"""
    n = (len(nodes) + 1) // 2
    ch = children(nodes)
    if semantics == "queue":
        bits = "".join(format(w, "032b")[::-1] for w in words)
    else:
        last = words[-1]
        top = last.bit_length() - 1
        bits = "".join(format(w, "032b")[::-1] for w in words[:-1]) + format(last, "032b")[::-1][:top]
        bits = bits[::-1]
    out, pos = [], 0
    for _ in range(count):
        v = 2 * n - 2
        while v >= n:
            if pos >= len(bits):
                return out, True
            v = ch[v - n][int(bits[pos])]
            pos += 1
        out.append(v)
    return out, False
