"""GPU: random access into ragged batches of the two symbol codes (cst_{huffman,exp_golomb}_decode_ragged_select).  What a query
owes is a slice of the INPUT symbols; a query the device refuses owes nothing at all, and its neighbours owe what they always do."""
import numpy as np
import pytest
import torch

import exp_golomb_ref as ER
import huffman_ref as HR

pytestmark = pytest.mark.gpu

OK, INVALID, OUT_OF_DATA = 0, 3, 4
LENGTHS = [0, 1, 31, 32, 33, 64, 65, 200]
N_STREAMS = 130
SENTINEL = 0x55
NP = {torch.int32: np.int32, torch.int16: np.int16, torch.uint8: np.uint8}
UNSIGNED = {torch.int32: np.uint32, torch.int16: np.uint16, torch.uint8: np.uint8}
KINDS = ["huffman-int32", "huffman-long", "huffman-uint8", "eg-uint8", "eg-int16", "eg-int32"]
DTYPE = {"huffman-int32": torch.int32, "huffman-long": torch.int32, "huffman-uint8": torch.uint8, "eg-uint8": torch.uint8, "eg-int16": torch.int16,
         "eg-int32": torch.int32}
BIG = 40 + 7          # a document of 200 symbols (LENGTHS[7]) in the middle of a wave


@pytest.fixture(scope="module")
def B():
    from constriction_amd import batched
    return batched


def dyadic(n):
    """probabilities 2^-1, 2^-2, ..., 2^-(n-1), 2^-(n-1): codeword lengths 1 .. n-1"""
    return np.array([2.0 ** -i for i in range(1, n)] + [2.0 ** -(n - 1)])


class Coder:
    """one of the six coders under test: how it encodes, selects, and what a reader finds at a bit position (the restatements)"""

    def __init__(self, B, kind):
        self.B, self.kind, self.dtype, self.huffman = B, kind, DTYPE[kind], kind.startswith("huffman")
        rng = np.random.default_rng(len(kind) * 31 + ord(kind[-1]))
        if self.huffman:
            probs = {"huffman-int32": lambda: rng.dirichlet(np.ones(300) * 0.5), "huffman-long": lambda: dyadic(34),
                     "huffman-uint8": lambda: rng.dirichlet(np.ones(23) * 0.5)}[kind]()
            self.cb = B.HuffmanCodebook.from_probabilities(probs)
            self.nodes = self.cb.nodes.tolist()
            self.n = len(probs)
            self.children = HR.children(self.nodes)
            lens = [len(c) for c in HR.prefix_codewords(self.nodes)]
            self.longest = int(np.argmax(lens))            # the symbol with the longest codeword
            assert kind != "huffman-long" or max(lens) == 33   # (the node-walking decoder: codewords beyond the table's 12 bits)
            self.kernel = "huffman_decode_ragged_jump_long_kernel<select>" if max(lens) > 12 else "huffman_decode_ragged_jump_kernel<select>"
            self.fail = OUT_OF_DATA
        else:
            self.bits = {"eg-uint8": 8, "eg-int16": 16, "eg-int32": 32}[kind]
            self.longest = (1 << self.bits) - 1
            self.kernel = "exp_golomb_decode_ragged_jump_kernel<select>"
            self.fail = INVALID
        docs = []
        for s in range(N_STREAMS):
            n = LENGTHS[s % len(LENGTHS)]
            if self.huffman:
                d = rng.integers(0, self.n, n)
            else:
                d = np.minimum(rng.geometric(0.08, n) - 1, self.longest)
                if n >= 3 and self.bits == 32:
                    d[:3] = [2 ** 17 - 1, 2 ** 32 - 1, 2 ** 17 - 2]
            docs.append(d.astype(np.uint64))
        docs[BIG][192:] = self.longest                     # (a reader that loses the container's end fails within a few symbols)
        self.docs = docs
        lengths = np.array([len(d) for d in docs], dtype=np.int64)
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).cuda()
        self.flat = torch.from_numpy(np.concatenate(docs).astype(UNSIGNED[self.dtype]).view(NP[self.dtype])).cuda()
        self.batches = {}

    def batch(self, semantics, interval):
        """the batch of (semantics, interval), encoded once; the tests that damage one work on a copy"""
        key = (semantics, interval)
        if key not in self.batches:
            B = self.B
            if self.huffman:
                self.batches[key] = B.huffman_encode_ragged(self.flat, self.offsets, self.cb, semantics, jump_every=interval)
            else:
                self.batches[key] = B.exp_golomb_encode_ragged(self.flat, self.offsets, semantics, jump_every=interval)
            assert self.batches[key].status.tolist() == [OK] * N_STREAMS and (self.batches[key].jump is not None) == (interval != 0)
        return self.batches[key]

    def copy(self, semantics, interval):
        b = self.batch(semantics, interval)
        jump = None if b.jump is None else self.B.BitJump(b.jump.interval, b.jump.chunk_offsets.clone(), b.jump.bits.clone())
        out = self.B.RaggedBatch(b.words.clone(), b.word_offsets.clone(), b.n_words.clone(), b.status.clone(), b.config, jump=jump, coder=b.coder)
        out.n_bits = b.n_bits
        return out

    def select(self, batch, streams, first=None, count=None, out=None):
        if self.huffman:
            return self.B.huffman_decode_ragged_select(batch, self.cb, self.offsets, streams, first, count, out)
        return self.B.exp_golomb_decode_ragged_select(batch, self.offsets, streams, first, count, out)

    def read(self, bits, count):
        """`count` symbols from the bit string in read order -> the symbols found before the bits ran out or a codeword was invalid"""
        out, pos = [], 0
        for _ in range(count):
            if self.huffman:
                v = 2 * self.n - 2
                while v >= self.n:
                    if pos >= len(bits):
                        return out
                    v = self.children[v - self.n][int(bits[pos])]
                    pos += 1
            else:
                v, pos = ER.decode_symbol(bits, pos, self.bits)
                if v is None:
                    return out
            out.append(v)
        return out


CODERS = {}


def coder(B, kind):
    if kind not in CODERS:
        CODERS[kind] = Coder(B, kind)
    return CODERS[kind]


def check(cd, batch, streams, first=None, count=None, dtype=None):
    """every query is OK and owns its slice of the input symbols; the output is pre-filled, and nothing lies behind the last slice"""
    docs = cd.docs
    nq = len(streams)
    f = [0] * nq if first is None else list(first)
    c = [len(docs[s]) - f[q] for q, s in enumerate(streams)] if count is None else list(count)
    total = sum(c)
    dtype = dtype or cd.dtype
    out = torch.full((total + 3,), SENTINEL, dtype=dtype, device="cuda")
    sym, out_offsets, status = cd.select(batch, streams, first, count, out=out)
    assert cd.B.last_kernel() == cd.kernel
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum(c)]).astype(np.int64).tolist()
    assert status.tolist() == [OK] * nq
    assert sym.dtype == dtype and sym.numel() == total and sym.data_ptr() == out.data_ptr()
    want = np.concatenate([docs[s][f[q]: f[q] + c[q]] for q, s in enumerate(streams)] + [np.zeros(0, np.uint64)])
    assert np.array_equal(sym.cpu().numpy().view(UNSIGNED[dtype]).astype(np.uint64), want)
    assert out[total:].tolist() == [SENTINEL] * 3
    return sym


CASES = [(k, s, i) for k in KINDS for s in ("stack", "queue") for i in (32, 64, 0)]


@pytest.mark.parametrize("kind,semantics,interval", CASES)
def test_whole_documents_in_reversed_order(B, kind, semantics, interval):
    cd = coder(B, kind)
    batch = cd.batch(semantics, interval)
    check(cd, batch, list(range(N_STREAMS - 1, -1, -1)))
    # a fresh output comes in the batch's dtype
    sym, _, status = cd.select(batch, [BIG, 0, 1])
    assert sym.dtype == cd.dtype and status.tolist() == [OK] * 3 and sym.numel() == 201
    # the same document three times
    check(cd, batch, [BIG, BIG, BIG])
    check(cd, batch, [BIG, BIG, BIG], [0, 1, 100], [200, 150, 100])


@pytest.mark.parametrize("kind,semantics,interval", CASES)
def test_ranges_at_every_edge(B, kind, semantics, interval):
    cd = coder(B, kind)
    batch = cd.batch(semantics, interval)
    I = interval or 32
    streams, first, count = [], [], []
    for s in (BIG, BIG - 1, BIG - 2, BIG + 8):              # 200, 65, 64 and 200 symbols
        n = len(cd.docs[s])
        for f in (0, 1, I - 1, I, I + 1):
            for c in (0, 1, I - 1, I, I + 1, None):
                c = n - f if c is None else c
                if f <= n and 0 <= c <= n - f:
                    streams.append(s), first.append(f), count.append(c)
    assert len(streams) > 64                                 # (more than one wave of queries)
    check(cd, batch, streams, first, count)


@pytest.mark.parametrize("kind,semantics,interval", CASES)
def test_65_queries(B, kind, semantics, interval):
    """a second wave of queries that is partial, in no order, with repeats and overlaps"""
    cd = coder(B, kind)
    rng = np.random.default_rng(interval + len(kind))
    streams = rng.integers(0, N_STREAMS, 65).tolist()
    first = [int(rng.integers(0, len(cd.docs[s]) + 1)) for s in streams]
    count = [int(rng.integers(0, len(cd.docs[s]) - f + 1)) for s, f in zip(streams, first)]
    check(cd, cd.batch(semantics, interval), streams, first, count)


def seal_of(words):
    return 32 * (len(words) - 1) + int(words[-1]).bit_length() - 1


@pytest.mark.parametrize("kind,semantics,interval", CASES)
def test_bad_queries_between_good_ones(B, kind, semantics, interval):
    cd = coder(B, kind)
    batch = cd.copy(semantics, interval)
    docs = cd.docs
    n = len(docs[BIG])
    # (stream, first, count, refused)
    queries = [(BIG - 1, 0, 65, False),
               (N_STREAMS, 0, 0, True),                        # no such stream
               (BIG, 3, 100, False),
               (BIG, n + 1, 1, True),                          # first = len + 1
               (BIG - 2, 1, 63, False),
               (BIG, 150, n - 150 + 1, True),                  # count = len - first + 1
               (BIG, 150, n - 150, False)]
    if interval:                                               # a table entry past its stream's bits: chunk 1 of document BIG + 8 (200 symbols)
        s = BIG + 8
        words = batch.stream(s)
        c0 = int(batch.jump.chunk_offsets[s])
        batch.jump.bits[c0 + 1] = 32 * len(words) + 1 if semantics == "queue" else seal_of(words) + 1
        queries += [(s, 0, interval, False),                   # chunk 0 alone
                    (s, interval - 1, 2, True),                # touches chunk 1
                    (s, 2 * interval, 10, False),
                    (s, 0, 200, True)]
    if semantics == "stack":                                   # a stack without a seal: the last word of document BIG + 16 zeroed
        s = BIG + 16
        batch.words[int(batch.word_offsets[s]) + int(batch.n_words[s]) - 1] = 0
        queries += [(s - 1, 0, 65, False), (s, 0, 200, True), (s, 190, 5, True), (s + 1, 0, 0, False)]
    queries.append((BIG, 0, 200, False))
    streams, first, count, refused = (list(x) for x in zip(*queries))
    # what the Python layer sizes a slice to: the count, never more than the document
    sizes = [min(c, len(docs[s]) if s < N_STREAMS else 0) for s, c in zip(streams, count)]
    total = sum(sizes)
    out = torch.full((total,), SENTINEL, dtype=cd.dtype, device="cuda")
    sym, out_offsets, status = cd.select(batch, streams, first, count, out=out)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()
    assert out_offsets.tolist() == offs
    assert status.tolist() == [INVALID if r else OK for r in refused]
    got = sym.cpu().numpy().view(UNSIGNED[cd.dtype]).astype(np.uint64)
    for q, (s, f, c, r) in enumerate(queries):
        mine = got[offs[q]: offs[q + 1]]
        if r:
            assert (mine == SENTINEL).all(), q                # a refused query writes nothing
        else:
            assert np.array_equal(mine, docs[s][f: f + c]), q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("interval", [32, 0])
def test_a_piece_that_fails_inside_its_dropped_symbols(B, kind, interval):
    """a queue that has lost its end: the last piece of document BIG runs out of bits among the symbols it drops, stores zeros and
    reports the coder's status for that; its neighbours and the other pieces of the same document are exact"""
    cd = coder(B, kind)
    batch = cd.copy("queue", interval)
    doc = cd.docs[BIG]
    words = batch.stream(BIG).tolist()
    if interval:
        entry = int(batch.jump.bits[int(batch.jump.chunk_offsets[BIG]) + 192 // interval])
        keep = (entry + 31) // 32                              # the entry still lies inside the bits: the query is not refused
        start = entry
    else:
        keep, start = 1, 0
    batch.n_words[BIG] = keep
    allbits = ER._bits(words[:keep])
    found = cd.read(allbits[start:], 198 - (192 if interval else 0))
    assert len(found) < 198 - (192 if interval else 0)         # the restatement runs out inside the dropped symbols too
    queries = [(BIG - 1, 0, 65), (BIG, 198, 2), (BIG + 2, 0, 1)] + ([(BIG, 0, 64)] if interval else [])
    streams, first, count = (list(x) for x in zip(*queries))
    sym, out_offsets, status = cd.select(batch, streams, first, count)
    assert status.tolist() == [OK, cd.fail, OK] + ([OK] if interval else [])
    got = sym.cpu().numpy().view(UNSIGNED[cd.dtype]).astype(np.uint64)
    offs = out_offsets.tolist()
    assert got[offs[1]: offs[2]].tolist() == [0, 0]
    for q in (0, 2) + ((3,) if interval else ()):
        s, f, c = queries[q]
        assert np.array_equal(got[offs[q]: offs[q + 1]], cd.docs[s][f: f + c]), q
    assert not np.array_equal(doc[198:], [0, 0])


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_out_of_the_other_dtype(B, semantics):
    for kind, other in (("huffman-uint8", torch.int32), ("eg-uint8", torch.int32), ("eg-uint8", torch.int16)):
        cd = coder(B, kind)
        for interval in (32, 0):
            check(cd, cd.batch(semantics, interval), [BIG, 3, BIG - 1], [5, 0, 60], [190, 31, 5], dtype=other)
    cd = coder(B, "huffman-int32")
    with pytest.raises(Exception):                             # 300 symbols do not fit uint8
        cd.select(cd.batch(semantics, 32), [0], out=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        cd.select(cd.batch(semantics, 32), [0], out=torch.zeros(8, dtype=torch.int16, device="cuda"))


@pytest.mark.parametrize("kind", ["huffman-uint8", "eg-int16"])
def test_no_queries_and_empty_queries(B, kind):
    cd = coder(B, kind)
    batch = cd.batch("stack", 32)
    sym, out_offsets, status = cd.select(batch, torch.zeros(0, dtype=torch.int64))
    assert sym.numel() == 0 and out_offsets.tolist() == [0] and status.numel() == 0
    sym, out_offsets, status = cd.select(batch, [BIG, 0, BIG], [10, 0, 200], [0, 0, 0])
    assert sym.numel() == 0 and out_offsets.tolist() == [0, 0, 0, 0] and status.tolist() == [OK] * 3


def test_refusals(B):
    hf, eg = coder(B, "huffman-uint8"), coder(B, "eg-uint8")
    hb, eb = hf.batch("queue", 32), eg.batch("queue", 32)
    with pytest.raises(ValueError, match="'huffman' decoder"):
        B.huffman_decode_ragged_select(eb, hf.cb, eg.offsets, [0])
    with pytest.raises(ValueError, match="'exp_golomb' decoder"):
        B.exp_golomb_decode_ragged_select(hb, hf.offsets, [0])
    model = B.Model.quantized_gaussian(0, 255, 8.0, 4.0, 24)
    flat32 = eg.flat.to(torch.int32)
    ans = B.ans_encode_ragged(flat32, eg.offsets, model, jump_every=32)
    rng_ = B.range_encode_ragged(flat32, eg.offsets, model)
    for theirs in (ans, rng_):
        with pytest.raises(ValueError, match="'huffman' decoder"):
            B.huffman_decode_ragged_select(theirs, hf.cb, eg.offsets, [0])
        with pytest.raises(ValueError, match="'exp_golomb' decoder"):
            B.exp_golomb_decode_ragged_select(theirs, eg.offsets, [0])
    for mine in (hb, eb):
        with pytest.raises(ValueError, match="'ans' decoder"):
            B.ans_decode_ragged_select(mine, model, eg.offsets, [0])
        with pytest.raises(ValueError, match="'range' decoder"):
            B.range_decode_ragged_select(mine, model, eg.offsets, [0])
    wrong = eg.copy("queue", 32)
    wrong.jump = ans.jump
    with pytest.raises(ValueError, match="jump points of another coder"):
        B.exp_golomb_decode_ragged_select(wrong, eg.offsets, [0])
    wrong = hf.copy("queue", 32)
    wrong.jump = ans.jump
    with pytest.raises(ValueError, match="jump points of another coder"):
        B.huffman_decode_ragged_select(wrong, hf.cb, hf.offsets, [0])
    with pytest.raises(TypeError):
        B.exp_golomb_decode_ragged_select(eb, eg.offsets, [0.5])
