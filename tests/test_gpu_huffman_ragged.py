"""GPU: the ragged Huffman coders (cst_huffman_count_bits, cst_huffman_{encode,decode}_ragged and their _jump forms) against the
plain-Python restatement of tests/huffman_ref.py: every stream's words are those of the reference's coder for that stream alone,
the jump table follows its two formulas, and bad input in one stream leaves its neighbours alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import huffman_ref as R

pytestmark = pytest.mark.gpu

OK, IMPOSSIBLE, CAPACITY, INVALID, OUT_OF_DATA = 0, 1, 2, 3, 4
NP = {torch.int32: np.int32, torch.uint8: np.uint8}


@pytest.fixture(scope="module")
def B():
    from constriction_amd import batched
    return batched


def dyadic(n):
    """probabilities 2^-1, 2^-2, ..., 2^-(n-1), 2^-(n-1): codeword lengths 1 .. n-1, the longest n-1 (test_gpu_huffman.py)"""
    return np.array([2.0 ** -i for i in range(1, n)] + [2.0 ** -(n - 1)])


class Book:
    """a device codebook with the restatement's codewords beside it"""

    def __init__(self, B, probs):
        self.cb = B.HuffmanCodebook.from_probabilities(probs)
        self.nodes = self.cb.nodes.tolist()
        assert self.nodes == R.tree(probs, probs.dtype == np.float32)
        self.codes = {"stack": R.suffix_codewords(self.nodes), "queue": R.prefix_codewords(self.nodes)}
        self.n = len(probs)
        self.children = R.children(self.nodes)
        longest = max(len(c) for c in self.codes["stack"])
        # codewords of more than 32 bits take the long encoder, of more than 12 (the decode table's bits) the node-walking decoders
        self.enc_kernel = "huffman_encode_ragged_long_kernel" if longest > 32 else "huffman_encode_ragged_kernel"
        self.dec_kernel = "huffman_decode_ragged_long_kernel" if longest > 12 else "huffman_decode_ragged_kernel"
        self.jump_kernel = "huffman_decode_ragged_jump_long_kernel" if longest > 12 else "huffman_decode_ragged_jump_kernel"

    def encode(self, doc, semantics):
        enc = R.stack_encode if semantics == "stack" else R.queue_encode
        return enc(self.nodes, list(doc), self.codes[semantics])

    def table(self, doc, interval, semantics):
        """queue: the bits of doc[: j I]; stack: the bits of doc[j I :]"""
        lens = np.array([len(self.codes[semantics][x]) for x in doc], dtype=np.int64)
        total = np.concatenate([[0], np.cumsum(lens)])
        starts = np.arange(0, len(doc), interval)
        return (total[starts] if semantics == "queue" else total[-1] - total[starts]).tolist()

    def walk(self, bits, count):
        """`count` symbols from the bit string -> (symbols, ran out of bits)"""
        out, pos = [], 0
        for _ in range(count):
            v = 2 * self.n - 2
            while v >= self.n:
                if pos >= len(bits):
                    return out, True
                v = self.children[v - self.n][int(bits[pos])]
                pos += 1
            out.append(v)
        return out, False


BOOKS = {}


def book(B, kind):
    """the codebooks the tests share, built once"""
    if kind not in BOOKS:
        rng = np.random.default_rng(len(kind) * 7919)
        if kind == "int32-f64":
            p = rng.dirichlet(np.ones(300) * 0.5)
        elif kind == "int32-f32":
            p = rng.dirichlet(np.ones(300) * 0.5).astype(np.float32)
        elif kind == "uint8-f64":
            p = rng.dirichlet(np.ones(23) * 0.5)
        elif kind == "uint8-f32":
            p = rng.dirichlet(np.ones(23) * 0.5).astype(np.float32)
        elif kind == "one":
            p = np.array([1.0])
        elif kind == "four":
            p = np.array([0.25, 0.25, 0.25, 0.25])
        elif kind.startswith("dyadic"):
            p = dyadic(int(kind[6:]))
        else:
            p = rng.random(9000) + 1e-3
        BOOKS[kind] = Book(B, p)
    return BOOKS[kind]


def draw(rng, n_streams, pool, n_sym):
    lengths = rng.choice(np.asarray(pool), n_streams)
    return [rng.integers(0, n_sym, int(n)) for n in lengths]


def device(docs, dtype):
    lengths = np.array([len(d) for d in docs], dtype=np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).cuda()
    flat = np.concatenate(docs) if docs else np.zeros(0)
    return torch.from_numpy(flat.astype(NP[dtype])).cuda(), offsets


def check_encoded(batch, bk, docs, semantics):
    """words, n_words, n_bits and status of every stream against the restatement; the slabs are exact"""
    want = [bk.encode(d, semantics) for d in docs]
    assert batch.coder == "huffman" and batch.status.tolist() == [OK] * len(docs)
    assert batch.n_bits.tolist() == [b for _, b in want]
    assert batch.n_words.tolist() == [len(w) for w, _ in want]
    assert (batch.word_offsets[1:] - batch.word_offsets[:-1]).tolist() == [(len(w) + 3) // 4 * 4 for w, _ in want]
    words, offs = batch.words.cpu().numpy().view(np.uint32), batch.word_offsets.tolist()
    for s, (w, _) in enumerate(want):
        assert words[offs[s]: offs[s] + len(w)].tolist() == w, s
    return want


def check_decoded(B, batch, bk, docs, offsets, dtype):
    dec, status = B.huffman_decode_ragged(batch, bk.cb, offsets)
    assert status.tolist() == [OK] * len(docs) and dec.dtype == dtype
    assert np.array_equal(dec.cpu().numpy().astype(np.int64), np.concatenate(docs).astype(np.int64) if docs else np.zeros(0, np.int64))


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("kind", ["int32-f64", "int32-f32", "uint8-f64", "uint8-f32"])
@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 130])
def test_plain_pair(B, semantics, kind, n_streams):
    dtype = torch.int32 if kind.startswith("int32") else torch.uint8
    bk = book(B, kind)
    rng = np.random.default_rng(n_streams * 17 + len(kind))
    docs = draw(rng, n_streams, [0, 1, 31, 32, 33, 100], bk.n)
    flat, offsets = device(docs, dtype)
    batch = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics)
    assert B.last_kernel() == bk.enc_kernel == "huffman_encode_ragged_kernel" and batch.jump is None and batch.config == (semantics, dtype)
    want = check_encoded(batch, bk, docs, semantics)
    check_decoded(B, batch, bk, docs, offsets, dtype)
    assert B.last_kernel() == bk.dec_kernel
    assert B.huffman_count_bits(flat, bk.cb, offsets).tolist() == [b for _, b in want]
    assert B.last_kernel() == "huffman_count_bits_kernel"
    # every stream is huffman_encode of that stream as a one-row batch
    for s in range(0, n_streams, 7 if n_streams > 65 else 1):
        row = B.huffman_encode(flat[int(offsets[s]): int(offsets[s + 1])].reshape(1, -1), bk.cb, semantics)
        assert row.status.tolist() == [OK] and int(row.n_bits[0]) == want[s][1] and row.stream(0).tolist() == batch.stream(s).tolist(), s


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("n_streams", [1, 65])
def test_all_streams_empty(B, semantics, n_streams):
    bk = book(B, "uint8-f64")
    docs = [np.zeros(0, dtype=np.int64)] * n_streams
    flat, offsets = device(docs, torch.uint8)
    for jump_every in (0, 32):
        batch = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics, jump_every=jump_every)
        check_encoded(batch, bk, docs, semantics)
        assert batch.n_words.tolist() == [1 if semantics == "stack" else 0] * n_streams
        check_decoded(B, batch, bk, docs, offsets, torch.uint8)
    assert batch.jump.chunk_offsets.tolist() == [0] * (n_streams + 1)


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_count_bits_of_a_matrix(B, dtype):
    bk = book(B, "uint8-f32")
    sym = np.random.default_rng(3).integers(0, bk.n, (70, 45))
    sym_t = torch.from_numpy(sym.astype(NP[dtype])).cuda()
    bits = B.huffman_count_bits(sym_t, bk.cb)
    assert bits.dtype == torch.int64 and bits.tolist() == B.huffman_encode(sym_t, bk.cb, "queue").n_bits.tolist()
    assert bits.tolist() == [bk.encode(row, "stack")[1] for row in sym.tolist()]
    if dtype == torch.int32:                          # a symbol outside the alphabet counts 0 bits
        sym_t[3, 4], sym_t[5, 0] = -1, bk.n
        want = bits.clone()
        want[3] -= len(bk.codes["stack"][sym[3, 4]])
        want[5] -= len(bk.codes["stack"][sym[5, 0]])
        assert torch.equal(B.huffman_count_bits(sym_t, bk.cb), want)


def check_jump(B, bk, docs, dtype, semantics, interval):
    """the jump encoder and decoder on `docs`: table, words, and every way round the table"""
    enc_kernel, dec_kernel = bk.enc_kernel, bk.jump_kernel
    flat, offsets = device(docs, dtype)
    plain = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics)
    batch = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics, jump_every=interval)
    assert B.last_kernel() == enc_kernel
    check_encoded(batch, bk, docs, semantics)
    # the plain call's words, bit for bit (what lies behind a stream's words in its slab is nobody's)
    assert torch.equal(batch.n_words, plain.n_words) and torch.equal(batch.word_offsets, plain.word_offsets)
    used = torch.zeros(batch.words.numel() + 1, dtype=torch.int32, device="cuda")
    used.index_add_(0, batch.word_offsets[:-1], torch.ones_like(batch.n_words))
    used.index_add_(0, batch.word_offsets[:-1] + batch.n_words, -torch.ones_like(batch.n_words))
    used = used.cumsum(0)[:-1] > 0
    assert torch.equal(batch.words[used], plain.words[used]) and int(used.sum()) == int(batch.n_words.sum())
    jump = batch.jump
    assert isinstance(jump, B.BitJump) and jump.interval == interval
    chunks = [-(-len(d) // interval) for d in docs]
    assert jump.chunk_offsets.tolist() == np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64).tolist()
    table = [e for d in docs for e in bk.table(d, interval, semantics)]
    assert jump.bits[: len(table)].tolist() == table
    check_decoded(B, batch, bk, docs, offsets, dtype)
    assert B.last_kernel() == dec_kernel
    # a table computed here, without the encoder, decodes the plain call's words
    plain.jump = B.BitJump(interval, jump.chunk_offsets.clone(), torch.tensor(table + [0], dtype=torch.int64).cuda())
    check_decoded(B, plain, bk, docs, offsets, dtype)
    assert B.last_kernel() == dec_kernel
    # and a reader that ignores the table loses only speed
    batch.jump = None
    check_decoded(B, batch, bk, docs, offsets, dtype)
    assert B.last_kernel() == bk.dec_kernel
    batch.jump = jump
    return batch, flat, offsets


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("interval", [32, 64])
@pytest.mark.parametrize("n_streams", [1, 64, 65, 130])
def test_jump_points(B, semantics, interval, n_streams):
    rng = np.random.default_rng(n_streams + interval)
    for kind, dtype in (("int32-f64", torch.int32), ("uint8-f32", torch.uint8)):
        bk = book(B, kind)
        docs = draw(rng, n_streams, [0, 1, 32, 33, 64, 65, 200], bk.n)
        if n_streams == 1:
            docs = [rng.integers(0, bk.n, 200)]
        check_jump(B, bk, docs, dtype, semantics, interval)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_one_symbol_alphabet(B, semantics):
    """n = 1: the empty codeword, 0 bits per symbol"""
    bk = book(B, "one")
    assert bk.codes["stack"] == [""]
    docs = [np.zeros(n, dtype=np.int64) for n in (0, 1, 31, 32, 33, 100, 65)]
    batch, _, _ = check_jump(B, bk, docs, torch.uint8, semantics, 32)
    assert batch.n_bits.tolist() == [0] * len(docs) and batch.n_words.tolist() == [1 if semantics == "stack" else 0] * len(docs)
    total = int(batch.jump.chunk_offsets[-1])
    assert total == 12 and batch.jump.bits[:total].tolist() == [0] * total          # all jump entries equal
    check_jump(B, bk, docs, torch.int32, semantics, 64)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_four_equiprobable_symbols_put_jump_points_on_word_boundaries(B, semantics):
    bk = book(B, "four")
    assert sorted(len(c) for c in bk.codes["queue"]) == [2, 2, 2, 2]
    rng = np.random.default_rng(4)
    docs = [rng.integers(0, 4, n) for n in (32, 64, 96, 320, 0, 32)]
    batch, _, _ = check_jump(B, bk, docs, torch.uint8, semantics, 32)
    total = int(batch.jump.chunk_offsets[-1])
    assert total == 17 and (batch.jump.bits[:total] & 31 == 0).all()                # every chunk is 64 bits
    if semantics == "stack":                                                        # the seal sits alone in its last word
        assert batch.n_words.tolist() == [len(d) // 16 + 1 for d in docs]
        assert [batch.stream(s)[-1] for s in range(len(docs))] == [1] * len(docs)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("n", [34, 300])
def test_long_codewords(B, semantics, n):
    """dyadic(34), dyadic(300): the long encoder (codewords of more than 32 bits) and the node-walking decoder (more than 12)"""
    bk = book(B, f"dyadic{n}")
    assert max(len(c) for c in bk.codes["stack"]) == n - 1
    rng = np.random.default_rng(n)
    docs = draw(rng, 70, [0, 1, 32, 33, 65, 100], n)
    for d in docs:
        d[:2] = n - 1                                                               # the longest codewords in every stream
    assert (bk.enc_kernel, bk.dec_kernel, bk.jump_kernel) == ("huffman_encode_ragged_long_kernel", "huffman_decode_ragged_long_kernel",
                                                             "huffman_decode_ragged_jump_long_kernel")
    batch, flat, offsets = check_jump(B, bk, docs, torch.int32, semantics, 32)
    plain = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics)
    assert B.last_kernel() == "huffman_encode_ragged_long_kernel"
    check_decoded(B, plain, bk, docs, offsets, torch.int32)
    assert B.last_kernel() == "huffman_decode_ragged_long_kernel"
    assert B.huffman_count_bits(flat, bk.cb, offsets).tolist() == plain.n_bits.tolist()


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_large_alphabet(B, semantics):
    """9000 symbols: the encoder reads its codeword table from global memory"""
    bk = book(B, "large")
    rng = np.random.default_rng(9000)
    docs = draw(rng, 66, [0, 1, 33, 64, 100], bk.n)
    docs[0][:1] = bk.n - 1
    assert (bk.enc_kernel, bk.jump_kernel) == ("huffman_encode_ragged_kernel", "huffman_decode_ragged_jump_long_kernel")
    check_jump(B, bk, docs, torch.int32, semantics, 64)


# ---- bad input between good neighbours in one wave ----

def neighbours_exact(dec, docs, offsets, damaged):
    dec, offs = dec.cpu().numpy().astype(np.int64), offsets.tolist()
    for s, d in enumerate(docs):
        if s not in damaged:
            assert np.array_equal(dec[offs[s]: offs[s + 1]], d), s


def setup_bad(B, semantics, interval=32):
    bk = book(B, "int32-f64")
    rng = np.random.default_rng(77)
    docs = draw(rng, 70, [1, 32, 33, 64, 65, 200], bk.n)
    docs[40] = rng.integers(0, bk.n, 200)
    flat, offsets = device(docs, torch.int32)
    batch = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics, jump_every=interval)
    return bk, docs, flat, offsets, batch


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("jump_every", [0, 32])
def test_impossible_symbol_in_one_stream(B, semantics, jump_every):
    bk, docs, flat, offsets, _ = setup_bad(B, semantics)
    flat = flat.clone()
    flat[int(offsets[40]) + 77] = bk.n
    flat[int(offsets[41])] = -1
    batch = B.huffman_encode_ragged(flat, offsets, bk.cb, semantics, jump_every=jump_every)
    want = [OK] * len(docs)
    want[40] = want[41] = IMPOSSIBLE
    assert batch.status.tolist() == want
    assert batch.n_words[40:42].tolist() == [0, 0] and batch.n_bits[40:42].tolist() == [0, 0]
    for s in (39, 42):
        assert batch.stream(s).tolist() == bk.encode(docs[s], semantics)[0]
    # the decoder finds no container where the encoder left none (a stack) or runs out of bits (a queue); the others decode
    dec, status = B.huffman_decode_ragged(batch, bk.cb, offsets)
    want[40] = want[41] = INVALID if semantics == "stack" else OUT_OF_DATA
    assert status.tolist() == want
    neighbours_exact(dec, docs, offsets, {40, 41})
    assert (dec[int(offsets[40]): int(offsets[42])] == 0).all()


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_slab_one_word_short(B, semantics):
    from constriction_amd import _native as N
    bk, docs, flat, offsets, good = setup_bad(B, semantics)
    n_words = good.n_words.tolist()
    slabs = list(n_words)                       # exact to the word (not to 16 bytes), and one stream a word short
    slabs[40] -= 1
    word_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(slabs)]).astype(np.int64)).cuda()
    words = torch.zeros(sum(slabs) + 4, dtype=torch.int32, device="cuda")
    out_n = torch.zeros(len(docs), dtype=torch.int32, device="cuda")
    out_bits = torch.zeros(len(docs), dtype=torch.int64, device="cuda")
    status = torch.zeros(len(docs), dtype=torch.int32, device="cuda")

    def p(t):
        return C.c_void_p(t.data_ptr())

    N.check(N.lib().cst_huffman_encode_ragged(bk.cb._h, N.HUFFMAN_STACK if semantics == "stack" else N.HUFFMAN_QUEUE, p(flat), 4, p(offsets),
                                              len(docs), p(words), p(word_offsets), 0, p(out_n), p(out_bits), p(status), None))
    want = [OK] * len(docs)
    want[40] = CAPACITY
    assert status.tolist() == want
    n_words[40] = 0
    assert out_n.tolist() == n_words and int(out_bits[40]) == 0
    host, offs = words.cpu().numpy().view(np.uint32), word_offsets.tolist()
    for s in (0, 39, 41, 69):
        assert host[offs[s]: offs[s] + n_words[s]].tolist() == bk.encode(docs[s], semantics)[0], s
    assert host[-4:].tolist() == [0, 0, 0, 0]


def chunk_expectation(bk, doc, words, table, interval, semantics):
    """what the jump decoder owes for one stream whose words or table have been damaged: (symbols, status)"""
    bits = "".join(format(w, "032b")[::-1] for w in words)
    if semantics == "queue":
        limit = len(bits)
    else:
        limit = 32 * (len(words) - 1) + int(words[-1]).bit_length() - 1 if len(words) and words[-1] else -1
    out, worst = [], OK
    for j, p in enumerate(table):
        count = min(interval, len(doc) - j * interval)
        if p > limit:
            got, st = [], INVALID
        else:
            got, ran_out = bk.walk(bits[p:] if semantics == "queue" else bits[:p][::-1], count)
            st = OUT_OF_DATA if ran_out else OK
        out += got + [0] * (count - len(got))
        worst = max(worst, st)
    return out, worst


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("damage", ["n_words_minus_one", "entry_beyond_the_bits", "last_word_zeroed"])
def test_damaged_stream_between_good_neighbours(B, semantics, damage):
    interval = 32
    bk, docs, flat, offsets, batch = setup_bad(B, semantics, interval)
    s = 40                                                          # 200 symbols: seven chunks
    c0 = int(batch.jump.chunk_offsets[s])
    table = batch.jump.bits[c0: c0 + 7].tolist()
    words = batch.stream(s).tolist()
    base = int(batch.word_offsets[s])
    if damage == "n_words_minus_one":
        batch.n_words[s] -= 1
        words = words[:-1]
    elif damage == "last_word_zeroed":
        batch.words[base + len(words) - 1] = 0
        words[-1] = 0
    else:
        seal = 32 * (len(words) - 1) + int(words[-1]).bit_length() - 1
        table[3] = 32 * len(words) + 1 if semantics == "queue" else seal + 1
        batch.jump.bits[c0 + 3] = table[3]
    want, want_status = chunk_expectation(bk, docs[s], words, table, interval, semantics)
    if damage == "entry_beyond_the_bits":
        assert want_status == INVALID and want[96:128] == [0] * 32 and want[:96] == docs[s][:96].tolist() and want[128:] == docs[s][128:].tolist()
    if damage == "last_word_zeroed" and semantics == "stack":
        assert want_status == INVALID and want == [0] * 200
    if damage == "n_words_minus_one" and semantics == "queue":     # the failing chunk reads zeros from the failure on, the earlier ones are intact
        assert want_status in (INVALID, OUT_OF_DATA) and want[:160] == docs[s][:160].tolist() and want[-1] == 0
    dec, status = B.huffman_decode_ragged(batch, bk.cb, offsets)
    assert B.last_kernel() == bk.jump_kernel
    expect = [OK] * len(docs)
    expect[s] = want_status
    assert status.tolist() == expect
    neighbours_exact(dec, docs, offsets, {s})
    assert dec[int(offsets[s]): int(offsets[s + 1])].tolist() == want
    # the plain decoder on the same words (it does not look at the table)
    batch.jump = None
    dec, status = B.huffman_decode_ragged(batch, bk.cb, offsets)
    got = dec[int(offsets[s]): int(offsets[s + 1])].tolist()
    if semantics == "stack" and (not words or words[-1] == 0):
        expect[s], plain = INVALID, [0] * 200
    else:
        plain, ran_out = R.decode(bk.nodes, words, 200, semantics)
        expect[s], plain = (OUT_OF_DATA if ran_out else OK), plain + [0] * (200 - len(plain))
    assert status.tolist() == expect and got == plain
    neighbours_exact(dec, docs, offsets, {s})


def test_a_table_that_does_not_describe_its_stream(B):
    bk, docs, flat, offsets, batch = setup_bad(B, "queue")
    chunk_offsets = batch.jump.chunk_offsets.clone()
    chunk_offsets[41:] += 1                                         # stream 40 claims a chunk too many
    batch.jump = B.BitJump(32, chunk_offsets, torch.cat([batch.jump.bits, torch.zeros(1, dtype=torch.int64, device="cuda")]))
    out = torch.full((int(offsets[-1]),), -7, dtype=torch.int32, device="cuda")
    dec, status = B.huffman_decode_ragged(batch, bk.cb, offsets, out=out)
    assert status[40].item() == INVALID and (dec[int(offsets[40]): int(offsets[41])] == -7).all()       # nothing is written for it
    neighbours_exact(dec, docs, offsets, set(range(40, len(docs))))


# ---- the Python layer ----

def test_refusals(B):
    bk = book(B, "uint8-f64")
    docs = draw(np.random.default_rng(1), 5, [10, 40], bk.n)
    flat, offsets = device(docs, torch.int32)
    batch = B.huffman_encode_ragged(flat, offsets, bk.cb, "queue")
    for decode in (B.ans_decode_ragged, B.range_decode_ragged):
        with pytest.raises(ValueError, match="huffman"):
            decode(batch, None, offsets)
    with pytest.raises(ValueError, match="huffman"):
        B.exp_golomb_decode_ragged(batch, offsets)
    model = B.Model.quantized_gaussian(0, bk.n - 1, 8.0, 4.0, 24)
    for theirs in (B.ans_encode_ragged(flat, offsets, model), B.range_encode_ragged(flat, offsets, model),
                   B.exp_golomb_encode_ragged(flat, offsets, "queue")):
        with pytest.raises(ValueError, match="'huffman' decoder"):
            B.huffman_decode_ragged(theirs, bk.cb, offsets)
    with pytest.raises(ValueError):
        B.huffman_encode_ragged(flat, offsets, bk.cb, "queue", jump_every=33)
    with pytest.raises(ValueError):
        B.huffman_encode_ragged(flat, offsets, bk.cb, "heap")
    with pytest.raises(TypeError):
        B.huffman_encode_ragged(flat.to(torch.int16), offsets, bk.cb)


def test_auto_takes_the_range_coders_rule(B):
    bk = book(B, "uint8-f64")
    rng = np.random.default_rng(2)
    for n, jumps in ((B.RAGGED_JUMP_EVERY, False), (B.RAGGED_JUMP_EVERY + 1, True)):
        docs = [rng.integers(0, bk.n, n) for _ in range(3)]
        flat, offsets = device(docs, torch.uint8)
        batch = B.huffman_encode_ragged(flat, offsets, bk.cb, "stack", jump_every="auto")
        assert (batch.jump is not None) == jumps
        if jumps:
            assert batch.jump.interval == B.RAGGED_JUMP_EVERY
        check_decoded(B, batch, bk, docs, offsets, torch.uint8)
