"""GPU: jump points of the ragged Exp-Golomb coders (cst_exp_golomb_{encode,decode}_ragged_jump) against the plain-Python restatement
of tests/exp_golomb_ref.py: the words are the plain ragged call's, the table follows its two formulas, the chunk-lane decoder gives
the input back whichever table it reads, and bad input in one stream leaves its neighbours in the same wave alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import exp_golomb_ref as R

pytestmark = pytest.mark.gpu

OK, CAPACITY, INVALID = 0, 2, 3
DTYPES = {8: (torch.uint8, np.uint8), 16: (torch.int16, np.uint16), 32: (torch.int32, np.uint32)}
LENGTHS = [0, 1, 31, 32, 33, 64, 65, 200]
ENC_KERNEL, DEC_KERNEL, PLAIN_DEC_KERNEL = "exp_golomb_encode_ragged_jump_kernel", "exp_golomb_decode_ragged_jump_kernel", "exp_golomb_decode_ragged_kernel"


@pytest.fixture(scope="module")
def B():
    from constriction_amd import batched
    return batched


def lengths_of(n_streams, shift=0):
    return [LENGTHS[(s + shift) % len(LENGTHS)] for s in range(n_streams)]


def draw(rng, kind, lengths, bits, interval):
    """documents of unsigned values below 2^bits"""
    top = (1 << bits) - 1
    docs = []
    for n in lengths:
        if kind == "zero":
            d = np.zeros(n, dtype=np.uint64)
        elif kind == "max":
            d = np.full(n, top, dtype=np.uint64)
        elif kind == "geometric":
            d = np.minimum(rng.geometric(0.08, n).astype(np.uint64) - 1, top)
        else:                   # u32: the values around the two-piece threshold and the type's end, on the chunk boundary
            d = np.minimum(rng.geometric(0.3, n).astype(np.uint64) - 1, top)
            edge = [2 ** 17 - 2, 2 ** 17 - 1, 2 ** 17, 2 ** 32 - 2, 2 ** 32 - 1, 0]
            for k, pos in enumerate((interval - 1, interval, interval + 1)):
                if pos < n:
                    d[pos] = edge[(k + n) % 3 + (3 if n % 2 else 0)]
            if n >= 3:
                d[:3] = [2 ** 17 - 1, 2 ** 32 - 1, 2 ** 17 - 2]
        docs.append(d)
    return docs


def device(docs, bits):
    tdtype, ndtype = DTYPES[bits]
    lengths = np.array([len(d) for d in docs], dtype=np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).cuda()
    flat = np.concatenate(docs).astype(ndtype) if docs else np.zeros(0, ndtype)
    return torch.from_numpy(flat.view({8: np.uint8, 16: np.int16, 32: np.int32}[bits])).cuda(), offsets


def unsigned(t, bits):
    return t.cpu().numpy().view(DTYPES[bits][1]).astype(np.uint64)


def code_lengths(doc):
    """2 floor(log2(x + 1)) + 1 for every symbol"""
    return np.array([2 * ((int(x) + 1).bit_length() - 1) + 1 for x in doc], dtype=np.int64)


def table_of(doc, interval, semantics):
    """queue: the bits of doc[: j I]; stack: the bits of doc[j I :]"""
    total = np.concatenate([[0], np.cumsum(code_lengths(doc))])
    starts = np.arange(0, len(doc), interval)
    return (total[starts] if semantics == "queue" else total[-1] - total[starts]).tolist()


def check_decoded(B, batch, docs, offsets, bits, kernel):
    dec, status = B.exp_golomb_decode_ragged(batch, offsets)
    assert B.last_kernel() == kernel or not len(docs)
    assert status.tolist() == [OK] * len(docs) and dec.dtype == DTYPES[bits][0]
    assert np.array_equal(unsigned(dec, bits), np.concatenate(docs) if docs else np.zeros(0, np.uint64))


def check_jump(B, docs, bits, semantics, interval, ref_streams=()):
    flat, offsets = device(docs, bits)
    plain = B.exp_golomb_encode_ragged(flat, offsets, semantics)
    assert plain.jump is None and B.last_kernel() == "exp_golomb_encode_ragged_kernel"
    batch = B.exp_golomb_encode_ragged(flat, offsets, semantics, jump_every=interval)
    assert B.last_kernel() == ENC_KERNEL
    assert batch.coder == "exp_golomb" and batch.status.tolist() == [OK] * len(docs) and batch.config == (semantics, DTYPES[bits][0])
    # the plain call's words and bit counts, bit for bit (what lies behind a stream's words in its slab is nobody's)
    assert torch.equal(batch.n_words, plain.n_words) and torch.equal(batch.word_offsets, plain.word_offsets) and torch.equal(batch.n_bits, plain.n_bits)
    assert batch.n_bits.tolist() == [int(code_lengths(d).sum()) for d in docs]
    used = torch.zeros(batch.words.numel() + 1, dtype=torch.int32, device="cuda")
    used.index_add_(0, batch.word_offsets[:-1], torch.ones_like(batch.n_words))
    used.index_add_(0, batch.word_offsets[:-1] + batch.n_words, -torch.ones_like(batch.n_words))
    used = used.cumsum(0)[:-1] > 0
    assert torch.equal(batch.words[used], plain.words[used]) and int(used.sum()) == int(batch.n_words.sum())
    for s in ref_streams:       # ... which are the restatement's
        enc = R.stack_encode if semantics == "stack" else R.queue_encode
        assert batch.stream(s).tolist() == enc([int(x) for x in docs[s]], bits)[0], s
    jump = batch.jump
    assert isinstance(jump, B.BitJump) and jump.interval == interval
    chunks = [-(-len(d) // interval) for d in docs]
    assert jump.chunk_offsets.tolist() == np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64).tolist()
    table = [e for d in docs for e in table_of(d, interval, semantics)]
    assert jump.bits[: len(table)].tolist() == table
    check_decoded(B, batch, docs, offsets, bits, DEC_KERNEL)
    # a table computed here, without the encoder, decodes the plain call's words
    plain.jump = B.BitJump(interval, jump.chunk_offsets.clone(), torch.tensor(table + [0], dtype=torch.int64).cuda())
    check_decoded(B, plain, docs, offsets, bits, DEC_KERNEL)
    # and a reader that ignores the table loses only speed
    batch.jump = None
    check_decoded(B, batch, docs, offsets, bits, PLAIN_DEC_KERNEL)
    batch.jump = jump
    return batch, flat, offsets


def test_the_restatements_table_is_the_formula():
    """table_of (codeword lengths) against the restatement's bit strings, once, on the values the u32 cases place on chunk boundaries"""
    doc = [0, 2 ** 17 - 2, 2 ** 17 - 1, 2 ** 17, 2 ** 32 - 2, 2 ** 32 - 1, 5]
    for interval in (1, 2, 3):
        assert table_of(doc, interval, "queue") == [len(R.queue_bits(doc[: j])) for j in range(0, len(doc), interval)]
        assert table_of(doc, interval, "stack") == [len(R.stack_bits(doc[j:])) for j in range(0, len(doc), interval)]


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("interval", [32, 64])
@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 130])
def test_jump_points(B, semantics, interval, bits, n_streams):
    rng = np.random.default_rng(n_streams * 131 + interval + bits)
    kinds = ["zero", "max", "geometric"] + (["edges"] if bits == 32 else [])
    for k, kind in enumerate(kinds):
        lengths = [200] if n_streams == 1 else lengths_of(n_streams, k)
        docs = draw(rng, kind, lengths, bits, interval)
        check_jump(B, docs, bits, semantics, interval, ref_streams=range(0, n_streams, 37))


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_two_piece_codewords_sit_on_chunk_boundaries(B, semantics):
    """u32 symbols of 2^k - 2, 2^k - 1, 2^k around k = 17 (the first that goes in two pieces) and 32 at positions I - 1, I, I + 1: a
    jump point is the container's length after the WHOLE codeword"""
    for interval in (32, 64):
        docs = []
        for a, b, c in ((2 ** 17 - 2, 2 ** 17 - 1, 2 ** 17), (2 ** 17 - 1, 2 ** 17 - 1, 2 ** 17 - 1), (2 ** 32 - 2, 2 ** 32 - 1, 0),
                        (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (2 ** 17, 2 ** 32 - 1, 2 ** 17 - 2)):
            d = np.arange(2 * interval + 5, dtype=np.uint64) % 7
            d[interval - 1: interval + 2] = [a, b, c]
            d[2 * interval - 1: 2 * interval + 2] = [c, b, a]
            docs.append(d)
        batch, _, _ = check_jump(B, docs, 32, semantics, interval, ref_streams=range(len(docs)))
        for s, d in enumerate(docs):
            c0 = int(batch.jump.chunk_offsets[s])
            want = [len(R.queue_bits([int(x) for x in d[: j]])) if semantics == "queue" else len(R.stack_bits([int(x) for x in d[j:]]))
                    for j in range(0, len(d), interval)]
            assert batch.jump.bits[c0: c0 + 3].tolist() == want


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("n_streams", [1, 65])
def test_all_streams_empty(B, semantics, n_streams):
    docs = [np.zeros(0, dtype=np.uint64)] * n_streams
    batch, _, offsets = check_jump(B, docs, 16, semantics, 32)
    assert batch.n_words.tolist() == [1 if semantics == "stack" else 0] * n_streams
    assert batch.jump.chunk_offsets.tolist() == [0] * (n_streams + 1)


# ---- bad input between good neighbours in one wave ----

def neighbours_exact(dec, docs, offsets, damaged, bits=32):
    dec, offs = unsigned(dec, bits), offsets.tolist()
    for s, d in enumerate(docs):
        if s not in damaged:
            assert np.array_equal(dec[offs[s]: offs[s + 1]], d), s


def setup_bad(B, semantics, interval=32, bits=32):
    rng = np.random.default_rng(77)
    docs = draw(rng, "geometric", [n or 7 for n in lengths_of(70, 3)], bits, interval)
    docs[40] = np.minimum(rng.geometric(0.08, 200).astype(np.uint64) - 1, (1 << bits) - 1)
    flat, offsets = device(docs, bits)
    batch = B.exp_golomb_encode_ragged(flat, offsets, semantics, jump_every=interval)
    return docs, flat, offsets, batch


def chunk_expectation(doc, words, table, interval, semantics, bits=32):
    """what the jump decoder owes for one stream whose words or table have been damaged: (symbols, status)"""
    allbits = R._bits(words)
    if semantics == "queue":
        limit = len(allbits)
    else:
        limit = 32 * (len(words) - 1) + int(words[-1]).bit_length() - 1 if len(words) and words[-1] else -1
    out, worst = [], OK
    for j, p in enumerate(table):
        count = min(interval, len(doc) - j * interval)
        got = []
        if p > limit:
            worst = INVALID
        else:
            stream, pos = (allbits[p:] if semantics == "queue" else allbits[:p][::-1]), 0
            for _ in range(count):
                sym, pos = R.decode_symbol(stream, pos, bits)
                if sym is None:
                    worst = INVALID
                    break
                got.append(sym)
        out += got + [0] * (count - len(got))
    return out, worst


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("damage", ["n_words_minus_one", "entry_beyond_the_bits", "last_word_zeroed"])
def test_damaged_stream_between_good_neighbours(B, semantics, damage):
    interval = 32
    docs, flat, offsets, batch = setup_bad(B, semantics, interval)
    s = 40                                                          # 200 symbols: seven chunks
    c0 = int(batch.jump.chunk_offsets[s])
    table = batch.jump.bits[c0: c0 + 7].tolist()
    words = batch.stream(s).tolist()
    base = int(batch.word_offsets[s])
    doc = [int(x) for x in docs[s]]
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
    want, want_status = chunk_expectation(doc, words, table, interval, semantics)
    if damage == "entry_beyond_the_bits":
        assert want_status == INVALID and want[96:128] == [0] * 32 and want[:96] == doc[:96] and want[128:] == doc[128:]
    if damage == "last_word_zeroed" and semantics == "stack":
        assert want_status == INVALID and want == [0] * 200
    if damage == "n_words_minus_one":        # the failing chunk reads zeros from the failure to its own end, the other chunks are intact
        assert want_status == INVALID
        if semantics == "queue":             # the last chunk loses its end
            assert want[:192] == doc[:192] and want[-1] == 0
        else:                                # every entry but the lowest lies beyond the shortened container... or a stale bit is its seal
            assert want != doc
    dec, status = B.exp_golomb_decode_ragged(batch, offsets)
    assert B.last_kernel() == DEC_KERNEL
    expect = [OK] * len(docs)
    expect[s] = want_status
    assert status.tolist() == expect
    neighbours_exact(dec, docs, offsets, {s})
    assert unsigned(dec[int(offsets[s]): int(offsets[s + 1])], 32).tolist() == want
    # the plain decoder on the same words (it does not look at the table)
    batch.jump = None
    dec, status = B.exp_golomb_decode_ragged(batch, offsets)
    plain, ok, _ = R.decode(words, 200, semantics)
    expect[s] = OK if ok else INVALID
    assert status.tolist() == expect and unsigned(dec[int(offsets[s]): int(offsets[s + 1])], 32).tolist() == plain
    neighbours_exact(dec, docs, offsets, {s})


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_a_table_with_one_chunk_too_many(B, semantics):
    docs, flat, offsets, batch = setup_bad(B, semantics)
    chunk_offsets = batch.jump.chunk_offsets.clone()
    chunk_offsets[41:] += 1                                         # stream 40 claims a chunk too many
    batch.jump = B.BitJump(32, chunk_offsets, torch.cat([batch.jump.bits, torch.zeros(1, dtype=torch.int64, device="cuda")]))
    out = torch.full((int(offsets[-1]),), -7, dtype=torch.int32, device="cuda")
    dec, status = B.exp_golomb_decode_ragged(batch, offsets, out=out)
    assert status[40].item() == INVALID and (dec[int(offsets[40]): int(offsets[41])] == -7).all()       # nothing is written for it
    assert status[:40].tolist() == [OK] * 40
    neighbours_exact(dec, docs, offsets, set(range(40, len(docs))))


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_slab_one_word_short(B, semantics):
    from constriction_amd import _native as N
    docs, flat, offsets, good = setup_bad(B, semantics)
    n_words = good.n_words.tolist()
    slabs = list(n_words)                       # exact to the word (not to 16 bytes), and one stream a word short
    slabs[40] -= 1
    word_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(slabs)]).astype(np.int64)).cuda()
    words = torch.zeros(sum(slabs) + 4, dtype=torch.int32, device="cuda")
    out_n = torch.zeros(len(docs), dtype=torch.int32, device="cuda")
    out_bits = torch.zeros(len(docs), dtype=torch.int64, device="cuda")
    status = torch.zeros(len(docs), dtype=torch.int32, device="cuda")
    n_chunks = int(good.jump.chunk_offsets[-1])
    table = torch.full((n_chunks + 1,), -5, dtype=torch.int64, device="cuda")

    def p(t):
        return C.c_void_p(t.data_ptr())

    N.check(N.lib().cst_exp_golomb_encode_ragged_jump(N.SYMBOL_STACK if semantics == "stack" else N.SYMBOL_QUEUE, p(flat), 4, p(offsets), len(docs),
                                                      p(words), p(word_offsets), 0, p(out_n), p(out_bits), 32, p(good.jump.chunk_offsets),
                                                      p(table), p(status), None))
    want = [OK] * len(docs)
    want[40] = CAPACITY
    assert status.tolist() == want
    n_words[40] = 0
    assert out_n.tolist() == n_words and int(out_bits[40]) == 0
    host, offs = words.cpu().numpy().view(np.uint32), word_offsets.tolist()
    for s in (0, 39, 41, 69):
        assert host[offs[s]: offs[s] + n_words[s]].tolist() == good.stream(s).tolist(), s
    assert host[-4:].tolist() == [0, 0, 0, 0]
    # the other streams' entries are the good call's, and nothing lies outside the table
    c0, c1 = int(good.jump.chunk_offsets[40]), int(good.jump.chunk_offsets[41])
    assert table[:c0].tolist() == good.jump.bits[:c0].tolist() and table[c1:n_chunks].tolist() == good.jump.bits[c1:n_chunks].tolist()
    assert int(table[n_chunks]) == -5


# ---- the Python layer ----

def test_refusals(B):
    docs = draw(np.random.default_rng(1), "geometric", [10, 40, 70], 32, 32)
    flat, offsets = device(docs, 32)
    batch = B.exp_golomb_encode_ragged(flat, offsets, "queue", jump_every=32)
    for decode in (B.ans_decode_ragged, B.range_decode_ragged):
        with pytest.raises(ValueError, match="exp_golomb"):
            decode(batch, None, offsets)
    with pytest.raises(ValueError, match="exp_golomb"):
        B.huffman_decode_ragged(batch, None, offsets)
    model = B.Model.quantized_gaussian(0, 255, 8.0, 4.0, 24)
    theirs = B.ans_encode_ragged(flat.clamp(0, 255), offsets, model, jump_every=32)
    batch.jump = theirs.jump
    with pytest.raises(ValueError, match="jump points"):
        B.exp_golomb_decode_ragged(batch, offsets)
    with pytest.raises(ValueError, match="jump_every"):
        B.exp_golomb_encode_ragged(flat, offsets, "queue", jump_every=33)


def test_auto_takes_the_huffman_coders_rule(B):
    rng = np.random.default_rng(2)
    for n, jumps in ((B.RAGGED_JUMP_EVERY, False), (B.RAGGED_JUMP_EVERY + 1, True)):
        docs = draw(rng, "geometric", [n] * 3, 8, 32)
        flat, offsets = device(docs, 8)
        batch = B.exp_golomb_encode_ragged(flat, offsets, "stack", jump_every="auto")
        assert (batch.jump is not None) == jumps
        if jumps:
            assert batch.jump.interval == B.RAGGED_JUMP_EVERY
        check_decoded(B, batch, docs, offsets, 8, DEC_KERNEL if jumps else PLAIN_DEC_KERNEL)
