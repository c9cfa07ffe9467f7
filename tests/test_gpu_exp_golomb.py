"""GPU: the batched and ragged Exponential-Golomb coders (cst_exp_golomb_*) against the known answers of
tests/golden/exp_golomb_vectors.json and the bit-by-bit restatement of tests/exp_golomb_ref.py: words, word counts, bit counts and
statuses of every stream, then decoded back."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import exp_golomb_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "exp_golomb_vectors.json").read_text())
OK, CAPACITY, INVALID_DATA = 0, 2, 3
TYPES = {8: (torch.uint8, np.uint8, np.uint8), 16: (torch.int16, np.uint16, np.int16), 32: (torch.int32, np.uint32, np.int32)}
N_STREAMS = (1, 63, 64, 65, 130)          # a partial wave, a full wave, a wave plus one, two waves and a bit
N_PER = (0, 1, 31, 32, 33, 100)           # around the 32-symbol tile and the 32-bit word


@pytest.fixture(scope="module")
def B():
    from constriction_amd import batched
    return batched


def device(values, bits):
    """unsigned values (any integer array) -> the device tensor of the width's type (the bit pattern for u16 / u32)"""
    _, unsigned, signed = TYPES[bits]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.uint64).astype(unsigned).view(signed))).cuda()


def host(t, bits):
    """device symbols -> unsigned values"""
    return t.cpu().numpy().view(TYPES[bits][1]).astype(np.uint64)


def expected(rows, semantics, bits):
    enc = R.stack_encode if semantics == "stack" else R.queue_encode
    return [enc([int(x) for x in row], bits) for row in rows]


def check_batch(batch, want, bad=()):
    words, n_words, status = batch.to_numpy()
    n_bits = batch.n_bits.cpu().numpy()
    for s, (w, bits) in enumerate(want):
        if s in bad:
            assert (status[s], n_words[s], n_bits[s]) == (CAPACITY, 0, 0), s
            continue
        assert status[s] == OK, s
        assert n_bits[s] == bits, s
        assert n_words[s] == len(w), s
        assert words[s, : n_words[s]].tolist() == w, s


def mix(kind, rng, shape, bits):
    top = (1 << bits) - 1
    if kind == "zeros":
        return np.zeros(shape, dtype=np.uint64)
    if kind == "max":
        return np.full(shape, top, dtype=np.uint64)
    if kind == "geometric":
        return np.minimum(rng.geometric(0.15, shape) - 1, top).astype(np.uint64)
    assert kind == "edges" and bits == 32        # where m = symbol + 1 wraps or gains a bit
    edges = sorted({x & top for k in range(1, 33) for x in ((1 << k) - 2, (1 << k) - 1, 1 << k)})
    assert top in edges and 0 in edges and len(edges) > 90
    return rng.choice(np.array(edges, dtype=np.uint64), shape)


@pytest.mark.parametrize("case", GOLDEN["known_answers"], ids=lambda c: f"{c['semantics']}-u{c['bits']}-{c['symbols'][0]}x{len(c['symbols'])}")
def test_known_answers(B, case):
    sym = device([case["symbols"]], case["bits"])
    batch = B.exp_golomb_encode(sym, case["semantics"])
    assert B.last_kernel() == "exp_golomb_encode_kernel"
    assert batch.status.tolist() == [OK] and batch.stream(0).tolist() == case["words"] and int(batch.n_bits[0]) == case["n_bits"]
    dec, status = B.exp_golomb_decode(batch, len(case["symbols"]), dtype=TYPES[case["bits"]][0])
    assert B.last_kernel() == "exp_golomb_decode_kernel"
    assert status.tolist() == [OK] and host(dec, case["bits"])[0].tolist() == case["symbols"]


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("bits,kind", [(8, "zeros"), (8, "max"), (8, "geometric"), (16, "zeros"), (16, "max"), (16, "geometric"),
                                       (32, "zeros"), (32, "max"), (32, "geometric"), (32, "edges")])
def test_batches_against_the_restatement(B, semantics, bits, kind):
    rng = np.random.default_rng(bits * 7 + len(kind))
    for n_streams in N_STREAMS:
        for n_per in N_PER:
            rows = mix(kind, rng, (n_streams, n_per), bits)
            want = expected(rows, semantics, bits)
            sym = device(rows, bits)
            assert B.exp_golomb_count_bits(sym).tolist() == [b for _, b in want]
            batch = B.exp_golomb_encode(sym, semantics)
            longest = max(b for _, b in want) + (semantics == "stack")
            assert batch.stride == ((longest + 31) // 32 + 3) // 4 * 4              # stride="exact": the longest stream, in 16-byte units
            check_batch(batch, want)
            dec, status = B.exp_golomb_decode(batch, n_per, dtype=TYPES[bits][0])
            assert (status.cpu().numpy() == OK).all(), (n_streams, n_per)
            assert np.array_equal(host(dec, bits), rows), (n_streams, n_per)
    # stride="max" holds the worst case of every width without a count pass
    rows = mix("max", rng, (3, 33), bits)
    batch = B.exp_golomb_encode(device(rows, bits), semantics, stride="max")
    assert batch.stride == B.exp_golomb_max_words(33, TYPES[bits][0], semantics)
    check_batch(batch, expected(rows, semantics, bits))


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_compacted_words_decode(B, semantics):
    rng = np.random.default_rng(11)
    rows = mix("geometric", rng, (130, 33), 32)
    rows[5] = mix("edges", rng, 33, 32)
    batch = B.exp_golomb_encode(device(rows, 32), semantics)
    packed, offsets = B.compact(batch)
    total = int(offsets[-1])
    assert total == batch.total_words()
    want = [w for ws, _ in expected(rows, semantics, 32) for w in ws]
    assert packed[:total].cpu().numpy().view(np.uint32).tolist() == want
    dec, status = B.exp_golomb_decode((packed[:total], batch.n_words), 33, semantics, offsets=offsets)
    assert (status.cpu().numpy() == OK).all() and np.array_equal(host(dec, 32), rows)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("bits", [8, 32])
def test_unaligned_and_short_slabs(B, semantics, bits):
    rng = np.random.default_rng(bits)
    rows = mix("geometric", rng, (130, 100), bits)
    rows[7, 50:] = (1 << bits) - 1                      # one stream much longer than the others
    rows[70] = rows[7]
    want = expected(rows, semantics, bits)
    need = [len(w) for w, _ in want]
    longest = max(need)
    assert need.count(longest) == 2 and longest > 8
    sym = device(rows, bits)
    # a stride that is no multiple of four words: words leave one by one
    odd = longest + (1 if (longest + 1) % 4 else 2)
    assert odd % 4 != 0
    batch = B.exp_golomb_encode(sym, semantics, stride=odd)
    check_batch(batch, want)
    dec, status = B.exp_golomb_decode(batch, 100, dtype=TYPES[bits][0])
    assert (status.cpu().numpy() == OK).all() and np.array_equal(host(dec, bits), rows)
    # one word too few: CAPACITY for exactly the streams that need the word, the others unharmed (both store paths)
    for stride in (longest - 1, (longest - 1) // 4 * 4):
        batch = B.exp_golomb_encode(sym, semantics, stride=stride)
        bad = {s for s, n in enumerate(need) if n > stride}
        assert {7, 70} <= bad and len(bad) < 130
        check_batch(batch, want, bad)


def crafted_streams(semantics, bits, n_per, rng):
    """-> (list of word lists, what each decodes to by the restatement, the indices of the bad streams).  70 streams of one batch: the
    bad ones sit between good neighbours of the same waves."""
    top = (1 << bits) - 1

    def container(read_bits):
        if semantics == "queue":
            return R._words(read_bits)
        return R._words(read_bits[::-1] + "1")

    def aligned(front, tail):
        """read-order bits that end exactly at a word boundary after `tail` (queue: nothing but the end of the words follows)"""
        pad = (-(len(front) + len(tail))) % 32
        return "1" * pad + front + tail          # (`pad` symbols 0 in front)

    streams, bad = [], {}
    good = "".join(R.prefix_codeword(int(x), bits) for x in (3, 0, top, 6))
    bad[3] = container(good + "0" * (bits + 1) + "1" + "0" * 40)                     # B + 1 zeros, then a one
    bad[17] = container(good + "0" * bits + "1" + "0" * (bits - 1) + "1")            # B zeros, a one, a tail that is not zero
    bad[40] = container(aligned(good, "000"))                                         # the stream ends inside the zero run
    bad[63] = container(aligned(good, "00001" + "01"))                                # the stream ends inside the value bits
    bad[64] = container(aligned(good, "0" * bits)) if bits == 32 else container(aligned(good, "0001"))
    if semantics == "stack":
        bad[66] = []                                                                  # an empty stack
        bad[69] = container(good) + [0]                                               # a stack with a zero last word
    rows = mix("geometric", rng, (70, n_per), bits)
    enc = R.stack_encode if semantics == "stack" else R.queue_encode
    for s in range(70):
        streams.append(bad[s] if s in bad else enc([int(x) for x in rows[s]], bits)[0])
    return streams, [R.decode(w, n_per, semantics, bits) for w in streams], sorted(bad)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("bits", [8, 32])
def test_crafted_words(B, semantics, bits):
    n_per = 45
    streams, want, bad = crafted_streams(semantics, bits, n_per, np.random.default_rng(3))
    stride = max(len(w) for w in streams) + 1
    words = np.zeros((70, stride), dtype=np.uint32)
    for s, w in enumerate(streams):
        words[s, : len(w)] = w
    n_words = torch.tensor([len(w) for w in streams], dtype=torch.int32).cuda()
    dec, status = B.exp_golomb_decode((torch.from_numpy(words.view(np.int32)).cuda(), n_words), n_per, semantics, dtype=TYPES[bits][0])
    dec, status = host(dec, bits), status.tolist()
    for s, (symbols, ok, _) in enumerate(want):
        assert ok == (s not in bad), s                        # (the restatement agrees on which streams are broken)
        assert status[s] == (OK if ok else INVALID_DATA), s
        assert dec[s].tolist() == symbols, s                  # zeros from the failing symbol on
    for s in bad:
        assert 0 in want[s][0] and not any(want[s][0][-3:])


def raw_encode(B, sym, bits, semantics, cont):
    """cst_exp_golomb_encode_batch with d_cont: -> (completed words per stream, cont after)"""
    from constriction_amd import _native as N
    n_streams, n_per = sym.shape
    stride = B.exp_golomb_max_words(n_per, TYPES[bits][0], semantics)
    words = torch.zeros((n_streams, stride), dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    status = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    cont = cont.clone()
    N.check(N.lib().cst_exp_golomb_encode_batch(N.SYMBOL_STACK if semantics == "stack" else N.SYMBOL_QUEUE, B._ptr(sym), bits // 8, n_streams,
                                                n_per, B._ptr(words), stride, B._ptr(n_words), None, B._ptr(cont), B._ptr(status),
                                                B._stream_ptr()))
    assert (status.cpu().numpy() == OK).all()
    w, n = words.cpu().numpy().view(np.uint32), n_words.tolist()
    return [w[s, : n[s]].tolist() for s in range(n_streams)], cont


def raw_decode(B, words, n_words, n_per, bits, semantics, cont):
    """cst_exp_golomb_decode_batch with d_cont / d_n_words_out: -> (symbols, cont after, n_words_out)"""
    from constriction_amd import _native as N
    n_streams = n_words.numel()
    out = torch.zeros((n_streams, n_per), dtype=TYPES[bits][0], device="cuda")
    status = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    n_out = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    cont = cont.clone()
    N.check(N.lib().cst_exp_golomb_decode_batch(N.SYMBOL_STACK if semantics == "stack" else N.SYMBOL_QUEUE, B._ptr(words), None, words.shape[1],
                                                words.numel(), B._ptr(n_words), B._ptr(out), bits // 8, n_streams, n_per, B._ptr(cont),
                                                B._ptr(n_out), B._ptr(status), B._stream_ptr()))
    assert (status.cpu().numpy() == OK).all()
    return host(out, bits), cont, n_out


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_continuation(B, semantics):
    bits, n_streams, n = 32, 70, 40
    rng = np.random.default_rng(17)
    rows = mix("geometric", rng, (n_streams, n), bits)
    rows[1::3] = mix("edges", rng, rows[1::3].shape, bits)
    one_call = B.exp_golomb_encode(device(rows, bits), semantics)
    want = [one_call.stream(s).tolist() for s in range(n_streams)]
    assert want == [w for w, _ in expected(rows, semantics, bits)]
    zero = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
    for k in (1, 17, n - 1):
        # a stack takes a stream's symbols back to front: its first call codes the tail
        first, second = (rows[:, k:], rows[:, :k]) if semantics == "stack" else (rows[:, :k], rows[:, k:])
        w1, cont = raw_encode(B, device(first, bits), bits, semantics, zero)
        w2, cont = raw_encode(B, device(second, bits), bits, semantics, cont)
        for s, c in enumerate(cont.tolist()):
            partial, nbits = c & 0xFFFFFFFF, c >> 32
            assert nbits < 32 and partial >> nbits == 0
            tail = [partial | (1 << nbits)] if semantics == "stack" else ([partial] if nbits else [])
            assert w1[s] + w2[s] + tail == want[s], (k, s)
        # decode in two calls from the one-call words
        if semantics == "stack":
            n_words = one_call.n_words - 1                   # the full words below the sealed partial word
            last = [w[-1] for w in want]
            cont = torch.tensor([(x ^ (1 << (x.bit_length() - 1))) | ((x.bit_length() - 1) << 32) for x in last], dtype=torch.int64).cuda()
        else:
            n_words, cont = one_call.n_words, zero
        d1, cont, n_out = raw_decode(B, one_call.words, n_words, k, bits, semantics, cont)
        if semantics == "stack":
            n_words = n_out
        else:
            assert n_out.tolist() == [(c + 31) // 32 for c in cont.tolist()]
        d2, cont, n_out = raw_decode(B, one_call.words, n_words, n - k, bits, semantics, cont)
        assert np.array_equal(np.concatenate([d1, d2], axis=1), rows), k
        if semantics == "stack":
            assert cont.tolist() == [0] * n_streams and n_out.tolist() == [0] * n_streams        # is_empty
        else:
            assert cont.tolist() == one_call.n_bits.tolist()


def test_failed_decode_leaves_the_continuation_alone(B):
    words = torch.tensor([[20740]], dtype=torch.int32, device="cuda")       # 3, 7, 0, 1 and zero padding
    n_words = torch.ones(1, dtype=torch.int32, device="cuda")
    from constriction_amd import _native as N
    cont = torch.tensor([5], dtype=torch.int64, device="cuda")              # behind symbol 3
    n_out = torch.tensor([77], dtype=torch.int32, device="cuda")
    out = torch.full((1, 4), 9, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    N.check(N.lib().cst_exp_golomb_decode_batch(N.SYMBOL_QUEUE, B._ptr(words), None, 1, 1, B._ptr(n_words), B._ptr(out), 4, 1, 4, B._ptr(cont),
                                                B._ptr(n_out), B._ptr(status), B._stream_ptr()))
    assert status.tolist() == [INVALID_DATA] and out.tolist() == [[7, 0, 1, 0]]
    assert cont.tolist() == [5] and n_out.tolist() == [77]


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("lengths", ["listed", "random"])
@pytest.mark.parametrize("bits", [8, 32])
def test_ragged(B, semantics, lengths, bits):
    rng = np.random.default_rng(29)
    lengths = [0, 1, 5, 64, 2000, 0, 33] if lengths == "listed" else rng.integers(0, 201, 300).tolist()
    docs = [mix("geometric", rng, n, bits) for n in lengths]
    docs[2 % len(docs)][:] = (1 << bits) - 1
    if bits == 32:
        docs[3] = mix("edges", rng, lengths[3], bits)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    flat = device(np.concatenate(docs), bits)
    batch = B.exp_golomb_encode_ragged(flat, offsets, semantics)
    assert B.last_kernel() == "exp_golomb_encode_ragged_kernel"
    assert batch.coder == "exp_golomb" and batch.status.tolist() == [OK] * len(docs)
    want = expected(docs, semantics, bits)
    assert batch.n_bits.tolist() == [b for _, b in want]
    assert batch.n_words.tolist() == [len(w) for w, _ in want]
    slabs = (batch.word_offsets[1:] - batch.word_offsets[:-1]).tolist()
    assert slabs == [(len(w) + 3) // 4 * 4 for w, _ in want]                  # exact slabs in 16-byte units
    for s, (w, _) in enumerate(want):
        assert batch.stream(s).tolist() == w, s
    dec, status = B.exp_golomb_decode_ragged(batch, offsets)
    assert B.last_kernel() == "exp_golomb_decode_ragged_kernel"
    assert status.tolist() == [OK] * len(docs) and dec.dtype == TYPES[bits][0]
    assert np.array_equal(host(dec, bits), np.concatenate(docs))
    with pytest.raises(ValueError, match="exp_golomb"):
        B.ans_decode_ragged(batch, None, offsets)
    with pytest.raises(ValueError, match="exp_golomb"):
        B.range_decode_ragged(batch, None, offsets)


def test_ragged_decoder_reports_broken_documents(B):
    docs = [[3, 7, 0, 1], [5] * 70, [0, 0], [2, 2, 2]]
    offsets = torch.tensor([0, 4, 74, 76, 79], dtype=torch.int64).cuda()
    batch = B.exp_golomb_encode_ragged(device(np.concatenate(docs), 32), offsets, "queue")
    longer = torch.tensor([0, 5, 75, 77, 80], dtype=torch.int64).cuda()       # one symbol more than the first document holds
    dec, status = B.exp_golomb_decode_ragged(batch, longer)
    want = [R.decode(batch.stream(s).tolist(), len(docs[s]) + (s == 0), "queue") for s in range(4)]
    assert status.tolist() == [OK if ok else INVALID_DATA for _, ok, _ in want] and status.tolist()[0] == INVALID_DATA
    assert dec.tolist() == [x for symbols, _, _ in want for x in symbols]
    stack =B.exp_golomb_encode_ragged(device(np.concatenate(docs), 32), offsets, "stack")
    stack.n_words[1] = 0                                                        # a stack without words
    dec, status = B.exp_golomb_decode_ragged(stack, offsets)
    assert status.tolist() == [OK, INVALID_DATA, OK, OK]
    assert dec.tolist() == docs[0] + [0] * 70 + docs[2] + docs[3]
