"""GPU parity tests of the ragged range coder with a shared table (`cst_range_{encode,decode}_ragged`, `cst_range_count_until`): one
queue per document, one launch.  Every comparison is against the CPU oracle coding that stream ALONE (`O.rc_encode_batch` /
`O.rc_decode_batch` on a one-row matrix); no GPU result is the reference for another, except in the last test, which says so."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from constriction_amd import batched
    return batched


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def oracle_words(O, doc, lo, cdf, cfg):
    """words and status of the reference RangeEncoder for this document alone"""
    W, S, P = cfg
    words, n, st = O.rc_encode_batch(np.asarray(doc, dtype=np.int32)[None, :], lo, cdf, P, W, S)
    return words[0, : n[0]], int(st[0])


def bound(n, cfg):
    W, S, P = cfg
    return min(n, (n * P + W - 1) // W) + 2


def check_all_streams(B, O, docs, enc, lo, cdf, cfg, every=1):
    """statuses 0, counts and words of every `every`-th stream equal the oracle's, inside the documented bound"""
    torch.cuda.synchronize()
    assert enc.coder == "range" and enc.jump is None
    assert (enc.status.cpu().numpy() == 0).all()
    n_words = enc.n_words.cpu().numpy()
    words, off = enc.words.cpu().numpy().view(np.uint32), enc.word_offsets.cpu().numpy()
    for s in range(0, len(docs), every):
        want, st = oracle_words(O, docs[s], lo, cdf, cfg)
        assert st == 0 and n_words[s] == len(want), f"stream {s} of {len(docs[s])} symbols: {n_words[s]} words, the oracle has {len(want)}"
        assert words[off[s]: off[s] + n_words[s]].tolist() == want.tolist(), f"stream {s} of {len(docs[s])} symbols"
        assert n_words[s] <= bound(len(docs[s]), cfg)
    return n_words


@pytest.mark.parametrize("cfg", [(32, 64, 24), (32, 64, 12), (16, 32, 12), (32, 64, 16)], ids=lambda c: "W%dS%dP%d" % c)
def test_every_stream_equals_its_oracle_coder(B, O, cfg):
    """300 documents (a partial last wave, a partial second workgroup) of 0 .. 41, 47 .. 49, 63 .. 65, 700 and random lengths below
    120 over 90 symbols at lo = -17.  Every fifth non-empty document is drawn uniformly over the alphabet; the batch is coded twice,
    with a Dirichlet table and with a table in which all but one symbol have probability 1 / 2^P -- there a uniform document costs
    about P bits per symbol, the most a stream can need.  ALL streams are compared with the oracle, both times."""
    W, S, P = cfg
    rng = np.random.default_rng(P * 7 + W)
    n_sym, lo = 90, -17
    dirichlet = O.categorical_fast_cdf(rng.dirichlet(np.ones(n_sym) * 0.4), P)
    p = np.ones(n_sym, dtype=np.int64)
    p[41] = (1 << P) - (n_sym - 1)
    spiky = np.concatenate([[0], np.cumsum(p)]).astype(np.uint32)
    lengths = np.concatenate([np.arange(0, 42), [47, 48, 49, 63, 64, 65, 700, 0], rng.integers(0, 120, 250)])
    assert len(lengths) == 300
    docs, k = [], 0
    for i, n in enumerate(lengths):
        if n == 0:
            docs.append(np.zeros(0, np.int32))
            continue
        k += 1
        docs.append((lo + rng.integers(0, n_sym, int(n))).astype(np.int32) if k % 5 == 0 else O.synth_symbols(i, 0, 1, int(n), lo, dirichlet, P)[0])
    flat, offsets = B.ragged(docs)
    for cdf in (dirichlet, spiky):
        model = B.Model.from_cdf(cdf, lo, P)
        enc = B.range_encode_ragged(flat, offsets, model, cfg)
        assert B.last_kernel() == "range_encode_ragged_kernel"
        check_all_streams(B, O, docs, enc, lo, cdf, cfg)
        slabs = np.diff(enc.word_offsets.cpu().numpy())
        assert slabs.tolist() == [(bound(int(n), cfg) + 3) // 4 * 4 for n in lengths]
        dec, status = B.range_decode_ragged(enc, model, offsets)
        assert B.last_kernel() == "range_decode_ragged_kernel"
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
        # ... and the oracle's decoder reads the device's words of the longest document
        s = int(np.argmax(lengths))
        got = enc.stream(s)
        back, st = O.rc_decode_batch(got[None, :], np.array([len(got)], np.uint32), len(docs[s]), lo, cdf, P, W, S)
        assert int(st[0]) == 0 and back[0].tolist() == docs[s].tolist()


@pytest.mark.parametrize("cfg,n_sym", [((32, 64, 6), 40), ((16, 32, 5), 20), ((32, 64, 16), 5000), ((32, 64, 20), 20000), ((16, 32, 16), 5000),
                                       ((32, 64, 22), 1000), ((32, 64, 24), 256)],
                         ids=lambda v: "W%dS%dP%d" % v if isinstance(v, tuple) else "n%d" % v)
def test_kernel_variants(B, O, cfg, n_sym):
    """The presets and alphabets of test_ragged_kernel_variants (tests/test_gpu_ragged.py): P < 8, 16-bit words, encoder tables in LDS
    (<= 4096 symbols) and in HBM, decoder tables as 16-byte bucket entries in LDS, as cdf + 16-bit bucket index in LDS, and in HBM.
    190 documents whose lengths cover every residue of the group of eight; the words of EVERY document against the oracle; then the
    terminator-delimited decode -- a queue writes the terminator last -- returns what the decode with known lengths returns."""
    W, S, P = cfg
    rng = np.random.default_rng(n_sym + P)
    lo = -3
    w = rng.gamma(0.3, 1.0, n_sym) + 1e-9
    p = np.maximum(1, np.floor(w / w.sum() * ((1 << P) - n_sym)).astype(np.int64))
    p[int(np.argmax(p))] += (1 << P) - int(p.sum())
    cdf = np.concatenate([[0], np.cumsum(p)]).astype(np.uint32)
    model = B.Model.from_cdf(cdf, lo, P)
    lengths = np.concatenate([np.arange(0, 41), rng.integers(0, 700, 149)])
    assert len(lengths) == 190
    eof = lo + int(np.argmin(p))
    docs = []
    for n in lengths:
        d = lo + rng.choice(n_sym, size=int(n), p=p / p.sum()).astype(np.int32)
        d[d == eof] = lo + int(np.argmax(p))
        docs.append(np.concatenate([d, [eof]]).astype(np.int32))           # the terminator is written -- and read -- last
    flat, offsets = B.ragged(docs)
    enc = B.range_encode_ragged(flat, offsets, model, cfg)
    check_all_streams(B, O, docs, enc, lo, cdf, cfg)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
    dec2, off2, status2 = B.range_decode_until(enc, model, eof)
    torch.cuda.synchronize()
    assert (status2.cpu().numpy() == 0).all() and torch.equal(off2, offsets) and torch.equal(dec2, dec)


def test_like_the_reference_index(B, O):
    """tests/issue52.rs with a queue: documents over a small alphabet, one RangeEncoder each, EOF appended; the words of a document are
    those of the drop-in RangeEncoder for it (constriction_amd.stream.queue), i.e. the reference's; no lengths are stored."""
    from constriction_amd.stream import model as M, queue
    text = ["the quick brown fox", "", "jumps", "over the lazy dog " * 40, "a"] * 30
    alphabet = sorted(set("".join(text)))
    eof = len(alphabet)
    probs = np.ones(eof + 1) / (eof + 1)
    docs = [np.array([alphabet.index(c) for c in doc] + [eof], dtype=np.int32) for doc in text]
    cdf = O.categorical_fast_cdf(probs, 24)
    model = B.Model.from_cdf(cdf, 0, 24)
    flat, offsets = B.ragged(docs)
    enc = B.range_encode_ragged(flat, offsets, model)
    torch.cuda.synchronize()
    assert enc.config == (32, 64, 24) and (enc.status.cpu().numpy() == 0).all()
    single = M.Categorical(probs, perfect=False)
    for s in (0, 1, 2, 3, 4, len(docs) - 1):
        coder = queue.RangeEncoder()
        coder.encode(docs[s], single)
        assert enc.stream(s).tolist() == coder.get_compressed().tolist()
        want, st = oracle_words(O, docs[s], 0, cdf, (32, 64, 24))
        assert st == 0 and enc.stream(s).tolist() == want.tolist()
    dec, off2, status = B.range_decode_until(enc, model, eof)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(off2, offsets) and torch.equal(dec, flat)
    out, off = dec.cpu().numpy(), offsets.cpu().numpy()
    assert ["".join(alphabet[i] for i in out[off[s]: off[s + 1] - 1]) for s in range(len(docs))] == text
    assert all(out[off[s + 1] - 1] == eof for s in range(len(docs)))
    # a limit below the longest documents: those report CAPACITY and decode to NOTHING, the others are unaffected
    dec3, off3, status3 = B.range_decode_until(enc, model, eof, max_symbols=100)
    lens, lens3 = np.diff(off), np.diff(off3.cpu().numpy())
    assert lens3.tolist() == np.where(lens > 100, 0, lens).tolist()
    assert status3.cpu().tolist() == [2 if n > 100 else 0 for n in lens]
    o3, f3 = dec3.cpu().numpy(), off3.cpu().numpy()
    assert all(o3[f3[s]: f3[s + 1]].tolist() == out[off[s]: off[s] + lens3[s]].tolist() for s in range(len(docs)))
    # no document has the terminator asked for: a range decoder never runs out of words, max_symbols stops every stream
    dec4, off4, status4 = B.range_decode_until(enc, model, eof + 5, max_symbols=1 << 12)
    assert dec4.numel() == 0 and int(off4[-1]) == 0 and (status4.cpu().numpy() == 2).all()


def _straddling_streams(cdf, P, lengths, seed, stay):
    """The generator of tests/test_gpu_range_batch.py for streams of given lengths: symbols chosen by following the encoder's interval
    (queue.rs:612-705 in Python integers) -- while the interval straddles a word boundary, the symbol whose bin contains the boundary
    is taken with probability `stay` (Inverted situations of many held-back words, queue.rs:126-142, far beyond what
    model-distributed data produces), another one otherwise (resolution with or without a carry).  Returns the streams and the
    longest run of held-back words in them."""
    rng = np.random.default_rng(seed)
    n = len(cdf) - 1
    top = 1 << 64
    out, longest = [], 0
    for n_per in lengths:
        row = np.zeros(int(n_per), dtype=np.int32)
        lower, rng_ = 0, top - 1
        held = 0
        for t in range(int(n_per)):
            scale = rng_ >> P
            pick = None
            if lower + rng_ >= top and rng.random() < stay:
                for i in range(n):
                    if lower + scale * int(cdf[i]) < top <= lower + scale * int(cdf[i + 1]):
                        pick = i
            if pick is None:
                pick = int(rng.integers(0, n))
            row[t] = pick
            lower = lower + scale * int(cdf[pick])
            rng_ = scale * int(cdf[pick + 1] - cdf[pick])
            if lower >= top:
                lower -= top
            if lower + rng_ < top:
                held = 0
            if rng_ < (1 << 32):
                lower = (lower << 32) % top
                rng_ <<= 32
                held = held + 1 if lower + rng_ >= top else 0
                longest = max(longest, held)
        out.append(row)
    return out, longest


@pytest.mark.parametrize("P", [12, 24])
def test_inverted_runs(B, O, P):
    """Carries that travel through many held-back words: 96 streams of 0 .. 640 symbols whose intervals keep straddling a word
    boundary.  Words of every stream equal the oracle's, decoding returns the input."""
    probs = np.array([1, 3, 1 << (P - 2), (1 << P) - 8 - (1 << (P - 2)), 2, 2], dtype=np.int64)
    cdf = np.concatenate([[0], np.cumsum(probs)]).astype(np.uint32)
    model = B.Model.from_cdf(cdf, 0, P)
    lengths = np.random.default_rng(P).integers(0, 641, 96)
    lengths[:8] = [0, 640, 1, 640, 7, 639, 8, 633]
    docs, longest = _straddling_streams(cdf, P, lengths, 5 + P, 0.995)
    assert longest >= 24          # (the fixture does what it is for: runs longer than a 64-byte group, and than most of a lane's ring)
    flat, offsets = B.ragged(docs)
    cfg = (32, 64, P)
    enc = B.range_encode_ragged(flat, offsets, model, cfg)
    check_all_streams(B, O, docs, enc, 0, cdf, cfg)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


def test_schedule_does_not_change_results(B, O):
    """Lane slot i codes stream order[i].  The identity, sorted by length, shuffled, reversed: the same counts and statuses, the
    oracle's words, the same decode under every decoder order; an entry that is no stream index idles its slot."""
    P, lo, cfg = 24, 0, (32, 64, 24)
    rng = np.random.default_rng(5)
    cdf = O.categorical_fast_cdf(rng.dirichlet(np.ones(50) * 0.5), P)
    model = B.Model.from_cdf(cdf, lo, P)
    lengths = np.exp(rng.uniform(np.log(1), np.log(1500), 700)).astype(np.int64)
    docs = [rng.integers(0, 50, int(n)).astype(np.int32) for n in lengths]
    flat, offsets = B.ragged(docs)
    ref = B.range_encode_ragged(flat, offsets, model, cfg, order=None)
    assert ref.order is None
    ref_n = check_all_streams(B, O, docs, ref, lo, cdf, cfg, every=9)
    ref_dec, ref_st = B.range_decode_ragged(ref, model, offsets, order=None)
    assert torch.equal(ref_dec, flat) and int(ref_st.abs().sum()) == 0
    perm = torch.from_numpy(rng.permutation(len(docs)).astype(np.int32)).cuda()
    reverse = torch.arange(len(docs) - 1, -1, -1, dtype=torch.int32, device="cuda")
    for order in ("sorted", perm, reverse):
        enc = B.range_encode_ragged(flat, offsets, model, cfg, order=order)
        torch.cuda.synchronize()
        assert enc.order is not None and sorted(enc.order.cpu().tolist()) == list(range(len(docs)))
        assert enc.n_words.cpu().tolist() == ref_n.tolist()
        check_all_streams(B, O, docs, enc, lo, cdf, cfg, every=9)
        for dec_order in ("auto", None, "sorted", perm, reverse):
            dec, st = B.range_decode_ragged(enc, model, offsets, order=dec_order)
            assert torch.equal(dec, flat) and int(st.abs().sum()) == 0
    # entries that are no stream indices: their slots idle -- prefilled words, counts and output keep their fill, the neighbours are coded
    bad = torch.arange(len(docs), dtype=torch.int32, device="cuda")
    bad[3] = -1
    bad[10] = len(docs)
    FILL = 0x5A5A5A5A
    woff = ref.word_offsets
    words = torch.full((int(woff[-1]),), FILL, dtype=torch.int32, device="cuda")
    n_words = torch.full((len(docs),), -5, dtype=torch.int32, device="cuda")
    status = torch.full((len(docs),), -5, dtype=torch.int32, device="cuda")
    from constriction_amd import _native as N
    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(N.lib().cst_range_encode_ragged(model._h, N.CoderConfig(*cfg), p(flat), p(offsets), len(docs), p(bad), p(words), p(woff), 0, p(n_words),
                                            p(status), None), "cst_range_encode_ragged")
    torch.cuda.synchronize()
    keep = np.ones(len(docs), bool); keep[[3, 10]] = False
    assert n_words.cpu().numpy()[keep].tolist() == ref_n[keep].tolist() and (status.cpu().numpy()[keep] == 0).all()
    assert n_words.cpu().numpy()[~keep].tolist() == [-5, -5] and status.cpu().numpy()[~keep].tolist() == [-5, -5]
    w, wo = words.cpu().numpy(), woff.cpu().numpy()
    for s in (3, 10):
        assert (w[wo[s]: wo[s + 1]] == FILL).all()
    for s in (2, 4, 9, 11):
        assert w[wo[s]: wo[s] + ref_n[s]].tolist() == ref.stream(s).view(np.int32).tolist()
    out = torch.full_like(flat, -7)
    dec, st = B.range_decode_ragged(ref, model, offsets, out=out, order=bad)
    off = offsets.cpu().numpy()
    assert (dec[off[3]: off[4]] == -7).all() and (dec[off[10]: off[11]] == -7).all()
    assert torch.equal(dec[off[11]:], flat[off[11]:]) and torch.equal(dec[: off[3]], flat[: off[3]]) and torch.equal(dec[off[4]: off[10]], flat[off[4]: off[10]])


def test_status_and_bounds(B, O):
    """an impossible symbol flags its stream only; corrupt counts / offsets are decoded as empty streams (INVALID_DATA) and nothing
    outside the buffer is read; backward slabs hold nothing; no streams at all is a no-op; the coders refuse each other's batches;
    and the argument checks of the C calls with a real model"""
    from constriction_amd import _native as N
    P, lo, cfg = 12, 0, (32, 64, 12)
    cdf = O.categorical_fast_cdf(np.ones(20) / 20, P)
    model = B.Model.from_cdf(cdf, lo, P)
    docs = [np.arange(n) % 20 for n in (5, 64, 0, 300, 17)]
    docs[3] = docs[3].copy(); docs[3][100] = 20
    flat, offsets = B.ragged(docs)
    enc = B.range_encode_ragged(flat, offsets, model, cfg)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [0, 0, 0, 1, 0] and enc.n_words.cpu().tolist()[3] == 0
    for s in (0, 1, 2, 4):
        want, _ = oracle_words(O, docs[s], lo, cdf, cfg)
        assert enc.stream(s).tolist() == want.tolist()
    good_docs = [d for k, d in enumerate(docs) if k != 3]
    good = B.ragged(good_docs)
    enc = B.range_encode_ragged(*good, model, cfg)
    ref, ref_st = B.range_decode_ragged(enc, model, good[1])
    assert ref_st.cpu().tolist() == [0, 0, 0, 0] and torch.equal(ref, good[0])
    enc.n_words[1] = 1 << 30                      # leaves the buffer
    enc.word_offsets[2] = 1 << 40
    dec, status = B.range_decode_ragged(enc, model, good[1])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 3, 3, 0]
    off = good[1].cpu().numpy()
    assert torch.equal(dec[off[3]: off[4]], ref[off[3]: off[4]]) and torch.equal(dec[: off[1]], ref[: off[1]])
    lengths, cstatus = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(N.lib().cst_range_count_until(model._h, N.CoderConfig(*cfg), p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), 4,
                                          None, 16, 50, p(lengths), p(cstatus), None), "cst_range_count_until")
    assert B.last_kernel() == "range_count_until_kernel"
    torch.cuda.synchronize()
    # stream 3 ends with its terminator (... 15, 16); stream 0 has none and is decoded on, past its words, as the reference does it
    # (zeros are shifted in): the oracle's decoder says where a 16 turns up among its first 50 symbols, if anywhere
    assert cstatus.cpu().tolist()[1:] == [3, 3, 0] and lengths.cpu().tolist()[3] == 17
    w0, _ = oracle_words(O, good_docs[0], lo, cdf, cfg)
    more, st = O.rc_decode_batch(w0[None, :], np.array([len(w0)], np.uint32), 50, lo, cdf, P)
    hits = np.flatnonzero(more[0] == 16)
    assert more[0, :5].tolist() == good_docs[0].tolist()
    assert (cstatus.cpu().tolist()[0], lengths.cpu().tolist()[0]) == ((0 if int(st[0]) == 0 else 3, int(hits[0]) + 1) if len(hits) else (2, 50))
    empty = B.range_encode_ragged(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), model, cfg)
    assert empty.n_words.numel() == 0 and empty.coder == "range"
    dec0, st0 = B.range_decode_ragged(empty, model, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert dec0.numel() == 0 and st0.numel() == 0
    # word offsets that run BACKWARDS: that stream gets a slab of no words -- CAPACITY, nothing written
    flat, offsets = good
    n = offsets.numel() - 1
    woff = torch.tensor([0, 64, 32, 512, 1024], dtype=torch.int64, device="cuda")      # stream 1: [64, 32)
    words = torch.full((2048,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    N.check(N.lib().cst_range_encode_ragged(model._h, N.CoderConfig(*cfg), p(flat), p(offsets), n, None, p(words), p(woff), 0, p(n_words), p(status),
                                            None), "cst_range_encode_ragged")
    torch.cuda.synchronize()
    st, nw = status.cpu().tolist(), n_words.cpu().tolist()
    assert st == [0, 2, 0, 0] and nw[1] == 0
    w = words.cpu().numpy().view(np.uint32)
    for s in (0, 3):
        want, _ = oracle_words(O, good_docs[s], lo, cdf, cfg)
        a = int(woff[s])
        assert w[a: a + nw[s]].tolist() == want.tolist()
    assert nw[2] == 0 and (w[nw[0]: 512] == 0x5A5A5A5A).all() and (w[512 + nw[3]:] == 0x5A5A5A5A).all()
    # the coders refuse each other's batches
    ans = B.ans_encode_ragged(*good, model, cfg, jump_every=0)
    rng_batch = B.range_encode_ragged(*good, model, cfg)
    with pytest.raises(ValueError):
        B.ans_decode_ragged(rng_batch, model, good[1])
    with pytest.raises(ValueError):
        B.ans_decode_until(rng_batch, model, 3)
    with pytest.raises(ValueError):
        B.range_decode_ragged(ans, model, good[1])
    with pytest.raises(ValueError):
        B.range_decode_until(ans, model, 3)
    # the C calls judge their arguments before they touch the device: HOST buffers behind the pointers of calls that must be refused
    bad = N.CST_ERR_INVALID_ARGUMENT
    host = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "lengths")}

    def call(name, c=cfg, null=(), stride=0, n_streams=1):
        q = {k: (None if k in null else C.c_void_p(v.ctypes.data)) for k, v in host.items()}
        L, cc = N.lib(), N.CoderConfig(*c)
        if name == "encode":
            return L.cst_range_encode_ragged(model._h, cc, q["symbols"], q["sym_offsets"], n_streams, q["order"], q["words"], q["word_offsets"],
                                             stride, q["n_words"], q["status"], None)
        if name == "decode":
            return L.cst_range_decode_ragged(model._h, cc, q["words"], q["word_offsets"], stride, 64, q["n_words"], q["symbols"], q["sym_offsets"],
                                             n_streams, q["order"], q["status"], None)
        return L.cst_range_count_until(model._h, cc, q["words"], q["word_offsets"], stride, 64, q["n_words"], n_streams, q["order"], 3, 100,
                                       q["lengths"], q["status"], None)

    required = {"encode": ("sym_offsets", "words", "n_words", "status"), "decode": ("sym_offsets", "n_words", "status"),
                "count": ("n_words", "lengths", "status")}
    for name in ("encode", "decode", "count"):
        for n_streams in (0, 1):
            for pointer in required[name]:
                assert call(name, null=(pointer,), n_streams=n_streams) == bad, (name, pointer)
            for c in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24), (32, 64, 24), (16, 32, 11)):
                assert call(name, c=c, n_streams=n_streams) == bad, (name, c)          # unsupported, or not the model's precision
            assert call(name, null=("word_offsets",), stride=0, n_streams=n_streams) == bad
        assert call(name, n_streams=1 << 32) == bad
        assert call(name, n_streams=0) == N.CST_OK and call(name, n_streams=0, null=("order",)) == N.CST_OK
        assert call(name, n_streams=0, null=("word_offsets",), stride=16) == N.CST_OK


def test_agrees_with_the_rectangular_call(B, O):
    """two GPU calls that must agree: 128 streams of equal length 96 through range_encode_ragged and through range_encode"""
    P, lo, cfg = 16, -5, (32, 64, 16)
    rng = np.random.default_rng(11)
    cdf = O.categorical_fast_cdf(rng.dirichlet(np.ones(300) * 0.3), P)
    model = B.Model.from_cdf(cdf, lo, P)
    sym = O.synth_symbols(3, 0, 128, 96, lo, cdf, P)
    flat = torch.from_numpy(sym.reshape(-1)).cuda()
    offsets = torch.arange(0, 129, dtype=torch.int64, device="cuda") * 96
    enc = B.range_encode_ragged(flat, offsets, model, cfg)
    rect = B.range_encode(torch.from_numpy(sym).cuda(), model, cfg)
    torch.cuda.synchronize()
    words, n_words, status = rect.to_numpy()
    assert (status == 0).all() and enc.n_words.cpu().tolist() == n_words.tolist() and int(enc.status.abs().sum()) == 0
    for s in range(128):
        assert enc.stream(s).tolist() == words[s, : n_words[s]].tolist(), f"stream {s}"
