"""GPU tests of jump points for ragged range batches (`cst_range_{encode,decode}_ragged_jump`): RangeEncoder::pos() in front of every
chunk of every document, and a decoder that runs every chunk as a coder of its own.  Every comparison is against the CPU oracle coding
that document ALONE (`O.rc_encode_batch`, `O.range_jump_table`, `O.range_decode_from`); no GPU result is the reference for another,
except where a test says "equals the plain call" (whose words tests/test_gpu_range_ragged.py pins to the oracle)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENC_KERNEL, DEC_KERNEL = "range_encode_ragged_kernel<jump>", "range_decode_ragged_kernel<jump>"


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
    W, S, P = cfg
    words, n, st = O.rc_encode_batch(np.asarray(doc, dtype=np.int32)[None, :], lo, cdf, P, W, S)
    return words[0, : n[0]], int(st[0])


def table_of(enc):
    """(chunk_offsets, pos, lower, range) of a batch on the host, unsigned"""
    j = enc.jump
    return (j.chunk_offsets.cpu().numpy(), j.pos.cpu().numpy().view(np.uint32), j.lower.cpu().numpy().view(np.uint64),
            j.range.cpu().numpy().view(np.uint64))


def assert_table_is_the_oracles(O, enc, docs, streams, lo, cdf, cfg, every):
    W, S, P = cfg
    co, pos, lower, rng = table_of(enc)
    for s in streams:
        if len(docs[s]) == 0:
            assert co[s] == co[s + 1]
            continue
        wp, wl, wr = O.range_jump_table(np.asarray(docs[s], np.int32)[None, :], lo, cdf, P, every, W, S)
        a, b = co[s], co[s + 1]
        assert b - a == wp.shape[1], f"stream {s}"
        assert pos[a:b].tolist() == wp[0].tolist(), f"pos of stream {s} ({len(docs[s])} symbols)"
        assert lower[a:b].tolist() == wl[0].tolist(), f"lower of stream {s} ({len(docs[s])} symbols)"
        assert rng[a:b].tolist() == wr[0].tolist(), f"range of stream {s} ({len(docs[s])} symbols)"


def assert_equals_the_plain_call(B, enc, plain, every, lengths, streams):
    assert plain.jump is None and plain.coder == "range"
    assert enc.coder == "range" and isinstance(enc.jump, B.RangeRaggedJump) and enc.jump.interval == every
    assert torch.equal(enc.n_words, plain.n_words) and torch.equal(enc.status, plain.status) and int(enc.status.abs().sum()) == 0
    assert torch.equal(enc.word_offsets, plain.word_offsets)
    for s in streams:
        assert enc.stream(s).tolist() == plain.stream(s).tolist(), f"stream {s}"
    co = enc.jump.chunk_offsets.cpu().numpy()
    assert co.tolist() == np.concatenate([[0], np.cumsum((np.asarray(lengths) + every - 1) // every)]).tolist()


@pytest.mark.parametrize("cfg", [(32, 64, 24), (32, 64, 12), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("every", [8, 64, 256, 1024])
def test_parity(B, O, cfg, every):
    """The document mix of test_ragged_jump_points (tests/test_gpu_ragged.py): empty documents, documents shorter than a chunk, lengths
    that are multiples of nothing.  Counts, statuses and words equal the plain call; the table is the oracle's for each document alone;
    the chunk decoder returns the documents, and so does the whole-stream decoder on the same batch; the oracle's RangeDecoder::seek
    reads the DEVICE's words from the device's jump points.
    (The whole-stream decode of the same batch is asked for with an explicit schedule: `order=None` means "no schedule", and a batch
    with jump points then decodes its chunks, as ans_decode_ragged has it.)"""
    W, S, P = cfg
    rng = np.random.default_rng(P + every)
    n_sym, lo = 90, -17
    cdf = O.categorical_fast_cdf(rng.dirichlet(np.ones(n_sym) * 0.4), P)
    model = B.Model.from_cdf(cdf, lo, P)
    lengths = np.concatenate([rng.integers(0, 200, 400), rng.integers(200, 3000, 60), [0, 1, 7, 8, 9, every - 1, every, every + 1, 2 * every, 2047]])
    rng.shuffle(lengths)
    docs = [O.synth_symbols(int(k), 0, 1, int(n), lo, cdf, P)[0] if n else np.zeros(0, np.int32) for k, n in enumerate(lengths)]
    flat, offsets = B.ragged(docs)
    plain = B.range_encode_ragged(flat, offsets, model, cfg)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    assert B.last_kernel() == ENC_KERNEL
    torch.cuda.synchronize()
    assert_equals_the_plain_call(B, enc, plain, every, lengths, range(0, len(docs), 5))
    longest = int(np.argmax(lengths))
    assert_table_is_the_oracles(O, enc, docs, list(range(0, len(docs), 9)) + [longest], lo, cdf, cfg, every)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == DEC_KERNEL
    assert int(status.abs().sum()) == 0 and torch.equal(dec, flat)
    dec2, status2 = B.range_decode_ragged(enc, model, offsets, order=None)
    assert B.last_kernel() == DEC_KERNEL                       # (no schedule asked for: the chunks)
    whole = torch.arange(len(docs), dtype=torch.int32, device="cuda")
    dec3, status3 = B.range_decode_ragged(enc, model, offsets, order=whole)
    assert B.last_kernel() == "range_decode_ragged_kernel"     # a schedule is honoured on whole streams
    assert torch.equal(dec2, flat) and torch.equal(dec3, flat) and int(status2.abs().sum()) == 0 and int(status3.abs().sum()) == 0
    # jump_every = 0 is exactly the plain call
    none = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=0)
    assert B.last_kernel() == "range_encode_ragged_kernel" and none.jump is None and torch.equal(none.n_words, plain.n_words)
    # the oracle's seek on the device's words, from the device's jump points: first, middle and last chunk of the longest document
    co, pos, lower, rg = table_of(enc)
    words, doc = enc.stream(longest), docs[longest]
    n_chunks = int(co[longest + 1] - co[longest])
    for j in sorted({0, n_chunks // 2, n_chunks - 1}):
        c = int(co[longest]) + j
        n = min(every, len(doc) - j * every)
        back, st = O.range_decode_from(words, pos[c], lower[c], rg[c], n, lo, cdf, P, W, S)
        assert int(st) == 0 and back.tolist() == doc[j * every: j * every + n].tolist(), f"chunk {j}"


def _straddling_streams(cdf, P, lengths, seed, stay):
    """The generator of tests/test_gpu_range_ragged.py: symbols chosen by following the encoder's interval (queue.rs:612-705 in Python
    integers) -- while the interval straddles a word boundary, the symbol whose bin contains the boundary is taken with probability
    `stay` (Inverted situations of many held-back words), another one otherwise."""
    rng = np.random.default_rng(seed)
    n = len(cdf) - 1
    top = 1 << 64
    out = []
    for n_per in lengths:
        row = np.zeros(int(n_per), dtype=np.int32)
        lower, rng_ = 0, top - 1
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
            if rng_ < (1 << 32):
                lower = (lower << 32) % top
                rng_ <<= 32
        out.append(row)
    return out


@pytest.fixture(scope="module", params=[12, 24], ids=lambda P: "P%d" % P)
def straddling(request, O):
    """the 96 streams and the table of test_inverted_runs (tests/test_gpu_range_ragged.py), made once per precision"""
    P = request.param
    probs = np.array([1, 3, 1 << (P - 2), (1 << P) - 8 - (1 << (P - 2)), 2, 2], dtype=np.int64)
    cdf = np.concatenate([[0], np.cumsum(probs)]).astype(np.uint32)
    lengths = np.random.default_rng(P).integers(0, 641, 96)
    lengths[:8] = [0, 640, 1, 640, 7, 639, 8, 633]
    return P, cdf, lengths, _straddling_streams(cdf, P, lengths, 5 + P, 0.995)


@pytest.mark.parametrize("every", [8, 64])
def test_jump_points_inside_inverted_runs(B, O, straddling, every):
    """Jump points that fall INSIDE runs of held-back words: there `pos` counts words that are not written yet, and lower + range
    wraps.  The fixture is judged by the oracle's table alone (at least 100 such points, every chunk decodable from its point by the
    oracle's seek); then ALL streams' tables and words against the oracle, and the decode."""
    P, cdf, lengths, docs = straddling
    cfg = (32, 64, P)
    inverted = 0
    for doc in docs:
        if len(doc) == 0:
            continue
        wp, wl, wr = O.range_jump_table(doc[None, :], 0, cdf, P, every)
        inverted += sum(1 for lo_, r_ in zip(wl[0].tolist(), wr[0].tolist()) if lo_ + r_ >= 1 << 64)
        want, st = oracle_words(O, doc, 0, cdf, cfg)
        assert st == 0
        for j in range(wp.shape[1]):
            n = min(every, len(doc) - j * every)
            back, st = O.range_decode_from(want, wp[0, j], wl[0, j], wr[0, j], n, 0, cdf, P)
            assert int(st) == 0 and back.tolist() == doc[j * every: j * every + n].tolist()
    print(f"P = {P}, every = {every}: {inverted} jump points inside Inverted runs")
    assert inverted >= 100
    model = B.Model.from_cdf(cdf, 0, P)
    flat, offsets = B.ragged(docs)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    assert B.last_kernel() == ENC_KERNEL
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    for s, doc in enumerate(docs):
        want, _ = oracle_words(O, doc, 0, cdf, cfg)
        assert enc.stream(s).tolist() == want.tolist(), f"stream {s} of {len(doc)} symbols"
    assert_table_is_the_oracles(O, enc, docs, range(len(docs)), 0, cdf, cfg, every)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == DEC_KERNEL
    assert int(status.abs().sum()) == 0 and torch.equal(dec, flat)


@pytest.mark.parametrize("cfg,n_sym", [((32, 64, 6), 40), ((16, 32, 5), 20), ((32, 64, 16), 5000), ((32, 64, 20), 20000), ((16, 32, 16), 5000),
                                       ((32, 64, 22), 1000), ((32, 64, 24), 256)],
                         ids=lambda v: "W%dS%dP%d" % v if isinstance(v, tuple) else "n%d" % v)
def test_kernel_variants(B, O, cfg, n_sym):
    """The (preset, alphabet) pairs and the 190 lengths of test_kernel_variants (tests/test_gpu_range_ragged.py): tables in LDS and in
    HBM, 16-bit words, P < 8.  Words and counts equal the plain call, the table of every tenth stream is the oracle's, decode returns
    the input."""
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
    docs = [(lo + rng.choice(n_sym, size=int(n), p=p / p.sum())).astype(np.int32) for n in lengths]
    flat, offsets = B.ragged(docs)
    plain = B.range_encode_ragged(flat, offsets, model, cfg)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=64)
    assert B.last_kernel() == ENC_KERNEL
    torch.cuda.synchronize()
    assert_equals_the_plain_call(B, enc, plain, 64, lengths, range(len(docs)))
    assert_table_is_the_oracles(O, enc, docs, range(0, len(docs), 10), lo, cdf, cfg, 64)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == DEC_KERNEL
    assert int(status.abs().sum()) == 0 and torch.equal(dec, flat)


@pytest.fixture(scope="module")
def small(B, O):
    """a 40-symbol table at P = 12 and 257 documents of 300 .. 899 symbols (chunk totals that are no multiples of 64)"""
    P, lo = 12, 0
    cdf = O.categorical_fast_cdf(np.ones(40) / 40, P)
    lengths = np.random.default_rng(3).integers(300, 900, 257)
    docs = [O.synth_symbols(int(k), 0, 1, int(n), lo, cdf, P)[0] for k, n in enumerate(lengths)]
    return P, lo, cdf, B.Model.from_cdf(cdf, lo, P), lengths, docs


@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 257])
def test_shapes_of_the_launch(B, O, small, n_streams):
    """partial last waves in both passes: the encoder's lanes are streams, the decoder's are chunks"""
    P, lo, cdf, model, lengths, docs = small
    cfg, every = (32, 64, P), 64
    docs, lengths = docs[:n_streams], lengths[:n_streams]
    total = int(((lengths + every - 1) // every).sum())
    assert total % 64 != 0
    flat, offsets = B.ragged(docs)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert int(enc.jump.chunk_offsets[-1]) == total and int(enc.status.abs().sum()) == 0
    for s in range(0, n_streams, 7):
        want, _ = oracle_words(O, docs[s], lo, cdf, cfg)
        assert enc.stream(s).tolist() == want.tolist()
    assert_table_is_the_oracles(O, enc, docs, range(0, n_streams, 7), lo, cdf, cfg, every)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == DEC_KERNEL
    assert int(status.abs().sum()) == 0 and torch.equal(dec, flat)


def test_no_streams_and_empty_streams(B, O, small):
    P, lo, cdf, model, _, _ = small
    cfg = (32, 64, P)
    none = B.range_encode_ragged_jump(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), model, cfg,
                                      jump_every=64)
    assert none.n_words.numel() == 0 and none.coder == "range" and none.jump is None
    dec, st = B.range_decode_ragged(none, model, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert dec.numel() == 0 and st.numel() == 0
    offsets = torch.zeros(71, dtype=torch.int64, device="cuda")
    empty = B.range_encode_ragged_jump(torch.zeros(0, dtype=torch.int32, device="cuda"), offsets, model, cfg, jump_every=64)
    assert B.last_kernel() == ENC_KERNEL
    torch.cuda.synchronize()
    assert empty.jump is not None and empty.jump.chunk_offsets.cpu().tolist() == [0] * 71
    assert empty.n_words.cpu().tolist() == [0] * 70 and empty.status.cpu().tolist() == [0] * 70
    dec, st = B.range_decode_ragged(empty, model, offsets)
    assert B.last_kernel() == DEC_KERNEL
    assert dec.numel() == 0 and st.cpu().tolist() == [0] * 70


def test_auto_notes_jump_points_for_long_documents_only(B, O, small):
    """jump_every="auto": a point every RAGGED_JUMP_EVERY symbols if the documents average more than that (more than one chunk each),
    none otherwise -- then the batch is the plain call's"""
    P, lo, cdf, model, lengths, docs = small
    cfg = (32, 64, P)
    long_docs = docs[:40]                                       # 300 .. 899 symbols each
    flat, offsets = B.ragged(long_docs)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg)
    assert B.last_kernel() == ENC_KERNEL and enc.jump is not None and enc.jump.interval == B.RAGGED_JUMP_EVERY == 256
    assert_table_is_the_oracles(O, enc, long_docs, range(0, 40, 3), lo, cdf, cfg, 256)
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == DEC_KERNEL and int(status.abs().sum()) == 0 and torch.equal(dec, flat)
    short_docs = [d[:200] for d in docs[:40]]                   # one chunk each: a table would buy nothing
    flat, offsets = B.ragged(short_docs)
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg)
    assert B.last_kernel() == "range_encode_ragged_kernel" and enc.jump is None
    dec, status = B.range_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == "range_decode_ragged_kernel" and int(status.abs().sum()) == 0 and torch.equal(dec, flat)


def test_schedule_does_not_change_results(B, O, small):
    """order="sorted" and a random permutation on the encoder: the identity order's table, words and decode"""
    P, lo, cdf, model, lengths, docs = small
    cfg, every = (32, 64, P), 64
    docs = docs[:150] + [np.zeros(0, np.int32), docs[150][:5]]
    flat, offsets = B.ragged(docs)
    ref = B.range_encode_ragged_jump(flat, offsets, model, cfg, order=None, jump_every=every)
    torch.cuda.synchronize()
    assert ref.order is None
    assert_table_is_the_oracles(O, ref, docs, range(0, len(docs), 9), lo, cdf, cfg, every)
    n_chunks = int(ref.jump.chunk_offsets[-1])
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(docs)).astype(np.int32)).cuda()
    for order in ("sorted", perm):
        enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, order=order, jump_every=every)
        assert B.last_kernel() == ENC_KERNEL
        torch.cuda.synchronize()
        assert enc.order is not None and sorted(enc.order.cpu().tolist()) == list(range(len(docs)))
        assert torch.equal(enc.n_words, ref.n_words) and torch.equal(enc.status, ref.status)
        assert torch.equal(enc.jump.chunk_offsets, ref.jump.chunk_offsets)
        for name in ("pos", "lower", "range"):
            assert torch.equal(getattr(enc.jump, name)[:n_chunks], getattr(ref.jump, name)[:n_chunks]), name
        for s in range(len(docs)):
            assert enc.stream(s).tolist() == ref.stream(s).tolist()
        dec, status = B.range_decode_ragged(enc, model, offsets)
        assert B.last_kernel() == DEC_KERNEL
        assert int(status.abs().sum()) == 0 and torch.equal(dec, flat)


def test_c_abi_with_slabs(B, O, small):
    """the C calls directly: slabs `stride_words` apart (d_word_offsets = NULL) on both sides, words_capacity exactly the buffer's size,
    n_chunks_total an upper bound of the chunks"""
    from constriction_amd import _native as N
    P, lo, cdf, model, lengths, docs = small
    cfg, every, n = (32, 64, P), 64, 70
    docs = docs[:n]
    flat, offsets = B.ragged(docs)
    off = offsets.cpu().numpy()
    stride = (max(len(d) for d in docs) * P + 31) // 32 + 2
    co = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    co[1:] = torch.cumsum((offsets[1:] - offsets[:-1] + every - 1) // every, 0)
    total, bound = int(co[-1]), int(co[-1]) + 37
    FILL = 0x5A5A5A5A
    words = torch.full((n * stride,), FILL, dtype=torch.int32, device="cuda")
    n_words, status = torch.full((n,), -5, dtype=torch.int32, device="cuda"), torch.full((n,), -5, dtype=torch.int32, device="cuda")
    pos = torch.full((bound,), -1, dtype=torch.int32, device="cuda")
    lower, rng = torch.full((bound,), -1, dtype=torch.int64, device="cuda"), torch.full((bound,), -1, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    L, cc = N.lib(), N.CoderConfig(*cfg)
    N.check(L.cst_range_encode_ragged_jump(model._h, cc, p(flat), p(offsets), n, None, p(words), None, stride, p(n_words), every, p(co), p(pos),
                                           p(lower), p(rng), p(status), None), "cst_range_encode_ragged_jump")
    assert B.last_kernel() == ENC_KERNEL
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    w, nw = words.cpu().numpy().view(np.uint32), n_words.cpu().numpy()
    for s in range(n):
        want, _ = oracle_words(O, docs[s], lo, cdf, cfg)
        assert w[s * stride: s * stride + nw[s]].tolist() == want.tolist()
        assert (w[s * stride + nw[s]: (s + 1) * stride] == FILL).all()
    # entries behind the last chunk are not written
    assert (pos[total:] == -1).all() and (lower[total:] == -1).all() and (rng[total:] == -1).all()
    hp, hl, hr = pos.cpu().numpy().view(np.uint32), lower.cpu().numpy().view(np.uint64), rng.cpu().numpy().view(np.uint64)
    hco = co.cpu().numpy()
    for s in range(0, n, 3):
        wp, wl, wr = O.range_jump_table(docs[s][None, :], lo, cdf, P, every)
        a, b = hco[s], hco[s + 1]
        assert (hp[a:b].tolist(), hl[a:b].tolist(), hr[a:b].tolist()) == (wp[0].tolist(), wl[0].tolist(), wr[0].tolist())
    # decode: the slabs, the buffer's exact size as words_capacity, `bound` > total table entries
    scratch = torch.empty(L.cst_range_ragged_jump_scratch_bytes(bound), dtype=torch.uint8, device="cuda")
    out = torch.full((flat.numel() + 4096,), 77, dtype=torch.int32, device="cuda")
    dstatus = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    N.check(L.cst_range_decode_ragged_jump(model._h, cc, p(words), None, stride, words.numel(), p(n_words), p(out), p(offsets), n, every, p(co),
                                           bound, p(pos), p(lower), p(rng), p(scratch), p(dstatus), None), "cst_range_decode_ragged_jump")
    assert B.last_kernel() == DEC_KERNEL
    torch.cuda.synchronize()
    assert dstatus.cpu().tolist() == [0] * n and torch.equal(out[: flat.numel()], flat) and bool((out[flat.numel():] == 77).all())
    # ... and a count larger than its slab flags that stream alone
    n_words[4] = stride + 1
    out.fill_(77)
    N.check(L.cst_range_decode_ragged_jump(model._h, cc, p(words), None, stride, words.numel(), p(n_words), p(out), p(offsets), n, every, p(co),
                                           bound, p(pos), p(lower), p(rng), p(scratch), p(dstatus), None), "cst_range_decode_ragged_jump")
    torch.cuda.synchronize()
    assert dstatus.cpu().tolist() == [3 if s == 4 else 0 for s in range(n)]
    assert torch.equal(out[: off[4]], flat[: off[4]]) and torch.equal(out[off[5]: flat.numel()], flat[off[5]:])
    assert bool((out[flat.numel():] == 77).all())
    # the refusals with a real model (HOST buffers behind the pointers of calls that must be refused)
    bad = N.CST_ERR_INVALID_ARGUMENT
    host = np.zeros(64, dtype=np.float64)
    h = C.c_void_p(host.ctypes.data)
    for n_streams in (0, 1):
        for interval in (0, 12, 1 << 31):
            assert L.cst_range_encode_ragged_jump(model._h, cc, h, h, n_streams, None, h, h, 0, h, interval, h, h, h, h, h, None) == bad
            assert L.cst_range_decode_ragged_jump(model._h, cc, h, h, 0, 64, h, h, h, n_streams, interval, h, 8, h, h, h, h, h, None) == bad
        assert L.cst_range_decode_ragged_jump(model._h, cc, h, h, 0, 64, h, h, h, n_streams, 64, h, 1 << 32, h, h, h, h, h, None) == bad
        assert L.cst_range_decode_ragged_jump(model._h, cc, h, h, 0, 64, h, h, h, n_streams, 64, h, 8, h, h, h, None, h, None) == bad
        assert L.cst_range_encode_ragged_jump(model._h, cc, h, h, n_streams, None, h, h, 0, h, 64, h, h, None, h, h, None) == bad
        assert L.cst_range_encode_ragged_jump(model._h, cc, h, h, n_streams, None, h, None, 0, h, 64, h, h, h, h, h, None) == bad
        assert L.cst_range_encode_ragged_jump(model._h, N.CoderConfig(32, 64, 24), h, h, n_streams, None, h, h, 0, h, 64, h, h, h, h, h, None) == bad
    assert L.cst_range_encode_ragged_jump(model._h, cc, h, h, 0, None, h, h, 0, h, 64, h, h, h, h, h, None) == N.CST_OK
    assert L.cst_range_decode_ragged_jump(model._h, cc, h, h, 0, 64, h, h, h, 0, 64, h, 8, h, h, h, h, h, None) == N.CST_OK


def test_tables_are_checked(B, O, small):
    """a jump point beyond its stream's words, a table that does not describe its streams: INVALID_DATA for that stream, the others
    decode; no access outside the buffers (guarded output); the coders refuse each other's batches"""
    P, lo, cdf, model, lengths, docs = small
    cfg, every = (32, 64, P), 64
    docs = docs[:200]
    flat, offsets = B.ragged(docs)
    off = offsets.cpu().numpy()
    enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    co = enc.jump.chunk_offsets.cpu().numpy()
    enc.jump.pos[int(co[17]) + 2] = 1 << 30                       # a jump point beyond everything
    guard = torch.full((flat.numel() + 4096,), 77, dtype=torch.int32, device="cuda")
    dec, status = B.range_decode_ragged(enc, model, offsets, out=guard[: flat.numel()])
    assert B.last_kernel() == DEC_KERNEL
    st = status.cpu().numpy()
    assert st[17] == 3 and st.sum() == 3
    assert bool((guard[flat.numel():] == 77).all())
    ok = np.ones(flat.numel(), bool); ok[off[17]: off[18]] = False
    assert torch.equal(dec[torch.from_numpy(ok).cuda()], flat[torch.from_numpy(ok).cuda()])
    # a table made for other lengths: one chunk too few for stream 5 -- it alone is flagged, and the streams behind it, whose chunks
    # are still theirs by the offsets, decode from jump points that are not theirs: whatever they report, nothing outside is touched
    enc2 = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    shifted = enc2.jump.chunk_offsets.clone(); shifted[6:] -= 1
    enc2.jump.chunk_offsets = shifted
    guard.fill_(77)
    dec, status = B.range_decode_ragged(enc2, model, offsets, out=guard[: flat.numel()])
    assert B.last_kernel() == DEC_KERNEL
    st = status.cpu().numpy()
    assert st[5] == 3 and (st[:5] == 0).all() and torch.equal(dec[: off[5]], flat[: off[5]])
    assert bool((guard[flat.numel():] == 77).all())
    # offsets beyond the table: the two streams that touch them are flagged, the streams in front decode, nothing outside is touched
    enc3 = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    wild = enc3.jump.chunk_offsets.clone(); wild[150] = 1 << 40
    enc3.jump.chunk_offsets = wild
    guard.fill_(77)
    dec, status = B.range_decode_ragged(enc3, model, offsets, out=guard[: flat.numel()])
    st = status.cpu().numpy()
    assert st[149] == 3 and st[150] == 3 and (st[:149] == 0).all()
    assert torch.equal(dec[: off[149]], flat[: off[149]]) and bool((guard[flat.numel():] == 77).all())
    # offsets that run backwards (such a table is no longer sorted: which other streams still find their chunks is unspecified)
    wild = enc3.jump.chunk_offsets.clone(); wild[100] = 0
    enc3.jump.chunk_offsets = wild
    guard.fill_(77)
    dec, status = B.range_decode_ragged(enc3, model, offsets, out=guard[: flat.numel()])
    st = status.cpu().numpy()
    assert st[99] == 3 and st[100] == 3 and set(st.tolist()) <= {0, 3} and bool((guard[flat.numel():] == 77).all())
    # the coders refuse each other's batches, with or without jump points
    ans = B.ans_encode_ragged(flat, offsets, model, cfg, jump_every=every)
    fresh = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    assert ans.jump is not None and fresh.jump is not None
    with pytest.raises(ValueError):
        B.range_decode_ragged(ans, model, offsets)
    with pytest.raises(ValueError):
        B.ans_decode_ragged(fresh, model, offsets)
