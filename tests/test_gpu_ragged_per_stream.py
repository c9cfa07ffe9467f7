"""GPU tests of ragged batches coded with ONE TABLE PER STREAM (cst_ragged_ps.hip): the ragged entry points of both coders, plain and with
jump points, given a per-stream model.  Every expectation comes from the CPU oracle coding document s ALONE under cdfs[s]
(tests/ragged_per_stream_rows.py); no GPU result is the reference for another, except where a test says "equals the plain call" (whose
words the parity tests pin to the oracle)."""
import ctypes as C

import numpy as np
import pytest

import ragged_per_stream_rows as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KERNELS = {"ans": ("ans_encode_ragged_ps_kernel", "ans_decode_ragged_ps_kernel"),
           "range": ("range_encode_ragged_ps_kernel", "range_decode_ragged_ps_kernel")}
SHARED_KERNELS = {"ans": ("ans_encode_ragged_kernel", "ans_decode_ragged_kernel"),
                  "range": ("range_encode_ragged_kernel", "range_decode_ragged_kernel")}
CODERS = ["ans", "range"]
FILL = 0x5A5A5A5A


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


def p(t):
    return C.c_void_p(t.data_ptr())


def model_of(B, cdfs, lo, P):
    return B.Model.from_cdf_rows_per_stream(np.array(cdfs, dtype=np.uint32), lo, P)


def encode(B, coder, flat, offsets, model, cfg, order="auto", every=0):
    if coder == "ans":
        return B.ans_encode_ragged(flat, offsets, model, cfg, order, jump_every=every)
    if every:
        return B.range_encode_ragged_jump(flat, offsets, model, cfg, order, jump_every=every)
    return B.range_encode_ragged(flat, offsets, model, cfg, order)


def decode(B, coder, enc, model, offsets, order="auto"):
    return (B.ans_decode_ragged if coder == "ans" else B.range_decode_ragged)(enc, model, offsets, order=order)


def host(enc):
    return (enc.words.cpu().numpy().view(np.uint32), enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy(), enc.status.cpu().numpy())


def assert_streams_are_the_oracles(enc, want):
    w, wo, n, st = host(enc)
    assert st.tolist() == [0] * len(want)
    assert n.tolist() == [len(x) for x in want]
    for s, x in enumerate(want):
        assert w[wo[s]: wo[s] + n[s]].tolist() == x.tolist(), f"stream {s}"


def table_of(coder, enc):
    """(chunk_offsets, [pos, state] resp. [pos, lower, range]) of a batch on the host, unsigned"""
    j = enc.jump
    rest = [j.state] if coder == "ans" else [j.lower, j.range]
    return j.chunk_offsets.cpu().numpy(), [j.pos.cpu().numpy().view(np.uint32)] + [x.cpu().numpy().view(np.uint64) for x in rest]


def parity(B, coder, case, n_streams, W, S):
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (W, S, P)
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    enc = encode(B, coder, flat, offsets, model, cfg)
    assert B.last_kernel() == KERNELS[coder][0]
    assert enc.jump is None                     # "auto" notes no jump points under tables per stream
    torch.cuda.synchronize()
    assert_streams_are_the_oracles(enc, R.oracle_words(coder, case, n_streams, W, S))
    dec, status = decode(B, coder, enc, model, offsets)
    assert B.last_kernel() == KERNELS[coder][1]
    assert status.cpu().tolist() == [0] * n_streams and torch.equal(dec, flat)


@pytest.mark.parametrize("coder", CODERS)
def test_parity(B, coder):
    """Words, counts and statuses of every stream are the oracle's for that stream alone under its own row; the decode returns the input.
    Every family of R.PARITY_CASES at every batch size of R.STREAM_COUNTS under (32, 64), the families of R.W16_CASES under (16, 32) too
    (one test per coder, the batches in a loop: about fifty launches of a few thousand symbols each)."""
    for case in R.PARITY_CASES:
        for W, S in [(32, 64)] + ([(16, 32)] if case in R.W16_CASES else []):
            for n_streams in R.STREAM_COUNTS:
                try:
                    parity(B, coder, case, n_streams, W, S)
                except AssertionError as e:
                    raise AssertionError(f"{coder}, {case}, {n_streams} streams, ({W}, {S}): {e}") from e


def check_jump_batch(B, coder, docs, cdfs, lo, cfg, every, streams):
    """tables == the oracle's, words == the plain call's, decode through the table == input, and a chunk decoded ALONE by the oracle from
    the device's entry on the device's words is that chunk"""
    W, S, P = cfg
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    plain = encode(B, coder, flat, offsets, model, cfg)
    enc = encode(B, coder, flat, offsets, model, cfg, every=every)
    assert B.last_kernel() == KERNELS[coder][0] + "<jump>"
    torch.cuda.synchronize()
    assert plain.jump is None and enc.jump is not None and enc.jump.interval == every
    pw, pwo, pn, pst = host(plain)
    w, wo, n, st = host(enc)
    assert st.tolist() == [0] * len(docs) and pst.tolist() == st.tolist() and pn.tolist() == n.tolist() and pwo.tolist() == wo.tolist()
    for s in range(len(docs)):
        assert w[wo[s]: wo[s] + n[s]].tolist() == pw[wo[s]: wo[s] + n[s]].tolist(), f"stream {s}"
    co, table = table_of(coder, enc)
    lengths = np.array([len(d) for d in docs])
    assert co.tolist() == np.concatenate([[0], np.cumsum((lengths + every - 1) // every)]).tolist()
    for s in streams:
        if len(docs[s]) == 0:
            continue
        want = R.oracle_jump_table(coder, docs[s], lo, cdfs[s], P, every, W, S)
        for got, exp, what in zip(table, want, ("pos", "state / lower", "range")):
            assert got[co[s]: co[s + 1]].tolist() == exp.tolist(), f"{what} of stream {s} ({len(docs[s])} symbols)"
    dec, status = decode(B, coder, enc, model, offsets)
    assert B.last_kernel() == KERNELS[coder][1] + "<jump>"
    assert status.cpu().tolist() == [0] * len(docs) and torch.equal(dec, flat)
    whole = torch.arange(len(docs), dtype=torch.int32, device="cuda")
    dec2, status2 = decode(B, coder, enc, model, offsets, order=whole)       # a schedule is honoured on whole streams
    assert B.last_kernel() == KERNELS[coder][1]
    assert status2.cpu().tolist() == [0] * len(docs) and torch.equal(dec2, flat)
    longest = int(np.argmax(lengths))
    doc, words = docs[longest], w[wo[longest]: wo[longest] + n[longest]]
    n_chunks = int(co[longest + 1] - co[longest])
    for j in sorted({0, n_chunks // 2, n_chunks - 1}):
        c = int(co[longest]) + j
        k = min(every, len(doc) - j * every)
        back, bst = R.oracle_decode_chunk(coder, words, [t[c] for t in table], k, lo, cdfs[longest], P, W, S)
        assert bst == 0 and back.tolist() == doc[j * every: j * every + k].tolist(), f"chunk {j}"
    return enc, model, flat, offsets


@pytest.mark.parametrize("coder", CODERS)
def test_jump_points(B, coder):
    """a jump point every 8, 64 and 256 symbols on three batches (a (16, 32) one and one below the bucket index among them): see
    check_jump_batch"""
    for case, n_streams, preset in [("bimodal", 130, (32, 64)), ("p16_n300", 65, (16, 32)), ("p5", 65, (32, 64))]:
        lo, P, cdfs, docs, _ = R.batch(case, n_streams)
        for every in (8, 64, 256):
            try:
                check_jump_batch(B, coder, docs, cdfs, lo, preset + (P,), every, range(n_streams))
            except AssertionError as e:
                raise AssertionError(f"{coder}, {case}, {n_streams} streams, {preset}, every {every}: {e}") from e


def test_jump_points_inside_inverted_runs(B, O):
    """The straddling construction of tests/test_gpu_range_ragged_jump.py, every stream with its own copy of the row: jump points that
    fall INSIDE runs of held-back words, where `pos` counts words that are not written yet and lower + range wraps.  The fixture is
    judged by the oracle's table alone (at least 100 such points at either interval)."""
    from test_gpu_range_ragged_jump import _straddling_streams
    P = 12
    probs = np.array([1, 3, 1 << (P - 2), (1 << P) - 8 - (1 << (P - 2)), 2, 2], dtype=np.int64)
    cdf = np.concatenate([[0], np.cumsum(probs)]).astype(np.uint32)
    lengths = np.random.default_rng(P).integers(0, 641, 96)
    lengths[:8] = [0, 640, 1, 640, 7, 639, 8, 633]
    docs = _straddling_streams(cdf, P, lengths, 5 + P, 0.995)
    cdfs = np.tile(cdf, (len(docs), 1))
    for every in (8, 64):
        inverted = 0
        for doc in docs:
            if len(doc):
                _, wl, wr = O.range_jump_table(doc[None, :], 0, cdf, P, every)
                inverted += sum(1 for lo_, r_ in zip(wl[0].tolist(), wr[0].tolist()) if lo_ + r_ >= 1 << 64)
        print(f"every = {every}: {inverted} jump points inside Inverted runs")
        assert inverted >= 100, f"every {every}"
        enc, _, _, _ = check_jump_batch(B, "range", docs, cdfs, 0, (32, 64, P), every, range(len(docs)))
        w, wo, n, _ = host(enc)
        for s, doc in enumerate(docs):
            want, st = R.oracle_range_words(doc, 0, cdf, P)
            assert st == 0 and w[wo[s]: wo[s] + n[s]].tolist() == want.tolist(), f"every {every}: stream {s} of {len(doc)} symbols"


def test_schedule_does_not_change_results(B):
    """order=None, a reversed permutation and "auto": identical words and symbols (a lane's row is that of the stream its slot names)"""
    for coder in CODERS:
        schedule_does_not_change_results(B, coder)


def schedule_does_not_change_results(B, coder):
    case, n_streams = "skewed_fitted", 130
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (32, 64, P)
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    want = R.oracle_words(coder, case, n_streams)
    reverse = torch.arange(n_streams - 1, -1, -1, dtype=torch.int32, device="cuda")
    for order in (None, reverse, "auto"):
        enc = encode(B, coder, flat, offsets, model, cfg, order=order)
        torch.cuda.synchronize()
        assert_streams_are_the_oracles(enc, want)
        for dec_order in (None, reverse, "auto"):
            dec, status = decode(B, coder, enc, model, offsets, order=dec_order)
            assert B.last_kernel() == KERNELS[coder][1]
            assert status.cpu().tolist() == [0] * n_streams and torch.equal(dec, flat)
    # an entry that is no stream index idles its slot: that stream is not coded, its neighbours are
    bad = torch.arange(n_streams, dtype=torch.int32, device="cuda")
    bad[3] = -1
    bad[70] = n_streams
    enc = encode(B, coder, flat, offsets, model, cfg, order=bad)
    torch.cuda.synchronize()
    w, wo, n, st = host(enc)
    for s in (2, 4, 69, 71):
        assert st[s] == 0 and w[wo[s]: wo[s] + n[s]].tolist() == want[s].tolist()


def test_fit_encode_decode_end_to_end(B):
    """Model.fit_per_stream on the ragged batch itself -> ans_encode_ragged -> ans_decode_ragged.  An empty stream takes the uniform row
    and yields what the oracle's coder yields without a symbol."""
    rng = np.random.default_rng(12)
    lo, hi, P = -127, 127, 12
    lengths = [300, 0, 1, 4099, 64, 7, 0, 515] + rng.integers(1, 400, 100).tolist()
    docs = [np.clip(np.rint(rng.normal(rng.uniform(-60, 60), rng.uniform(0.5, 20), n)), lo, hi).astype(np.int32) for n in lengths]
    flat, offsets = B.ragged(docs)
    model = B.Model.fit_per_stream(flat, lo, hi, P, sym_offsets=offsets)
    assert model.n_tables == len(docs) and model.per_stream
    enc = B.ans_encode_ragged(flat, offsets, model, (32, 64, P))
    assert B.last_kernel() == "ans_encode_ragged_ps_kernel" and enc.jump is None
    torch.cuda.synchronize()
    w, wo, n, st = host(enc)
    assert st.tolist() == [0] * len(docs)
    for s in (0, 1, 2, 3, 6, 50):
        cdf = model.cdf(s)
        assert w[wo[s]: wo[s] + n[s]].tolist() == R.oracle_ans_words(docs[s], lo, cdf, P).tolist(), f"stream {s}"
    for s in (1, 6):
        prob = np.diff(model.cdf(s).astype(np.int64))
        assert prob.max() - prob.min() <= 1 and n[s] == len(R.oracle_ans_words(docs[s], lo, model.cdf(s), P))
    dec, status = B.ans_decode_ragged(enc, model, offsets)
    assert B.last_kernel() == "ans_decode_ragged_ps_kernel"
    assert status.cpu().tolist() == [0] * len(docs) and torch.equal(dec, flat)
    # the decoder has the rows alone
    rebuilt = B.Model.from_cdf_rows_per_stream(model.cdfs_device(), lo, P)
    dec2, status2 = B.ans_decode_ragged(enc, rebuilt, offsets)
    assert status2.cpu().tolist() == [0] * len(docs) and torch.equal(dec2, flat)


def test_status_and_bounds(B):
    """Through the C ABI, d_word_offsets == NULL: slabs `stride_words` apart, against the oracle -- and a stride too small for some
    streams: CST_STREAM_CAPACITY for exactly those, nothing written outside a slab (the fill behind every neighbour's words stays).
    Through the binding: an impossible symbol, an n_words beyond its slab, a jump point beyond its stream's words, a table with a chunk
    too many -- each flags its own stream alone."""
    for coder in CODERS:
        stride_slabs(B, coder)
        status_and_bounds(B, coder)


def stride_slabs(B, coder):
    from constriction_amd import _native as N
    case, n_streams = "skewed_fitted", 130
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (32, 64, P)
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    want = R.oracle_words(coder, case, n_streams)
    counts = np.array([len(x) for x in want])
    L, cc = N.lib(), N.CoderConfig(*cfg)

    def run(stride):
        words = torch.full((n_streams * stride + 8,), FILL, dtype=torch.int32, device="cuda")
        n_words = torch.full((n_streams,), -5, dtype=torch.int32, device="cuda")
        status = torch.full((n_streams,), -5, dtype=torch.int32, device="cuda")
        if coder == "ans":
            N.check(L.cst_ans_encode_ragged(model._h, cc, p(flat), p(offsets), n_streams, p(words), None, stride, p(n_words), p(status), None),
                    "cst_ans_encode_ragged")
        else:
            N.check(L.cst_range_encode_ragged(model._h, cc, p(flat), p(offsets), n_streams, None, p(words), None, stride, p(n_words), p(status),
                                              None), "cst_range_encode_ragged")
        assert B.last_kernel() == KERNELS[coder][0]
        torch.cuda.synchronize()
        return words, n_words, status

    stride = int(counts.max()) + 3              # (an odd stride: slabs that do not start on 16 bytes)
    words, n_words, status = run(stride)
    w = words.cpu().numpy().view(np.uint32)
    assert status.cpu().tolist() == [0] * n_streams and n_words.cpu().tolist() == counts.tolist()
    for s in range(n_streams):
        assert w[s * stride: s * stride + counts[s]].tolist() == want[s].tolist(), f"stream {s}"
        assert (w[s * stride + counts[s]: (s + 1) * stride] == FILL).all(), f"behind stream {s}"
    out = torch.full_like(flat, -7)
    dstatus = torch.full((n_streams,), -5, dtype=torch.int32, device="cuda")
    if coder == "ans":
        N.check(L.cst_ans_decode_ragged(model._h, cc, p(words), None, stride, words.numel(), p(n_words), p(out), p(offsets), n_streams, p(dstatus),
                                        None), "cst_ans_decode_ragged")
    else:
        N.check(L.cst_range_decode_ragged(model._h, cc, p(words), None, stride, words.numel(), p(n_words), p(out), p(offsets), n_streams, None,
                                          p(dstatus), None), "cst_range_decode_ragged")
    assert B.last_kernel() == KERNELS[coder][1]
    assert dstatus.cpu().tolist() == [0] * n_streams and torch.equal(out, flat)
    # a stride between the streams' needs: the median of the oracle's counts
    small = int(np.sort(counts)[n_streams // 2])
    over = counts > small
    assert over.any() and (~over).any()
    words, n_words, status = run(small)
    w = words.cpu().numpy().view(np.uint32)
    assert status.cpu().tolist() == np.where(over, 2, 0).tolist()
    assert n_words.cpu().tolist() == np.where(over, 0, counts).tolist()
    for s in np.flatnonzero(~over):
        assert w[s * small: s * small + counts[s]].tolist() == want[s].tolist(), f"stream {s}"
        assert (w[s * small + counts[s]: (s + 1) * small] == FILL).all(), f"behind stream {s}"
    assert (w[n_streams * small:] == FILL).all()


def status_and_bounds(B, coder):
    case, n_streams = "bimodal", 65
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (32, 64, P)
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    off = offsets.cpu().numpy()
    lengths = np.diff(off)
    # an impossible symbol flags its stream only
    victim = int(np.flatnonzero(lengths >= 64)[0])
    spoiled = flat.clone()
    spoiled[off[victim] + 20] = lo + R.CASES[case][0]
    enc = encode(B, coder, spoiled, offsets, model, cfg)
    torch.cuda.synchronize()
    want = R.oracle_words(coder, case, n_streams)
    w, wo, n, st = host(enc)
    assert st.tolist() == [1 if s == victim else 0 for s in range(n_streams)] and n[victim] == 0
    for s in (victim - 1, victim + 1):
        assert w[wo[s]: wo[s] + n[s]].tolist() == want[s].tolist()
    # an n_words beyond its stream's slab: that stream decodes as the empty stream and says INVALID_DATA, the others decode
    enc = encode(B, coder, flat, offsets, model, cfg)
    ref, ref_st = decode(B, coder, enc, model, offsets)
    assert ref_st.cpu().tolist() == [0] * n_streams and torch.equal(ref, flat)
    enc.n_words[victim] = 1 << 30
    dec, status = decode(B, coder, enc, model, offsets)
    assert status.cpu().tolist() == [3 if s == victim else 0 for s in range(n_streams)]
    assert torch.equal(dec[: off[victim]], flat[: off[victim]]) and torch.equal(dec[off[victim + 1]:], flat[off[victim + 1]:])
    # a jump point beyond its stream's words; a table with one chunk too many for its stream
    every = 64
    long_one = int(np.argmax(lengths))
    enc = encode(B, coder, flat, offsets, model, cfg, every=every)
    torch.cuda.synchronize()
    co = enc.jump.chunk_offsets.cpu().numpy()
    pos0 = enc.jump.pos.clone()
    enc.jump.pos[int(co[long_one]) + 3] = int(enc.n_words[long_one]) + 5
    dec, status = decode(B, coder, enc, model, offsets)
    assert B.last_kernel() == KERNELS[coder][1] + "<jump>"
    assert status.cpu().tolist() == [3 if s == long_one else 0 for s in range(n_streams)]
    assert torch.equal(dec[: off[long_one]], flat[: off[long_one]]) and torch.equal(dec[off[long_one + 1]:], flat[off[long_one + 1]:])
    enc.jump.pos.copy_(pos0)
    enc.jump.chunk_offsets[-1] += 1
    dec, status = decode(B, coder, enc, model, offsets)
    assert status.cpu().tolist() == [3 if s == n_streams - 1 else 0 for s in range(n_streams)]
    assert torch.equal(dec[: off[n_streams - 1]], flat[: off[n_streams - 1]])


def test_refusals(B):
    """n_tables != n_streams, a config whose precision is not the model's, and the calls that take shared tables only: ValueError before
    any launch (the last kernel's name is unchanged)"""
    case, n_streams = "skewed_fitted", 65
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (32, 64, P)
    model = model_of(B, cdfs, lo, P)
    flat, offsets = B.ragged(docs)
    shared = B.Model.from_cdf(np.array(cdfs[0]), lo, P)
    for coder in CODERS:
        enc = encode(B, coder, flat, offsets, model, cfg)
        jenc = encode(B, coder, flat, offsets, model, cfg, every=64)
        senc = encode(B, coder, flat, offsets, shared, cfg)
        name = SHARED_KERNELS[coder][0] + ("<jump>" if senc.jump is not None else "")
        assert B.last_kernel() == name
        fewer = B.ragged(docs[:-1])
        calls = [lambda: encode(B, coder, *fewer, model, cfg),
                 lambda: encode(B, coder, *fewer, model, cfg, every=64),
                 lambda: encode(B, coder, flat, offsets, model, (32, 64, P + 1)),
                 lambda: encode(B, coder, flat, offsets, model, (32, 64, P + 1), every=64),
                 lambda: decode(B, coder, enc, model, fewer[1]) if coder == "ans" else decode(B, coder, senc, model_of(B, cdfs[:-1], lo, P), offsets),
                 lambda: decode(B, coder, jenc, model_of(B, cdfs[:-1], lo, P), offsets),
                 lambda: (B.ans_decode_until if coder == "ans" else B.range_decode_until)(enc, model, lo),
                 lambda: (B.ans_decode_ragged_select if coder == "ans" else B.range_decode_ragged_select)(enc, model, offsets, [0, 1]),
                 lambda: (B.ans_decode_ragged_select if coder == "ans" else B.range_decode_ragged_select)(jenc, model, offsets, [0], [8], [8])]
        for k, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
            assert B.last_kernel() == name, f"call {k}"
    # the C entry points that keep refusing a per-stream model say so with their status
    from constriction_amd import _native as N
    L, cc = N.lib(), N.CoderConfig(*cfg)
    enc = encode(B, "ans", flat, offsets, model, cfg)
    lengths = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
    status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    assert L.cst_ans_count_until(model._h, cc, p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), n_streams, lo, 100, p(lengths),
                                 p(status), None) == N.CST_ERR_INVALID_ARGUMENT
    assert L.cst_range_count_until(model._h, cc, p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), n_streams, None, lo, 100,
                                   p(lengths), p(status), None) == N.CST_ERR_INVALID_ARGUMENT
    # ... and so does a ragged call whose stream count is not the model's table count
    assert L.cst_ans_encode_ragged(model._h, cc, p(flat), p(offsets), n_streams - 1, p(enc.words), p(enc.word_offsets), 0, p(enc.n_words),
                                   p(enc.status), None) == N.CST_ERR_INVALID_ARGUMENT
    assert L.cst_range_encode_ragged(model._h, cc, p(flat), p(offsets), n_streams - 1, None, p(enc.words), p(enc.word_offsets), 0, p(enc.n_words),
                                     p(enc.status), None) == N.CST_ERR_INVALID_ARGUMENT


def test_dispatch(B):
    """every route names its kernel; a shared-table ragged call still names the shared-table kernel"""
    from constriction_amd import _native as N
    case, n_streams = "p5", 63
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    cfg = (32, 64, P)
    model = model_of(B, cdfs, lo, P)
    shared = B.Model.from_cdf(np.array(cdfs[0]), lo, P)
    flat, offsets = B.ragged(docs)
    L, cc = N.lib(), N.CoderConfig(*cfg)
    for coder in CODERS:
        enc_name, dec_name = KERNELS[coder]
        enc = encode(B, coder, flat, offsets, model, cfg)
        assert B.last_kernel() == enc_name
        decode(B, coder, enc, model, offsets)
        assert B.last_kernel() == dec_name
        jenc = encode(B, coder, flat, offsets, model, cfg, every=8)
        assert B.last_kernel() == enc_name + "<jump>"
        decode(B, coder, jenc, model, offsets)
        assert B.last_kernel() == dec_name + "<jump>"
        senc = encode(B, coder, flat, offsets, shared, cfg, every=0)
        assert B.last_kernel() == SHARED_KERNELS[coder][0]
        decode(B, coder, senc, shared, offsets)
        assert B.last_kernel() == SHARED_KERNELS[coder][1]
    # the two ANS calls without a schedule (the binding goes through the *_ordered ones)
    enc = encode(B, "ans", flat, offsets, model, cfg)
    encode(B, "ans", flat, offsets, shared, cfg, every=0)
    N.check(L.cst_ans_encode_ragged(model._h, cc, p(flat), p(offsets), n_streams, p(enc.words), p(enc.word_offsets), 0, p(enc.n_words),
                                    p(enc.status), None), "cst_ans_encode_ragged")
    assert B.last_kernel() == "ans_encode_ragged_ps_kernel"
    out = torch.empty_like(flat)
    status = torch.empty(n_streams, dtype=torch.int32, device="cuda")
    encode(B, "ans", flat, offsets, shared, cfg, every=0)
    N.check(L.cst_ans_decode_ragged(model._h, cc, p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), p(out), p(offsets),
                                    n_streams, p(status), None), "cst_ans_decode_ragged")
    assert B.last_kernel() == "ans_decode_ragged_ps_kernel"
    assert status.cpu().tolist() == [0] * n_streams and torch.equal(out, flat)
