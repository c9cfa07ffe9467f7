"""GPU: the range coder with one table per stream (cst_range_ps.hip) -- plain calls, jump points, narrow symbol matrices, fitted models
and the errors that must not disturb a stream's neighbours -- against the CPU oracle's range coder run once per stream, every stream
of every case compared bit for bit (tests/per_stream_rows.py; tests/test_range_per_stream_cpu.py shows that the comparison is sound)."""
import numpy as np
import pytest

import per_stream_rows as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IMPOSSIBLE, CAPACITY, INVALID = 1, 2, 3
GUARD = 0x5EEDBEEF


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from constriction_amd import batched
    return batched


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared batches are read-only)


def model_of(B, cdfs, lo, P):
    return B.Model.from_cdf_rows_per_stream(dev(cdfs.view(np.int32)), lo, P)


def assert_words(enc, want, streams=None, where=""):
    """words and counts of the oracle, stream by stream; statuses 0"""
    want_words, want_n, want_status = want
    words, n_words, status = enc.to_numpy()
    streams = range(len(want_n)) if streams is None else streams
    for s in streams:
        assert status[s] == 0 and want_status[s] == 0, f"{where} stream {s}"
        assert n_words[s] == want_n[s], f"{where} stream {s}"
        assert np.array_equal(words[s, : n_words[s]], want_words[s, : want_n[s]]), f"{where} stream {s}"


def roundtrip(B, case, n_streams, n_per, W, S):
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    cfg, shape = (W, S, P), (n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    enc = B.range_encode(dev(sym), model, cfg)
    assert B.last_kernel() == "range_encode_ps_kernel", (shape, B.last_kernel())
    assert enc.jump is None, shape                          # ("auto" notes no points for tables per stream)
    assert_words(enc, R.oracle_encode(case, n_streams, n_per, W, S), where=shape)
    dec, status = B.range_decode(enc, model, n_per)
    assert B.last_kernel() == "range_decode_ps_kernel", (shape, B.last_kernel())
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym), shape


@pytest.mark.parametrize("case", list(R.CASES))
def test_words_are_the_oracles(B, case):
    """every shape of R.SHAPES in one test per row family (a shape costs some 10 ms)"""
    for n_streams, n_per in R.SHAPES:
        roundtrip(B, case, n_streams, n_per, 32, 64)


@pytest.mark.parametrize("case", R.W16_CASES)
def test_words_are_the_oracles_w16(B, case):
    for n_streams, n_per in R.W16_SHAPES:
        roundtrip(B, case, n_streams, n_per, 16, 32)


@pytest.mark.parametrize("W,S", [(32, 64), (16, 32)])
def test_empty_streams(B, O, W, S):
    lo, P, cdfs, _ = R.batch("bimodal", 64, 96)
    sym = np.zeros((64, 0), np.int32)
    model = model_of(B, cdfs, lo, P)
    enc = B.range_encode(dev(sym), model, (W, S, P))
    assert B.last_kernel() == "range_encode_ps_kernel"
    assert_words(enc, R.oracle_encode_rows(sym, lo, cdfs, P, W, S))
    dec, status = B.range_decode(enc, model, 0)
    assert tuple(dec.shape) == (64, 0) and (status.cpu().numpy() == 0).all()


@pytest.mark.parametrize("case,n_streams,n_per", [("bimodal", 65, 33), ("p16_n300", 130, 100)])
def test_symbol_major(B, case, n_streams, n_per):
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    plain = B.range_encode(dev(sym), model, (32, 64, P))
    encT = B.range_encode(dev(sym.T), model, (32, 64, P), "symbol_major")
    assert B.last_kernel() == "range_encode_ps_kernel"
    assert_words(encT, plain.to_numpy())
    assert_words(encT, R.oracle_encode(case, n_streams, n_per))
    decT, status = B.range_decode(encT, model, n_per, "symbol_major")
    assert B.last_kernel() == "range_decode_ps_kernel"
    assert tuple(decT.shape) == (n_per, n_streams) and (status.cpu().numpy() == 0).all() and np.array_equal(decT.cpu().numpy().T, sym)


@pytest.mark.parametrize("cfg", [(32, 64, 12), (16, 32, 12), (32, 64, 16)], ids=lambda c: "W%dS%dP%d" % c)
def test_gaussian_rows(B, cfg):
    """Model.quantized_gaussian_per_stream: the words of the oracle's range coder over the model's own rows"""
    n_streams, n_per, P = 130, 100, cfg[2]
    rng = np.random.default_rng(P)
    mu, sigma = rng.uniform(-10, 10, n_streams), np.exp(rng.uniform(np.log(0.5), np.log(16), n_streams))
    model = B.Model.quantized_gaussian_per_stream(-127, 127, dev(mu), dev(sigma), P)
    cdfs = model.cdfs_device().cpu().numpy().view(np.uint32)
    assert R.rows_are_valid(cdfs, P)
    sym = np.clip(np.rint(rng.normal(mu[:, None], sigma[:, None], (n_streams, n_per))), -127, 127).astype(np.int32)
    enc = B.range_encode(dev(sym), model, cfg)
    assert B.last_kernel() == "range_encode_ps_kernel"
    assert_words(enc, R.oracle_encode_rows(sym, -127, cdfs, P, cfg[0], cfg[1]))
    dec, status = B.range_decode(enc, model, n_per)
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


def assert_jump_table(ck, want):
    pos, lower, rng = want
    assert np.array_equal(ck.pos.cpu().numpy().view(np.uint32), pos)
    assert np.array_equal(ck.lower.cpu().numpy().view(np.uint64), lower)
    assert np.array_equal(ck.range.cpu().numpy().view(np.uint64), rng)


def assert_chunk_decodes_alone(O, enc, ck, stream, chunk, lo, cdfs, P, sym, W=32, S=64):
    """the oracle's RangeDecoder, sought to the device's table entry, returns that chunk"""
    words, n_words, _ = enc.to_numpy()
    first = chunk * ck.interval
    count = min(ck.interval, sym.shape[1] - first)
    got, st = O.range_decode_from(words[stream, : n_words[stream]], ck.pos.cpu().numpy().view(np.uint32)[stream, chunk],
                                  ck.lower.cpu().numpy().view(np.uint64)[stream, chunk], ck.range.cpu().numpy().view(np.uint64)[stream, chunk],
                                  count, lo, cdfs[stream], P, W, S)
    assert st == 0 and np.array_equal(got, sym[stream, first: first + count])


# (case, n_streams, n_per, interval, W, S): intervals that divide the rows -- 32 (whole tiles), 100 and 4099 (one chunk), 50, 25 and 20
# (several chunks that are no whole tiles; 25: rows of the virtual matrix that are not 16-byte aligned)
JUMPS = [("bimodal", 64, 96, 32, 32, 64), ("bimodal", 130, 100, 100, 32, 64), ("skewed_fitted", 130, 100, 50, 32, 64),
         ("p16_n300", 130, 100, 25, 32, 64), ("n_2_to_P", 130, 100, 20, 32, 64), ("p5", 130, 100, 50, 16, 32),
         ("bimodal", 257, 4099, 4099, 32, 64), ("n_2_to_P", 64, 96, 32, 16, 32)]


@pytest.mark.parametrize("case,n_streams,n_per,interval,W,S", JUMPS)
def test_jump_points(B, O, case, n_streams, n_per, interval, W, S):
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    cfg = (W, S, P)
    model = model_of(B, cdfs, lo, P)
    plain = B.range_encode(dev(sym), model, cfg, jump_points=0)
    assert plain.jump is None and B.last_kernel() == "range_encode_ps_kernel"
    enc = B.range_encode(dev(sym), model, cfg, jump_points=n_per // interval)
    assert B.last_kernel() == "range_encode_ps_kernel<ckpt>", B.last_kernel()
    assert isinstance(enc.jump, B.RangeCheckpoints) and enc.jump.interval == interval
    assert_jump_table(enc.jump, R.oracle_jump_table(sym, lo, cdfs, P, interval, W, S))
    assert_words(enc, plain.to_numpy())                                         # the words of the plain call, bit for bit
    assert_words(enc, R.oracle_encode(case, n_streams, n_per, W, S))
    dec, status = B.range_decode(enc, model, n_per)
    assert B.last_kernel() == "range_decode_ps_kernel<chunks>", B.last_kernel()
    assert tuple(status.shape) == (n_streams,) and (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    last = n_per // interval - 1
    for stream, chunk in ((0, 0), (n_streams // 2, last // 2), (n_streams - 1, last)):
        assert_chunk_decodes_alone(O, enc, enc.jump, stream, chunk, lo, cdfs, P, sym, W, S)


@pytest.mark.parametrize("case,n_streams,n_per,interval", [("bimodal", 130, 100, 32), ("uniform", 257, 4099, 100), ("p16_n300", 257, 4099, 32)])
def test_jump_interval_that_does_not_divide_the_rows(B, O, case, n_streams, n_per, interval):
    """range_encode_checkpointed notes ceil(n_per / interval) points, the last chunk is short; such a table decodes chunk by chunk
    (RangeDecoder.seek), not through range_decode_checkpointed"""
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    enc, ck = B.range_encode_checkpointed(dev(sym), model, interval, (32, 64, P))
    assert B.last_kernel() == "range_encode_ps_kernel<ckpt>", B.last_kernel()
    n_chunks = -(-n_per // interval)
    assert tuple(ck.pos.shape) == (n_streams, n_chunks)
    assert_jump_table(ck, R.oracle_jump_table(sym, lo, cdfs, P, interval))
    assert_words(enc, R.oracle_encode(case, n_streams, n_per))
    for stream, chunk in ((0, 0), (n_streams - 1, n_chunks - 1), (n_streams // 2, n_chunks // 2)):
        assert_chunk_decodes_alone(O, enc, ck, stream, chunk, lo, cdfs, P, sym)
    with pytest.raises(ValueError):                                             # a table whose shape does not fit raises, as for shared tables
        B.range_decode_checkpointed(enc, ck, model, n_per)


@pytest.mark.parametrize("dtype", [np.int8, np.int16], ids=["int8", "int16"])
def test_narrow_symbols(B, dtype):
    """int8 / int16 matrices are widened / narrowed next to the int32 kernels: the words of the int32 call"""
    case, n_streams, n_per = "bimodal", 130, 100
    tdtype = torch.int8 if dtype == np.int8 else torch.int16
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    want = R.oracle_encode(case, n_streams, n_per)
    narrow = dev(sym.astype(dtype))
    enc = B.range_encode(narrow, model, (32, 64, P))
    assert B.last_kernel() == "range_encode_ps_kernel", B.last_kernel()
    assert_words(enc, B.range_encode(dev(sym), model, (32, 64, P)).to_numpy())
    assert_words(enc, want)
    dec, status = B.range_decode(enc, model, n_per, dtype=tdtype)
    assert B.last_kernel() == "range_decode_ps_kernel", B.last_kernel()
    assert dec.dtype == tdtype and (status.cpu().numpy() == 0).all() and torch.equal(dec, narrow)
    encj = B.range_encode(narrow, model, (32, 64, P), jump_points=2)
    assert B.last_kernel() == "range_encode_ps_kernel<ckpt>", B.last_kernel()
    assert_words(encj, want)
    assert_jump_table(encj.jump, R.oracle_jump_table(sym, lo, cdfs, P, n_per // 2))
    decj, status = B.range_decode(encj, model, n_per, dtype=tdtype)
    assert B.last_kernel() == "range_decode_ps_kernel<chunks>", B.last_kernel()
    assert decj.dtype == tdtype and (status.cpu().numpy() == 0).all() and torch.equal(decj, narrow)


def test_fit_per_stream_end_to_end(B):
    """static two-pass coding of a queue: fit one table per stream, range-encode; the decoder has the rows alone"""
    rng = np.random.default_rng(5)
    n_streams, n_per, lo, hi, P = 130, 100, -127, 127, 12
    mu, sigma = rng.uniform(-60, 60, (n_streams, 1)), np.exp(rng.uniform(np.log(0.3), np.log(30), (n_streams, 1)))
    sym_np = np.clip(np.round(rng.normal(mu, sigma, (n_streams, n_per))), lo, hi).astype(np.int32)
    sym_np[7] = 5                                           # a stream of one symbol
    sym = dev(sym_np)
    model = B.Model.fit_per_stream(sym, lo, hi, P)
    enc = B.range_encode(sym, model, (32, 64, P))
    assert B.last_kernel() == "range_encode_ps_kernel"
    assert int(enc.status.abs().sum()) == 0
    rebuilt = B.Model.from_cdf_rows_per_stream(model.cdfs_device().clone(), lo, P)
    dec, st = B.range_decode(enc, rebuilt, n_per)
    assert B.last_kernel() == "range_decode_ps_kernel"
    assert int(st.abs().sum()) == 0 and torch.equal(dec, sym)


def test_tuned_stride_takes_per_stream_models(B):
    lo, P, cdfs, sym = R.batch("bimodal", 130, 100)
    model = model_of(B, cdfs, lo, P)
    stride = B.tuned_stride(dev(sym), model, (32, 64, P), coder="range")        # (a small batch: max_words at once, nothing is measured)
    assert stride == B.range_max_words(100, (32, 64, P))
    enc = B.range_encode(dev(sym), model, (32, 64, P), stride="tuned")
    assert enc.stride == stride
    assert_words(enc, R.oracle_encode("bimodal", 130, 100))


# ---- errors that must not disturb a stream's neighbours ----------------------------------------------------------------------------

def test_impossible_symbol(B):
    case, n_streams, n_per = "bimodal", 130, 100
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    want = R.oracle_encode(case, n_streams, n_per)
    for bad_stream, at, value in ((64, 37, lo + cdfs.shape[1] - 1), (129, 99, lo - 1), (0, 0, 1 << 30)):
        broken = sym.copy()
        broken[bad_stream, at] = value
        enc = B.range_encode(dev(broken), model, (32, 64, P))
        _, n_words, status = enc.to_numpy()
        assert status[bad_stream] == IMPOSSIBLE and n_words[bad_stream] == 0
        assert_words(enc, want, [s for s in range(n_streams) if s != bad_stream])


def test_capacity(B):
    """a stride too small for some streams: they report CST_STREAM_CAPACITY, nothing outside the slabs changes, no stream writes
    behind its own count into a neighbour's slab, and the streams that fit are the oracle's"""
    case, n_streams, n_per = R.CAPACITY_CASE
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    want_words, want_n, _ = R.oracle_encode(case, n_streams, n_per)
    stride = R.capacity_stride()
    over = want_n > stride
    assert over.any() and (~over).any()
    model = model_of(B, cdfs, lo, P)
    front, back = 7, 9                                      # (guard words around the slabs; the slabs start off a 16-byte boundary)
    flat = torch.full((front + n_streams * stride + back,), GUARD, dtype=torch.int32, device="cuda")
    slabs = flat[front: front + n_streams * stride].view(n_streams, stride)
    out = B.EncodedBatch(slabs, torch.zeros(n_streams, dtype=torch.int32, device="cuda"), torch.zeros(n_streams, dtype=torch.int32, device="cuda"),
                         (32, 64, P))
    enc = B.range_encode(dev(sym), model, (32, 64, P), out=out)
    assert B.last_kernel() == "range_encode_ps_kernel"
    torch.cuda.synchronize()
    words, n_words, status = enc.to_numpy()
    everything = flat.cpu().numpy().view(np.uint32)
    guard = np.uint32(GUARD)
    assert (everything[:front] == guard).all() and (everything[front + n_streams * stride:] == guard).all()
    assert (status[over] == CAPACITY).all() and (n_words[over] == 0).all()
    assert (status[~over] == 0).all()
    for s in np.flatnonzero(~over):
        assert n_words[s] == want_n[s] and np.array_equal(words[s, : want_n[s]], want_words[s, : want_n[s]]), f"stream {s}"
        assert (words[s, want_n[s]:] == guard).all(), f"stream {s} wrote behind its words"
    for s in np.flatnonzero(over):                          # what an overflowing stream did write is the front of its own words
        written = words[s] != guard
        assert np.array_equal(words[s][written], want_words[s, :stride][written]), f"stream {s}"


def test_bad_word_counts(B):
    """packed words with offsets (what container.load hands over): offsets beyond the buffer and counts that run past its end report
    CST_STREAM_INVALID_DATA and read nothing; the other streams decode"""
    case, n_streams, n_per = "bimodal", 257, 4099
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    enc = B.range_encode(dev(sym), model, (32, 64, P))
    packed, offsets = B.compact(enc)
    torch.cuda.synchronize()
    total = int(offsets[-1].item())
    packed = packed[:total].clone()                                   # the buffer IS its valid words: capacity = total
    off = offsets.cpu().numpy().astype(np.int64)
    n = enc.n_words.cpu().numpy().astype(np.int64)
    off[3] = total + 1
    off[64] = 1 << 40
    off[65] = -8                                                      # (2^64 - 8 as unsigned)
    n[100] = total                                                    # starts inside, ends far outside
    n[200] = 0xFFFFFFFF
    n[256] = n[256] + 1                                               # one word past the end of the buffer
    bad = [3, 64, 65, 100, 200, 256]
    dec, status = B.range_decode((packed, dev(n.astype(np.uint32).view(np.int32))), model, n_per, offsets=dev(off), config=(32, 64, P))
    assert B.last_kernel() == "range_decode_ps_kernel"
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    ok = np.ones(n_streams, bool)
    ok[bad] = False
    assert (st[~ok] == INVALID).all() and (st[ok] == 0).all()
    assert np.array_equal(dec.cpu().numpy()[ok], sym[ok])


def test_jump_point_beyond_its_stream(B):
    """a jump point that claims more words than its stream has: that chunk reports CST_STREAM_INVALID_DATA, the others decode"""
    case, n_streams, n_per = "bimodal", 130, 100
    lo, P, cdfs, sym = R.batch(case, n_streams, n_per)
    model = model_of(B, cdfs, lo, P)
    enc = B.range_encode(dev(sym), model, (32, 64, P), jump_points=2)
    ck = enc.jump
    pos = ck.pos.cpu().numpy().copy()
    n_words = enc.n_words.cpu().numpy()
    pos[5, 1] = n_words[5] + 1
    pos[129, 1] = -1                                                  # (2^32 - 1 as unsigned)
    broken = B.RangeCheckpoints(ck.interval, dev(pos), ck.lower, ck.range)
    dec, status = B.range_decode_checkpointed(enc, broken, model, n_per)
    assert B.last_kernel() == "range_decode_ps_kernel<chunks>"
    st = status.cpu().numpy()
    want = np.zeros((n_streams, 2), np.int32)
    want[5, 1] = want[129, 1] = INVALID
    assert np.array_equal(st, want)
    got = dec.cpu().numpy().reshape(n_streams, 2, 50)
    ok = want == 0
    assert np.array_equal(got[ok], sym.reshape(n_streams, 2, 50)[ok])


def test_refused_without_a_launch(B):
    from constriction_amd import _native as N
    lo, P, cdfs, sym = R.batch("bimodal", 130, 100)
    model = model_of(B, cdfs, lo, P)
    B.range_encode(dev(sym), model, (32, 64, P))
    before = B.last_kernel()
    assert before == "range_encode_ps_kernel"
    with pytest.raises(ValueError, match="one table per stream"):           # 130 tables, 129 streams
        B.range_encode(dev(sym[:129]), model, (32, 64, P))
    enc = B.range_encode(dev(sym), model, (32, 64, P))
    with pytest.raises(ValueError, match="one table per stream"):
        B.range_decode((enc.words[:129], enc.n_words[:129]), model, 100, config=(32, 64, P))
    with pytest.raises(ValueError, match="stream-major"):                   # symbol-major with jump points
        B.range_encode(dev(sym.T), model, (32, 64, P), "symbol_major", jump_points=2)
    with pytest.raises(ValueError, match="stream-major"):
        B.range_encode_checkpointed(dev(sym.T), model, 50, (32, 64, P), "symbol_major")
    # the C calls themselves: CST_FLAG_RAW_STATE, another number of streams, symbol-major with jump points
    L = N.lib()
    d_sym = dev(sym)
    words = torch.zeros((130, B.range_max_words(100, (32, 64, P))), dtype=torch.int32, device="cuda")
    n_words, status = torch.zeros(130, dtype=torch.int32, device="cuda"), torch.zeros(130, dtype=torch.int32, device="cuda")
    rstate = torch.zeros((130, 5), dtype=torch.int64, device="cuda")        # (cst_range_state: 40 bytes)
    out = torch.zeros((130, 100), dtype=torch.int32, device="cuda")
    cfg, p, sp = B._cfg(32, 64, P), B._ptr, B._stream_ptr()
    assert L.cst_range_encode_batch(model._h, cfg, p(d_sym), 130, 100, N.LAYOUT_STREAM_MAJOR, p(words), words.shape[1], p(n_words), p(rstate),
                                    p(status), N.FLAG_RAW_STATE, sp) == N.CST_ERR_INVALID_ARGUMENT
    assert L.cst_range_decode_batch(model._h, cfg, p(enc.words), None, enc.stride, enc.words.numel(), p(enc.n_words), p(out), 130, 100,
                                    N.LAYOUT_STREAM_MAJOR, p(rstate), p(status), N.FLAG_RAW_STATE, sp) == N.CST_ERR_INVALID_ARGUMENT
    assert L.cst_range_encode_batch(model._h, cfg, p(d_sym), 129, 100, N.LAYOUT_STREAM_MAJOR, p(words), words.shape[1], p(n_words), None,
                                    p(status), N.FLAG_NONE, sp) == N.CST_ERR_INVALID_ARGUMENT
    pos = torch.zeros((130, 2), dtype=torch.int32, device="cuda")
    lower, rng = torch.zeros((130, 2), dtype=torch.int64, device="cuda"), torch.zeros((130, 2), dtype=torch.int64, device="cuda")
    assert L.cst_range_encode_batch_ckpt(model._h, cfg, p(d_sym), 130, 100, N.LAYOUT_SYMBOL_MAJOR, p(words), words.shape[1], p(n_words), 50,
                                         p(pos), p(lower), p(rng), p(status), sp) == N.CST_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert B.last_kernel() == "range_encode_ps_kernel"                      # (the last launch is still the good encode call above)
    assert int(words.abs().sum()) == 0 and int(out.abs().sum()) == 0
