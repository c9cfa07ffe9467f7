"""GPU tests of the ragged per-symbol Categorical calls: batched.{ans,range}_{encode,decode}_categorical_ragged, their `jump_every`, and the
kernels behind them (csrc/cst_persymbol_categorical_ragged.hip).

Every expected word, count and jump table comes from the CPU oracle alone: one tabulated model per symbol over
oracle.categorical_fast_cdf (f32 rows in f32, f64 rows in f64) fed to one oracle coder per stream, and the same coder coded chunk by chunk
for the tables (tests/persymbol_jump_oracle.py).  No GPU result is the reference for another, except where a test says that two GPU
calls must agree.  Rows and symbols are drawn by the recipe of tests/test_gpu_categorical_batch.py::workload: unnormalised Dirichlet(0.3)
rows with exact zeros inside, a last entry of at least 2e-3 of the sum (every table here is strictly increasing; the degenerate ones
are run through these kernels by tests/test_gpu_categorical_extremes.py), and symbols 0 and K - 1 in front of every stream.  A batch
and its oracle results are built once per key, shared, and never modified."""
import numpy as np
import pytest

from persymbol_jump_oracle import ans_table, range_table

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 64                  # kCatChunk: columns of a row staged at a time
CONFIGS = [(32, 64, 24), (16, 32, 12)]
CODERS = ["ans", "range"]
# paired, not a cross product: the chunk edges C - 1, C, C + 1, 2 C + 1, and both load paths (16-byte loads need K * sizeof % 16 == 0)
MODELS = [(2, "f64"), (5, "f32"), (CHUNK - 1, "f32"), (CHUNK, "f64"), (CHUNK + 1, "f32"), (2 * CHUNK + 1, "f64"), (257, "f32")]
DTYPES = {"f32": np.float32, "f64": np.float64}
# 70 streams: a full decoder wave and a partial one
PARITY_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300, 0] * 5
OK, IMPOSSIBLE, CAPACITY, INVALID = 0, 1, 2, 3
cfg_id = lambda c: "W%dS%dP%d" % c
model_id = lambda m: "K%d-%s" % m


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def workload(lengths, k, dtype, seed):
    """flat probabilities [sum(lengths), k] and flat symbols: uniform draws (so they sit on exact-zero entries too), with symbol 0 and
    symbol k - 1 in front of every stream (alternating over the streams where a stream has one symbol)"""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    probs = rng.dirichlet(np.full(k, 0.3), size=n)
    if k > 2:
        probs[:, 1:-1][rng.random((n, k - 2)) < 0.3] = 0.0
    probs[:, -1] = np.maximum(probs[:, -1], 2e-3)               # (the sum stays below 1.002: at least 1e-3 of it)
    probs *= np.exp(rng.uniform(-3.0, 3.0, (n, 1)))              # not normalised
    probs = np.ascontiguousarray(probs.astype(dtype))
    sym = rng.integers(0, k, n).astype(np.int32)
    off = offsets_of(lengths)
    for s, length in enumerate(lengths):
        if length >= 2:
            sym[off[s]], sym[off[s] + 1] = 0, k - 1
        elif length == 1:
            sym[off[s]] = k - 1 if s % 2 == 0 else 0
    return sym, probs


def models_of(O, probs, P):
    return [O.TableModel(O.categorical_fast_cdf(row, P), 0, P) for row in probs]


def oracle_words(O, coder, cfg, sym, models):
    """get_compressed() of one oracle coder (a zero-length stream: no words from either coder)"""
    W, S, P = cfg
    if coder == "ans":
        if len(sym) == 0:
            return np.zeros(0, np.uint32)
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return np.asarray(c.get_compressed())


_BATCHES = {}       # (lengths key, k, dtype, P) -> (sym, probs, off, models per stream)
_WORDS = {}         # (batch key, coder, cfg) -> oracle words per stream
_TABLES = {}        # (batch key, coder, cfg, every) -> [(words, table)] per stream


def batch(O, name, lengths, k, dtype, P):
    key = (name, k, dtype, P)
    if key not in _BATCHES:
        sym, probs = workload(lengths, k, DTYPES[dtype], 17 * k + P + len(lengths))
        off = offsets_of(lengths)
        models = models_of(O, probs, P)
        _BATCHES[key] = (sym, probs, off, [models[off[s]: off[s + 1]] for s in range(len(lengths))])
    return key, _BATCHES[key]


def words_of(O, key, coder, cfg):
    if (key, coder, cfg) not in _WORDS:
        sym, _, off, models = _BATCHES[key]
        _WORDS[(key, coder, cfg)] = [oracle_words(O, coder, cfg, sym[off[s]: off[s + 1]], models[s]) for s in range(len(models))]
    return _WORDS[(key, coder, cfg)]


def tables_of(O, key, coder, cfg, every):
    if (key, coder, cfg, every) not in _TABLES:
        sym, _, off, models = _BATCHES[key]
        table_of = ans_table if coder == "ans" else range_table
        _TABLES[(key, coder, cfg, every)] = [table_of(O, cfg, sym[off[s]: off[s + 1]], models[s], every) for s in range(len(models))]
    return _TABLES[(key, coder, cfg, every)]


def batch_streams(enc):
    """every stream's words of a RaggedBatch, with one copy to the host"""
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n[s]] for s in range(len(n))], n


def assert_streams_equal(got, n_words, want, skip=()):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        if s not in skip:
            assert n_words[s] == len(w) and g.tolist() == w.tolist(), f"stream {s}: {n_words[s]} words, the oracle has {len(w)}"


def device_tables(enc):
    """the batch's jump table, per stream, as the oracle helpers give it: [(pos, state)] or [(pos, lower, range)]"""
    jump = enc.jump
    off = jump.chunk_offsets.cpu().numpy()
    pos = jump.pos.cpu().numpy().view(np.uint32)
    arrays = [jump.state] if enc.coder == "ans" else [jump.lower, jump.range]
    cols = [pos] + [a.cpu().numpy().view(np.uint64) for a in arrays]
    return [[tuple(int(c[k]) for c in cols) for k in range(off[s], off[s + 1])] for s in range(len(off) - 1)]


def calls(B, coder):
    return getattr(B, f"{coder}_encode_categorical_ragged"), getattr(B, f"{coder}_decode_categorical_ragged")


def assert_all_ok(status):
    assert (status.cpu().numpy() == OK).all(), status.cpu().tolist()


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("model", MODELS, ids=model_id)
def test_parity(B, O, model, coder, cfg):
    """70 streams of 0 .. 300 symbols: words, counts and statuses of every stream are its oracle coder's, decoding returns the input"""
    k, dtype = model
    lengths = PARITY_LENGTHS
    assert len(lengths) == 70
    key, (sym, probs, off, _) = batch(O, "parity", lengths, k, dtype, cfg[2])
    want = words_of(O, key, coder, cfg)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    for order in (None, B.ragged_order(dev(np.asarray(lengths, dtype=np.int64)))):
        enc = encode(d_sym, d_off, d_probs, cfg, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_encode_categorical_ragged_two_pass"
        assert enc.coder == coder and enc.jump is None and (enc.order is None) == (order is None)
        assert_all_ok(enc.status)
        got, n_words = batch_streams(enc)
        assert_streams_equal(got, n_words, want)
        dec, status = decode(enc, d_off, d_probs, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_decode_categorical_ragged_kernel"
        assert_all_ok(status)
        assert torch.equal(dec, d_sym)
    # "auto": the encoder's schedule, or none below RAGGED_BALANCE_FROM streams
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)


@pytest.mark.parametrize("coder", CODERS)
def test_more_streams_than_one_encoder_workgroup(B, O, coder):
    """300 streams of 0 .. 40 symbols: two workgroups of pass 2, five decoder waves"""
    cfg, k = (32, 64, 24), 5
    lengths = np.random.default_rng(300).integers(0, 41, 300).tolist()
    key, (sym, probs, off, _) = batch(O, "wide", lengths, k, "f32", cfg[2])
    want = words_of(O, key, coder, cfg)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg)
    torch.cuda.synchronize()
    assert_all_ok(enc.status)
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)


@pytest.mark.parametrize("every", [16, 48])
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("model", MODELS, ids=model_id)
def test_jump_points(B, O, model, coder, cfg, every):
    """the parity batch with a jump point every 16 / 48 symbols (210 / 95 table entries: several decoder waves and a partial one)"""
    k, dtype = model
    lengths = PARITY_LENGTHS
    key, (sym, probs, off, _) = batch(O, "parity", lengths, k, dtype, cfg[2])
    want = tables_of(O, key, coder, cfg, every)
    chunks = [-(-n // every) for n in lengths]
    assert sum(chunks) > 64 and sum(chunks) % 64 != 0
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_encode_categorical_ragged_two_pass<jump>"
    assert_all_ok(enc.status)
    # the words are the oracle's, coded chunk by chunk and in one go, and the plain call's: the same slabs, counts and statuses
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, [w for w, _ in want])
    assert_streams_equal(got, n_words, words_of(O, key, coder, cfg))
    plain = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=0)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_encode_categorical_ragged_two_pass" and plain.jump is None
    assert torch.equal(plain.word_offsets, enc.word_offsets) and torch.equal(plain.n_words, enc.n_words) and torch.equal(plain.status, enc.status)
    got_plain, _ = batch_streams(plain)
    assert_streams_equal(got, n_words, got_plain)
    # the table equals the oracle's pos(), per chunk
    jump = enc.jump
    assert isinstance(jump, B.RaggedJump if coder == "ans" else B.RangeRaggedJump) and jump.interval == every
    assert jump.chunk_offsets.cpu().tolist() == offsets_of(chunks).tolist() and jump.pos.numel() >= sum(chunks)
    for s, (g, (_, w)) in enumerate(zip(device_tables(enc), want)):
        assert g == w, f"stream {s} ({lengths[s]} symbols): the table differs from the oracle's"
    # decoding through the chunks ...
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_decode_categorical_ragged_kernel<jump>"
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)
    # ... a schedule handed in decodes whole streams ...
    dec, status = decode(enc, d_off, d_probs, order=torch.arange(len(lengths), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_decode_categorical_ragged_kernel"
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)
    # ... and Seek: one chunk decoded alone from its entry -- a batch of one stream that is that chunk -- equals that slice
    s = int(np.argmax(lengths))
    c0, w_off = int(jump.chunk_offsets[s].item()), enc.word_offsets[s: s + 2].clone()
    for j in (0, chunks[s] // 2, chunks[s] - 1):
        lo, hi = int(off[s]) + j * every, int(off[s]) + min((j + 1) * every, lengths[s])
        entry = [t[c0 + j: c0 + j + 1].clone() for t in ((jump.pos, jump.state) if coder == "ans" else (jump.pos, jump.lower, jump.range))]
        one = type(jump)(every, dev(np.array([0, 1], dtype=np.int64)), *entry)
        alone = B.RaggedBatch(enc.words, w_off, enc.n_words[s: s + 1].clone(), enc.status[s: s + 1].clone(), enc.config, None, one, coder)
        out = torch.full_like(d_sym, -7)
        _, status = decode(alone, dev(np.array([lo, hi], dtype=np.int64)), d_probs, out=out)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [OK], (j, status.cpu().tolist())
        assert torch.equal(out[lo:hi], d_sym[lo:hi]), j
        assert (out[:lo] == -7).all() and (out[hi:] == -7).all(), j


LOCAL_LENGTHS = [100, 0, 200, 47, 48, 150, 49, 500, 96]


@pytest.mark.parametrize("every", [0, 48])
@pytest.mark.parametrize("coder", CODERS)
def test_failures_stay_local(B, O, coder, every):
    """a NaN row in stream 2 and a symbol >= K in stream 5: those two report IMPOSSIBLE_SYMBOL and no words, every other stream's
    words are the oracle's and decode to their input.  Nothing is asserted about what the flagged streams decode to."""
    cfg, k = (32, 64, 24), 65
    lengths = LOCAL_LENGTHS
    key, (sym, probs, off, _) = batch(O, "local", lengths, k, "f32", cfg[2])
    want = words_of(O, key, coder, cfg)
    sym, probs = sym.copy(), probs.copy()
    probs[off[2] + 100, 7] = np.nan
    sym[off[5] + 149] = k
    flagged = (2, 5)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [IMPOSSIBLE if s in flagged else OK for s in range(len(lengths))]
    got, n_words = batch_streams(enc)
    assert all(n_words[s] == 0 for s in flagged)
    assert_streams_equal(got, n_words, want, skip=flagged)
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    if not every:
        assert st[2] == IMPOSSIBLE                              # (the plain decoder meets the NaN row too; a flagged stream's table is unspecified)
    for s in range(len(lengths)):
        if s not in flagged:
            assert st[s] == OK and torch.equal(dec[off[s]: off[s + 1]], d_sym[off[s]: off[s + 1]]), s


@pytest.mark.parametrize("coder", CODERS)
def test_another_batchs_chunk_offsets(B, O, coder):
    """decoded with the chunk_offsets of a batch whose streams 2, 3 and 8 have other chunk counts (the offsets of all other streams
    agree): those three report INVALID_DATA, the rest decode"""
    cfg, k, every = (32, 64, 24), 65, 48
    lengths = LOCAL_LENGTHS
    other = list(lengths)
    other[2], other[3], other[8] = 150, 95, 20                  # 5 + 1 chunks -> 4 + 2, and 2 -> 1
    key, (sym, probs, off, _) = batch(O, "local", lengths, k, "f32", cfg[2])
    _, (osym, oprobs, ooff, _) = batch(O, "other", other, k, "f32", cfg[2])
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, jump_every=every)
    foreign = encode(dev(osym), dev(ooff), dev(oprobs), cfg, jump_every=every)
    torch.cuda.synchronize()
    assert_all_ok(enc.status)
    mine, theirs = enc.jump.chunk_offsets.cpu().tolist(), foreign.jump.chunk_offsets.cpu().tolist()
    assert [i for i in range(len(mine)) if mine[i] != theirs[i]] == [3, 9]
    jump = enc.jump
    arrays = (jump.pos, jump.state) if coder == "ans" else (jump.pos, jump.lower, jump.range)
    swapped = type(jump)(every, foreign.jump.chunk_offsets, *arrays)
    mixed = B.RaggedBatch(enc.words, enc.word_offsets, enc.n_words, enc.status, enc.config, None, swapped, coder)
    dec, status = decode(mixed, d_off, d_probs)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_decode_categorical_ragged_kernel<jump>"
    st = status.cpu().tolist()
    for s in range(len(lengths)):
        if s in (2, 3, 8):
            assert st[s] == INVALID, (s, st)
        else:
            assert st[s] == OK and torch.equal(dec[off[s]: off[s + 1]], d_sym[off[s]: off[s + 1]]), (s, st)


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("coder", CODERS)
def test_symbol_ranges_are_bounded_by_n_total(B, O, coder, every):
    """the C entry points (slabs of `stride` words, d_word_offsets = NULL) with sym_offsets that name rows the matrix does not have
    (INVALID_DATA) or run backwards (CAPACITY): such a stream codes nothing, the streams around it are their oracle coders', and no
    symbol outside a stream's own is written"""
    import ctypes as C
    from constriction_amd import _native as N
    cfg, k = (32, 64, 24), 5
    key, (sym, probs, off, _) = batch(O, "bounds", [40, 30, 50], k, "f64", cfg[2])
    want = words_of(O, key, coder, cfg)
    n_total = int(off[-1])
    assert n_total == 120
    # streams: rows 0..40 and 40..70 (the oracle's streams 0 and 1), 70..123 (three rows too many), an empty one out there, one that
    # runs backwards, and rows 118..120 (which no chunk of the stream in front of them can reach: its last one is refused whole)
    sym_off = np.array([0, 40, 70, 123, 123, 118, 120], dtype=np.int64)
    expect = [OK, OK, INVALID, OK, CAPACITY, OK]
    n, stride = 6, 64
    chunks = [3, 2, 4, 0, 0, 1]
    n_chunks = sum(chunks) + 2
    d_sym, d_probs, d_off, chunk_off = dev(sym), dev(probs), dev(sym_off), dev(offsets_of(chunks))
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
    words, n_words, status = torch.full((n * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), z(n, torch.int32), z(n, torch.int32)
    table = [z(n_chunks, torch.int32)] + [z(n_chunks, torch.int64) for _ in range(1 if coder == "ans" else 2)]
    p = lambda t: C.c_void_p(t.data_ptr())
    L = N.lib()
    name = f"cst_{coder}_encode_categorical_ragged" + ("_jump" if every else "")
    tail = (every, p(chunk_off), *(p(t) for t in table)) if every else ()
    N.check(getattr(L, name)(N.CoderConfig(*cfg), p(d_sym), p(d_probs), 8, k, n_total, p(d_off), n, None, p(words), None, stride, p(n_words),
                             *tail, p(status), None), name)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == expect
    w, nw = words.cpu().numpy().view(np.uint32), n_words.cpu().numpy()
    for s, ww in ((0, want[0]), (1, want[1])):
        assert nw[s] == len(ww) and w[s * stride: s * stride + nw[s]].tolist() == ww.tolist(), s
    assert nw[2] == 0 and nw[3] == 0 and nw[4] == 0 and nw[5] > 0
    for s in range(n):
        assert (w[s * stride + nw[s]: (s + 1) * stride] == 0x5A5A5A5A).all(), s
    out = torch.full((n_total,), -7, dtype=torch.int32, device="cuda")
    status.fill_(-1)
    name = f"cst_{coder}_decode_categorical_ragged" + ("_jump" if every else "")
    if every:
        scratch = torch.empty(L.cst_persymbol_ragged_jump_scratch_bytes(n_chunks), dtype=torch.uint8, device="cuda")
        tail = (every, p(chunk_off), n_chunks, *(p(t) for t in table), p(scratch))
    else:
        tail = (None,)
    N.check(getattr(L, name)(N.CoderConfig(*cfg), p(words), None, stride, words.numel(), p(n_words), p(d_probs), 8, k, n_total, p(out), p(d_off), n,
                             *tail, p(status), None), name)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    if every:
        # (a chunk of stream 2 that lies inside the matrix is decoded from no words, whatever that gives; the one that does not is refused)
        assert st[2] != OK and st[:2] + st[3:] == expect[:2] + expect[3:], st
    else:
        assert st == expect
        assert (out[70:118] == -7).all()
    assert torch.equal(out[:70], d_sym[:70]) and torch.equal(out[118:], d_sym[118:])


def test_a_rectangular_batch_through_the_ragged_calls(B):
    """64 streams x 33 symbols, K = 65: the words of ans_encode_categorical for the same matrix (two GPU calls that must agree; each
    has its own oracle test)"""
    n_streams, n_per, k = 64, 33, CHUNK + 1
    sym, probs = workload([n_per] * n_streams, k, np.float32, 6433)
    d_sym, d_probs = dev(sym), dev(probs)
    d_off = dev(offsets_of([n_per] * n_streams))
    rect = B.ans_encode_categorical(d_sym.view(n_streams, n_per), d_probs.view(n_streams, n_per, k))
    enc = B.ans_encode_categorical_ragged(d_sym, d_off, d_probs)
    torch.cuda.synchronize()
    words, n_words, status = rect.to_numpy()
    assert (status == 0).all()
    assert_all_ok(enc.status)
    got, n = batch_streams(enc)
    assert n.tolist() == n_words.tolist()
    for s in range(n_streams):
        assert got[s].tolist() == words[s, : n_words[s]].tolist(), s
    dec, st = B.ans_decode_categorical_ragged(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert_all_ok(st)
    assert torch.equal(dec, d_sym)


def test_arguments(B):
    probs, sym, off = torch.ones(8, 5, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), dev(np.array([0, 3, 8], dtype=np.int64))
    with pytest.raises(ValueError, match="shape"):
        B.ans_encode_categorical_ragged(sym, off, probs[:7])
    with pytest.raises(ValueError, match="2-d"):
        B.range_encode_categorical_ragged(sym, off, probs.view(2, 4, 5))
    with pytest.raises(TypeError):
        B.ans_encode_categorical_ragged(sym, off, probs.half())
    with pytest.raises(ValueError, match="K"):
        B.ans_encode_categorical_ragged(sym, off, probs[:, :1])
    enc = B.ans_encode_categorical_ragged(sym, off, probs)
    with pytest.raises(ValueError, match="number of streams"):
        B.ans_decode_categorical_ragged(enc, dev(np.array([0, 3, 5, 8], dtype=np.int64)), probs)
    with pytest.raises(ValueError, match="coder"):
        B.range_decode_categorical_ragged(enc, off, probs)
    # no streams, and streams without symbols: nothing to code, CST_STREAM_OK
    none = B.range_encode_categorical_ragged(sym[:0], off[:1], probs[:0])
    assert none.n_words.numel() == 0
    empty = B.range_encode_categorical_ragged(sym[:0], torch.zeros(4, dtype=torch.int64, device="cuda"), probs[:0], jump_every=16)
    dec, st = B.range_decode_categorical_ragged(empty, torch.zeros(4, dtype=torch.int64, device="cuda"), probs[:0])
    torch.cuda.synchronize()
    assert empty.status.cpu().tolist() == [OK] * 3 and empty.n_words.cpu().tolist() == [0] * 3 and st.cpu().tolist() == [OK] * 3 and dec.numel() == 0
