"""GPU tests of the ragged per-symbol Categorical(perfect=True) calls: batched.{ans,range}_{encode,decode}_categorical_perfect_ragged,
their `jump_every`, and the kernels behind them (the ragged mode of categorical_perfect_kernel and decode_rows_piece_ragged_kernel,
csrc/cst_persymbol_categorical_ragged.hip).

Every expected word, count, status and jump table comes from the CPU oracle alone: one tabulated model per symbol over
oracle.categorical_perfect_cdf of the row as f64, fed to one oracle coder per stream, and the same coder coded chunk by chunk for the
tables (tests/persymbol_jump_oracle.py).  No GPU result is the reference for another, except where a test says that two GPU calls must
agree.  The batches and their oracle results are those of tests/categorical_perfect_ragged_rows.py: built once per key, shared, never
modified; tests/test_categorical_perfect_ragged_cpu.py checks on the CPU that every row of them quantises."""
import ctypes as C

import numpy as np
import pytest

import categorical_perfect_ragged_rows as R
from categorical_perfect_ragged_rows import (CAPACITY, CODERS, CONFIGS, IMPOSSIBLE, INVALID, LOCAL_LENGTHS, MODELS, OK, PARITY_LENGTHS, cfg_id,
                                             model_id, offsets_of)

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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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
    return getattr(B, f"{coder}_encode_categorical_perfect_ragged"), getattr(B, f"{coder}_decode_categorical_perfect_ragged")


def assert_all_ok(status):
    assert (status.cpu().numpy() == OK).all(), status.cpu().tolist()


def encode_name(coder, jump=False):
    return f"{coder}_encode_categorical_perfect_ragged_two_pass" + ("<jump>" if jump else "")


def decode_name(coder, jump=False):
    return f"{coder}_decode_categorical_perfect_ragged_by_rows" + ("<jump>" if jump else "")


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("model", MODELS, ids=model_id)
def test_parity(B, O, model, coder, cfg):
    """70 streams of 0 .. 300 symbols, with and without a schedule: words, counts and statuses of every stream are its oracle coder's,
    decoding returns the input"""
    k, dtype = model
    lengths = PARITY_LENGTHS
    assert len(lengths) == 70 and sum(lengths) == 2955
    key, (sym, probs, off, _) = R.batch(O, "parity", lengths, k, dtype, cfg[2])
    want = R.words_of(O, key, coder, cfg)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    for order in (None, B.ragged_order(dev(np.asarray(lengths, dtype=np.int64)))):
        enc = encode(d_sym, d_off, d_probs, cfg, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == encode_name(coder)
        assert enc.coder == coder and enc.jump is None and (enc.order is None) == (order is None)
        assert_all_ok(enc.status)
        got, n_words = batch_streams(enc)
        assert_streams_equal(got, n_words, want)
        dec, status = decode(enc, d_off, d_probs, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == decode_name(coder)
        assert_all_ok(status)
        assert torch.equal(dec, d_sym)
    # "auto": the encoder's schedule, or none below RAGGED_BALANCE_FROM streams
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)


@pytest.mark.parametrize("every", [0, 48])
@pytest.mark.parametrize("coder", CODERS)
def test_the_largest_model(B, O, coder, every):
    """K = 1024, every slot of the largest quantiser, float32, P = 24: 9 streams of 0 .. 500 symbols, plain and with jump points"""
    cfg, k = (32, 64, 24), 1024
    lengths = LOCAL_LENGTHS
    key, (sym, probs, off, _) = R.batch(O, "local", lengths, k, "f32", cfg[2])
    want = R.words_of(O, key, coder, cfg)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == encode_name(coder, bool(every))
    assert_all_ok(enc.status)
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert B.last_kernel() == decode_name(coder, bool(every))
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)


@pytest.mark.parametrize("every", [16, 48])
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("model", MODELS, ids=model_id)
def test_jump_points(B, O, model, coder, cfg, every):
    """the parity batch with a jump point every 16 / 48 symbols (210 / 95 table entries)"""
    k, dtype = model
    lengths = PARITY_LENGTHS
    key, (sym, probs, off, _) = R.batch(O, "parity", lengths, k, dtype, cfg[2])
    want = R.tables_of(O, key, coder, cfg, every)
    chunks = [-(-n // every) for n in lengths]
    assert sum(chunks) == {16: 210, 48: 95}[every]
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == encode_name(coder, True)
    assert_all_ok(enc.status)
    # the words are the oracle's, coded chunk by chunk and in one go, and the plain call's: the same slabs, counts and statuses
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, [w for w, _ in want])
    assert_streams_equal(got, n_words, R.words_of(O, key, coder, cfg))
    plain = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=0)
    torch.cuda.synchronize()
    assert B.last_kernel() == encode_name(coder) and plain.jump is None
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
    assert B.last_kernel() == decode_name(coder, True)
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)
    # ... and a schedule handed in decodes whole streams
    dec, status = decode(enc, d_off, d_probs, order=torch.arange(len(lengths), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert B.last_kernel() == decode_name(coder)
    assert_all_ok(status)
    assert torch.equal(dec, d_sym)


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("model", [(5, "f32"), (65, "f32")], ids=model_id)
def test_pieces_and_groups(B, O, knob, model, coder, every):
    """CST_PERFECT_RAGGED_BUDGET (words of tabulated rows per step): one group in pieces of 7 positions -- piece ends fall inside
    streams, and units finish in different pieces -- and groups of 40 units (40 + 30 streams) in pieces of one position.  The symbols
    and statuses are the default budget's, and the input the oracle's words were made from."""
    k, dtype = model
    cfg, lengths = (32, 64, 24), PARITY_LENGTHS
    key, (sym, probs, off, _) = R.batch(O, "parity", lengths, k, dtype, cfg[2])
    want = R.words_of(O, key, coder, cfg)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=every)
    torch.cuda.synchronize()
    assert_all_ok(enc.status)
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    # the units of the decode: streams, or the entries of the table (an upper bound of the chunks, the rest empty)
    n_units = enc.jump.pos.numel() if every else len(lengths)
    bound = every if every else max(lengths)
    assert n_units > 40 and bound > 7
    default, default_status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert B.last_kernel() == decode_name(coder, bool(every))
    assert_all_ok(default_status)
    assert torch.equal(default, d_sym)
    for budget in (7 * n_units * (k + 1), 40 * (k + 1)):
        knob(CST_PERFECT_RAGGED_BUDGET=budget)
        out = torch.full_like(d_sym, -7)
        dec, status = decode(enc, d_off, d_probs, out=out)
        torch.cuda.synchronize()
        assert B.last_kernel() == decode_name(coder, bool(every))
        assert torch.equal(status, default_status), budget
        assert torch.equal(dec, d_sym) and torch.equal(dec, default), budget


def _spoil(case, sym, probs, off, k):
    """one failure in one stream of LOCAL_LENGTHS: (stream, whether the encoder sees it)"""
    if case == "negative":
        probs[off[2] + 100, 7] = -probs[off[2] + 100, 7] - 1e-3
        return 2, True
    if case == "all_zero":
        probs[off[5] + 149, :] = 0.0
        return 5, True
    if case == "nan":
        probs[off[7] + 3, k - 1] = np.nan
        return 7, True
    if case == "symbol_k":
        sym[off[0] + 99] = k
        return 0, True
    assert case == "truncated"
    return 7, False


@pytest.mark.parametrize("every", [0, 48])
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("case", ["negative", "all_zero", "nan", "symbol_k", "truncated"])
def test_failures_stay_local(B, O, case, coder, every):
    """a bad row (code 1 of the quantiser), a symbol outside [0, K), or half of a stream's words withheld from the decoder: that stream
    alone reports it, every other stream's words are the oracle's and decode to their input.  Of a stream that the encoder flagged,
    only this is asserted of the decoder: whole streams meet a bad row again (a flagged stream's table is unspecified)."""
    cfg, k = (32, 64, 24), 65
    lengths = LOCAL_LENGTHS
    key, (sym, probs, off, _) = R.batch(O, "local", lengths, k, "f32", cfg[2])
    want = R.words_of(O, key, coder, cfg)
    sym, probs = sym.copy(), probs.copy()
    flagged, at_encode = _spoil(case, sym, probs, off, k)
    encode, decode = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [IMPOSSIBLE if at_encode and s == flagged else OK for s in range(len(lengths))]
    got, n_words = batch_streams(enc)
    if at_encode:
        assert n_words[flagged] == 0
        assert_streams_equal(got, n_words, want, skip=(flagged,))
    else:
        assert_streams_equal(got, n_words, want)
        cut = enc.n_words.clone()
        cut[flagged] = cut[flagged] // 2
        enc = B.RaggedBatch(enc.words, enc.word_offsets, cut, enc.status, enc.config, enc.order, enc.jump, coder)
    dec, status = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    if case in ("negative", "all_zero", "nan") and not every:
        assert st[flagged] == IMPOSSIBLE, st
    if case == "truncated" and every:
        assert st[flagged] == INVALID, st                      # (jump points that lie beyond the stream's words)
    for s in range(len(lengths)):
        if s != flagged:
            assert st[s] == OK and torch.equal(dec[off[s]: off[s + 1]], d_sym[off[s]: off[s + 1]]), (s, st)


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("coder", CODERS)
def test_symbol_ranges_are_bounded_by_n_total(B, O, coder, every):
    """the C entry points (slabs of `stride` words, d_word_offsets = NULL) with sym_offsets that name rows the matrix does not have
    (INVALID_DATA) or run backwards (CAPACITY): refusals judged before any address is formed -- such a stream codes nothing, the streams
    around it are their oracle coders', and no symbol outside a stream's own is written"""
    from constriction_amd import _native as N
    cfg, k = (32, 64, 24), 5
    key, (sym, probs, off, _) = R.batch(O, "bounds", [40, 30, 50], k, "f64", cfg[2])
    want = R.words_of(O, key, coder, cfg)
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
    name = f"cst_{coder}_encode_categorical_perfect_ragged" + ("_jump" if every else "")
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
    name = f"cst_{coder}_decode_categorical_perfect_ragged" + ("_jump" if every else "")
    head = (N.CoderConfig(*cfg), p(words), None, stride, words.numel(), p(n_words), p(d_probs), 8, k, n_total)
    if every:
        scratch = torch.empty(L.cst_persymbol_ragged_jump_scratch_bytes(n_chunks), dtype=torch.uint8, device="cuda")
        N.check(getattr(L, name)(*head, p(out), p(d_off), n, every, p(chunk_off), n_chunks, *(p(t) for t in table), p(scratch), p(status), None), name)
    else:
        N.check(getattr(L, name)(*head, 53, p(out), p(d_off), n, None, p(status), None), name)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    if every:
        # (a chunk of stream 2 that lies inside the matrix is decoded from no words, whatever that gives; the one that does not is refused)
        assert st[2] != OK and st[:2] + st[3:] == expect[:2] + expect[3:], st
    else:
        assert st == expect
        assert (out[70:118] == -7).all()
    assert torch.equal(out[:70], d_sym[:70]) and torch.equal(out[118:], d_sym[118:])


@pytest.mark.parametrize("coder", CODERS)
def test_max_len_below_the_longest_stream(B, O, coder):
    """the plain decoders through _native with max_len = 150 on streams of up to 500 symbols: the two streams longer than that (200 and
    500 symbols) report CAPACITY and nothing of theirs is written; the other streams, the one of exactly 150 symbols among them, decode"""
    from constriction_amd import _native as N
    cfg, k = (32, 64, 24), 65
    lengths = LOCAL_LENGTHS
    key, (sym, probs, off, _) = R.batch(O, "local", lengths, k, "f32", cfg[2])
    encode, _ = calls(B, coder)
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(off)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None)
    torch.cuda.synchronize()
    assert_all_ok(enc.status)
    p = lambda t: C.c_void_p(t.data_ptr())
    name = f"cst_{coder}_decode_categorical_perfect_ragged"
    for max_len, over in ((150, (2, 7)), (499, (7,)), (500, ())):
        out = torch.full_like(d_sym, -7)
        status = torch.full((len(lengths),), -1, dtype=torch.int32, device="cuda")
        N.check(getattr(N.lib(), name)(N.CoderConfig(*cfg), p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), p(d_probs), 4, k,
                                       len(sym), max_len, p(out), p(d_off), len(lengths), None, p(status), None), name)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [CAPACITY if s in over else OK for s in range(len(lengths))], max_len
        for s in range(len(lengths)):
            mine = out[off[s]: off[s + 1]]
            assert (mine == -7).all() if s in over else torch.equal(mine, d_sym[off[s]: off[s + 1]]), (max_len, s)


@pytest.mark.parametrize("coder", CODERS)
def test_a_rectangular_batch_through_the_ragged_calls(B, coder):
    """64 streams x 48 symbols, K = 65: the words of {ans,range}_encode_categorical(..., perfect=True) for the same matrix (two GPU
    calls that must agree; each has its own oracle test)"""
    n_streams, n_per, k = 64, 48, 65
    sym, probs = R.workload([n_per] * n_streams, k, np.float32, 6448)
    d_sym, d_probs = dev(sym), dev(probs)
    d_off = dev(offsets_of([n_per] * n_streams))
    encode, decode = calls(B, coder)
    rect = getattr(B, f"{coder}_encode_categorical")(d_sym.view(n_streams, n_per), d_probs.view(n_streams, n_per, k), perfect=True)
    enc = encode(d_sym, d_off, d_probs)
    torch.cuda.synchronize()
    words, n_words, status = rect.to_numpy()
    assert (status == 0).all()
    assert_all_ok(enc.status)
    got, n = batch_streams(enc)
    assert n.tolist() == n_words.tolist()
    for s in range(n_streams):
        assert got[s].tolist() == words[s, : n_words[s]].tolist(), s
    dec, st = decode(enc, d_off, d_probs)
    torch.cuda.synchronize()
    assert_all_ok(st)
    assert torch.equal(dec, d_sym)


def test_arguments(B):
    probs, sym, off = torch.ones(8, 5, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), dev(np.array([0, 3, 8], dtype=np.int64))
    with pytest.raises(ValueError, match="shape"):
        B.ans_encode_categorical_perfect_ragged(sym, off, probs[:7])
    with pytest.raises(ValueError, match="2-d"):
        B.range_encode_categorical_perfect_ragged(sym, off, probs.view(2, 4, 5))
    with pytest.raises(TypeError):
        B.ans_encode_categorical_perfect_ragged(sym, off, probs.half())
    with pytest.raises(ValueError, match="K"):
        B.ans_encode_categorical_perfect_ragged(sym, off, probs[:, :1])
    with pytest.raises(ValueError, match="K"):
        B.ans_encode_categorical_perfect_ragged(sym, off, torch.ones(8, 1025, device="cuda"))
    enc = B.ans_encode_categorical_perfect_ragged(sym, off, probs)
    with pytest.raises(ValueError, match="number of streams"):
        B.ans_decode_categorical_perfect_ragged(enc, dev(np.array([0, 3, 5, 8], dtype=np.int64)), probs)
    with pytest.raises(ValueError, match="coder"):
        B.range_decode_categorical_perfect_ragged(enc, off, probs)
    # no streams, and streams without symbols: nothing to code, CST_STREAM_OK
    none = B.range_encode_categorical_perfect_ragged(sym[:0], off[:1], probs[:0])
    assert none.n_words.numel() == 0
    for every in (0, 16):
        empty = B.range_encode_categorical_perfect_ragged(sym[:0], torch.zeros(4, dtype=torch.int64, device="cuda"), probs[:0], jump_every=every)
        dec, st = B.range_decode_categorical_perfect_ragged(empty, torch.zeros(4, dtype=torch.int64, device="cuda"), probs[:0])
        torch.cuda.synchronize()
        assert empty.status.cpu().tolist() == [OK] * 3 and empty.n_words.cpu().tolist() == [0] * 3 and st.cpu().tolist() == [OK] * 3
        assert dec.numel() == 0
