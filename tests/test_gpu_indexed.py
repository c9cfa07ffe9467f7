"""GPU tests of indexed table coding (csrc/cst_indexed.hip; batched.TableSet, batched.{ans,range}_{encode,decode}_indexed): every
symbol is coded with the table its index names, out of K tables that share a support and a precision.

Every expected word, state and symbol comes from the CPU oracle: one oracle coder per stream, fed the per-symbol model list
[TableModel(cdfs[k], lo, P) for k in indices[s]].  No GPU result is the reference for another (the comparison with the shared-table
calls below stands beside the oracle's words, not in their place).  Tables: oracle-built leaky Gaussians from needle-thin (std 0.05:
one symbol holds 2^P - (n - 1), every other 1) to wider than the support, and handmade rows whose mass sits in different places."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KERNELS = {(c, d): f"{c}_{d}_indexed_kernel" for c in ("ans", "range") for d in ("encode", "decode")}
# (n_streams, n_per_stream, K, n_symbols, P, tables): n_streams {1, 63, 64, 65, 257}, n_per_stream {1, 31, 32, 33, 100}, K {1, 2, 64, 256},
# n_symbols {2, 64, 255} and P {8, 12, 16, 17, 24} all appear; at most 25 700 symbols a case
CASES = [(1, 100, 1, 2, 8, "hand"), (63, 31, 2, 64, 12, "gauss"), (64, 32, 64, 255, 16, "gauss"), (65, 33, 256, 64, 16, "hand"),
         (257, 100, 64, 255, 24, "gauss"), (65, 1, 64, 255, 17, "gauss"), (64, 100, 2, 2, 24, "hand")]
IDS = ["%dx%d-K%d-n%d-P%d-%s" % c for c in CASES]
INDEX_DTYPES = {"u8": np.uint8, "i32": np.int32}


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_cdfs(O, K, n, P, kind):
    lo = -(n // 2)
    hi = lo + n - 1
    if kind == "gauss":         # std from needle-thin to four times the support, means across it and beyond its ends
        stds = np.concatenate([[0.05], np.geomspace(0.11, 4.0 * n, K - 1)]) if K > 1 else np.array([0.05])
        means = np.linspace(lo - 2.0, hi + 2.0, K) if K > 1 else np.array([0.3])
        means[0] = 0.3
        return lo, np.stack([O.GaussianModel(lo, hi, m, s, P).cdf_table() for m, s in zip(means, stds)])
    rows = np.zeros((K, n + 1), dtype=np.uint32)
    total = 1 << P
    for r in range(K):          # the mass of row r: all on symbol r % n / split between the ends / flat / a ramp
        w = np.ones(n, dtype=np.int64)
        rest = total - n
        if r % 4 == 0:
            w[r % n] += rest
        elif r % 4 == 1:
            w[0] += rest // 2
            w[n - 1] += rest - rest // 2
        elif r % 4 == 2:
            w += rest // n
            w[(r // 4) % n] += rest - (rest // n) * n
        else:
            ramp = np.arange(1, n + 1, dtype=np.int64)[:: 1 if r % 8 == 3 else -1]
            add = rest * ramp // ramp.sum()
            w += add
            w[(r // 8) % n] += rest - add.sum()
        rows[r, 1:] = np.cumsum(w)
    return lo, rows


def make_batch(n_streams, n_per, K, n, P, lo, cdfs, seed):
    """indices: runs of one value / a change at every position / random, by stream, with 0 and K - 1 present; symbols: half uniform over
    the support, half drawn from their own table, and in front of every stream the first, last, most and least probable symbol of the
    row its index names (one of the four, by stream, where a stream has a single symbol)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, K, (n_streams, n_per))
    t = np.arange(n_per)
    for s in range(n_streams):
        if s % 3 == 0:
            idx[s] = np.repeat(rng.integers(0, K, n_per // 5 + 1), 5)[:n_per]
        elif s % 3 == 1:
            idx[s] = (rng.integers(0, K) + t * (1 + s % max(K - 1, 1))) % K
    idx[0, 0], idx[-1, -1] = 0, K - 1
    if n_streams > 2:
        idx[1, 0], idx[2, -1] = K - 1, 0
    q = rng.integers(0, 1 << P, (n_streams, n_per))
    drawn = np.empty((n_streams, n_per), dtype=np.int64)
    for k in range(K):
        m = idx == k
        drawn[m] = np.searchsorted(cdfs[k, :n], q[m], side="right") - 1
    sym = np.where(rng.random((n_streams, n_per)) < 0.5, rng.integers(0, n, (n_streams, n_per)), drawn)
    prob = np.diff(cdfs.astype(np.int64), axis=1)
    special = [lambda k: 0, lambda k: n - 1, lambda k: int(prob[k].argmax()), lambda k: int(prob[k].argmin())]
    for s in range(n_streams):
        for j in range(4):
            if n_per >= 4:
                sym[s, j] = special[j](idx[s, j])
            elif j == s % 4:
                sym[s, 0] = special[j](idx[s, 0])
    return (sym + lo).astype(np.int32), idx.astype(np.int32)


def oracle_encode(O, coder, P, sym, models):
    """(words, state in front of the seal): the ANS state, or (words emitted, (lower, range))"""
    if coder == "ans":
        c = O.AnsCoder()
        c.encode_reverse(sym, models, P)
        return c.get_compressed(), c.pos()[1]
    c = O.RangeEncoder()
    c.encode(sym, models, P)
    pos = c.pos()
    return c.get_compressed(), pos


_cache = {}


def workload(O, case):
    if case not in _cache:
        n_streams, n_per, K, n, P, kind = case
        lo, cdfs = make_cdfs(O, K, n, P, kind)
        sym, idx = make_batch(n_streams, n_per, K, n, P, lo, cdfs, sum(case[:5]))
        _cache[case] = (lo, cdfs, sym, idx, [O.TableModel(cdfs[k], lo, P) for k in range(K)])
    return _cache[case]


def expected(O, case, coder):
    if (case, coder) not in _cache:
        lo, cdfs, sym, idx, tm = workload(O, case)
        _cache[(case, coder)] = [oracle_encode(O, coder, case[4], sym[s], [tm[k] for k in idx[s]]) for s in range(case[0])]
    return _cache[(case, coder)]


def table_set(B, case, lo, cdfs):
    if ("set", case) not in _cache:
        _cache[("set", case)] = B.TableSet.from_cdfs(cdfs, lo, case[4])
    return _cache[("set", case)]


def native_encode(B, coder, tables, d_sym, d_idx, stride):
    """the C entry point with its optional state output: (EncodedBatch, state tensor)"""
    from constriction_amd import _native as N
    n_streams, n_per = d_sym.shape
    out = B._new_batch(n_streams, stride, d_sym.device, (32, 64, tables.precision))
    state = torch.zeros((n_streams, 5 if coder == "range" else 1), dtype=torch.int64, device=d_sym.device)
    fn = getattr(N.lib(), f"cst_{coder}_encode_indexed_batch")
    N.check(fn(tables._h, N.CoderConfig(32, 64, tables.precision), B._ptr(d_sym), B._ptr(d_idx), d_idx.element_size(), n_streams, n_per, 0,
               B._ptr(out.words), stride, B._ptr(out.n_words), B._ptr(state), B._ptr(out.status), 0, B._stream_ptr()))
    torch.cuda.synchronize()
    assert B.last_kernel() == KERNELS[(coder, "encode")]
    return out, state.cpu().numpy().view(np.uint64)


def native_decode(B, coder, tables, words, offsets, stride, capacity, n_words, d_idx, out=None):
    """... and the decoders': (symbols, status, state [n_streams, 1 or 5] (ANS: the state; range: lower, range, point, -, position),
    n_words_out (ANS))"""
    from constriction_amd import _native as N
    n_streams, n_per = d_idx.shape
    out = torch.empty((n_streams, n_per), dtype=torch.int32, device=d_idx.device) if out is None else out
    status = torch.empty(n_streams, dtype=torch.int32, device=d_idx.device)
    state = torch.zeros((n_streams, 5 if coder == "range" else 1), dtype=torch.int64, device=d_idx.device)
    left = torch.zeros(n_streams, dtype=torch.int32, device=d_idx.device)
    args = [tables._h, N.CoderConfig(32, 64, tables.precision), B._ptr(words), B._ptr(offsets), stride, capacity, B._ptr(n_words), B._ptr(d_idx),
            d_idx.element_size(), B._ptr(out), n_streams, n_per, 0, B._ptr(state)]
    if coder == "ans":
        args.append(B._ptr(left))
    N.check(getattr(N.lib(), f"cst_{coder}_decode_indexed_batch")(*args, B._ptr(status), 0, B._stream_ptr()))
    torch.cuda.synchronize()
    assert B.last_kernel() == KERNELS[(coder, "decode")]
    return out.cpu().numpy(), status.cpu().numpy(), state.cpu().numpy().view(np.uint64), left.cpu().numpy()


def slabs_of(streams, stride):
    words = np.zeros((len(streams), stride), dtype=np.uint32)
    for s, w in enumerate(streams):
        words[s, : len(w)] = w
    return dev(words.view(np.int32)), dev(np.array([len(w) for w in streams], dtype=np.int32))


@pytest.mark.parametrize("dtype", list(INDEX_DTYPES))
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_words_states_and_symbols_are_the_oracles(B, O, case, coder, dtype):
    n_streams, n_per, K, n, P, _ = case
    lo, cdfs, sym, idx, tm = workload(O, case)
    want = expected(O, case, coder)
    tables = table_set(B, case, lo, cdfs)
    assert (tables.precision, tables.min_symbol, tables.n_symbols, tables.n_tables) == (P, lo, n, K) and np.array_equal(tables.cdfs(), cdfs)
    d_sym, d_idx = dev(sym), dev(idx.astype(INDEX_DTYPES[dtype]))
    stride = (B.max_words if coder == "ans" else B.range_max_words)(n_per, (32, 64, P))
    # 1. encode: words, counts, the state in front of the seal
    enc, state = native_encode(B, coder, tables, d_sym, d_idx, stride)
    words, n_words, status = enc.to_numpy()
    assert (status == 0).all()
    assert n_words.tolist() == [len(w) for w, _ in want]
    for s, (w, st) in enumerate(want):
        assert words[s, : n_words[s]].tolist() == w.tolist(), f"stream {s}"
        if coder == "ans":
            assert int(state[s, 0]) == st, f"stream {s}"
        else:
            assert (int(state[s, 0]), int(state[s, 1])) == st[1], f"stream {s}"
    # 2. decode of the ORACLE's words: the symbols, and what is left of the coder
    d_words, d_n = slabs_of([w for w, _ in want], stride)
    got, dstatus, dstate, left = native_decode(B, coder, tables, d_words, None, stride, d_words.numel(), d_n, d_idx)
    assert (dstatus == 0).all() and np.array_equal(got, sym)
    for s, (w, st) in enumerate(want):
        if coder == "ans":
            c = O.AnsCoder(w)
            assert c.decode([tm[k] for k in idx[s]], P=P).tolist() == sym[s].tolist()
            assert (int(left[s]), int(dstate[s, 0])) == c.pos(), f"stream {s}"
        else:       # a decoder that has read every symbol stands where the encoder stood in front of its seal, two words ahead
            assert (int(dstate[s, 0]), int(dstate[s, 1])) == st[1], f"stream {s}"
            assert int(dstate[s, 4]) == min(st[0] + 2, len(w)), f"stream {s}"


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_round_trip_through_the_python_layer_compact_and_offsets(B, O, case, coder):
    n_streams, n_per, K, n, P, _ = case
    lo, cdfs, sym, idx, _ = workload(O, case)
    want = expected(O, case, coder)
    tables = table_set(B, case, lo, cdfs)
    encode, decode = getattr(B, f"{coder}_encode_indexed"), getattr(B, f"{coder}_decode_indexed")
    for dtype in INDEX_DTYPES.values():
        d_sym, d_idx = dev(sym), dev(idx.astype(dtype))
        enc = encode(d_sym, d_idx, tables, (32, 64, P))
        torch.cuda.synchronize()
        assert B.last_kernel() == KERNELS[(coder, "encode")] and enc.jump is None
        assert [enc.stream(s).tolist() for s in range(n_streams)] == [w.tolist() for w, _ in want]
        dec, st = decode(enc, d_idx, tables, n_per)
        torch.cuda.synchronize()
        assert B.last_kernel() == KERNELS[(coder, "decode")]
        assert (st.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
        packed, offsets = B.compact(enc)
        assert packed[: int(offsets[-1])].cpu().numpy().view(np.uint32).tolist() == np.concatenate([w for w, _ in want]).tolist()
        dec, st = decode((packed, enc.n_words), d_idx, tables, n_per, offsets=offsets)
        torch.cuda.synchronize()
        assert B.last_kernel() == KERNELS[(coder, "decode")]
        assert (st.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    if coder == "ans":          # the words the other way round and back are the same batch
        back = B.reverse_words(B.reverse_words(enc))
        assert [back.stream(s).tolist() for s in range(n_streams)] == [w.tolist() for w, _ in want]


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_maximum_word_rate_fits_max_words(B, O, coder):
    """every coded symbol has probability 1 at P = 24 (24 bits each: three words per four symbols): a slab of cst_*_max_words suffices"""
    n_streams, n_per, K, n, P = 65, 100, 2, 64, 24
    lo = -(n // 2)
    cdfs = np.stack([O.GaussianModel(lo, lo + n - 1, m, 0.05, P).cdf_table() for m in (-3.0, 7.0)])
    prob = np.diff(cdfs.astype(np.int64), axis=1)
    assert sorted(prob[0].tolist()) == [1] * (n - 1) + [(1 << P) - (n - 1)]
    rng = np.random.default_rng(24)
    idx = rng.integers(0, K, (n_streams, n_per)).astype(np.int32)
    sym = rng.integers(0, n, (n_streams, n_per))
    sym = np.where(prob[idx, sym] == 1, sym, (sym + 1) % n)
    assert (prob[idx, sym] == 1).all()
    sym = (sym + lo).astype(np.int32)
    tm = [O.TableModel(cdfs[k], lo, P) for k in range(K)]
    want = [oracle_encode(O, coder, P, sym[s], [tm[k] for k in idx[s]])[0] for s in range(n_streams)]
    stride = (B.max_words if coder == "ans" else B.range_max_words)(n_per, (32, 64, P))
    assert max(len(w) for w in want) >= n_per * P // 32 and max(len(w) for w in want) <= stride
    tables = B.TableSet.from_cdfs(cdfs, lo, P)
    enc = getattr(B, f"{coder}_encode_indexed")(dev(sym), dev(idx.astype(np.uint8)), tables, (32, 64, P))
    torch.cuda.synchronize()
    assert enc.stride == stride and (enc.status.cpu().numpy() == 0).all()
    assert [enc.stream(s).tolist() for s in range(n_streams)] == [w.tolist() for w in want]
    dec, st = getattr(B, f"{coder}_decode_indexed")(enc, dev(idx.astype(np.uint8)), tables, n_per)
    assert (st.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_one_index_everywhere_is_the_shared_table_call(B, O, case, coder):
    """on top of the oracle, not in its place: with every index equal to k the words are those of the shared-table coder over cdfs[k]"""
    n_streams, n_per, K, n, P, _ = case
    lo, cdfs, sym, _, tm = workload(O, case)
    tables = table_set(B, case, lo, cdfs)
    for k in (0, K - 1):
        d_sym = dev(sym)
        enc = getattr(B, f"{coder}_encode_indexed")(d_sym, dev(np.full(sym.shape, k, dtype=np.uint8)), tables, (32, 64, P))
        ref = getattr(B, f"{coder}_encode")(d_sym, B.Model.from_cdf(cdfs[k], lo, P), (32, 64, P), jump_points=0)
        torch.cuda.synchronize()
        assert np.array_equal(enc.n_words.cpu().numpy(), ref.n_words.cpu().numpy())
        for s in range(n_streams):
            assert enc.stream(s).tolist() == ref.stream(s).tolist(), (k, s)
        assert enc.stream(0).tolist() == oracle_encode(O, coder, P, sym[0], tm[k])[0].tolist()


FAIL_CASE = (65, 33, 2, 64, 12, "gauss")


def check_others(want, enc, victim):
    words, n_words, status = enc.to_numpy()
    for s, (w, _) in enumerate(want):
        if s != victim:
            assert status[s] == 0 and words[s, : n_words[s]].tolist() == w.tolist(), f"stream {s}"


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_an_impossible_symbol_or_index_fails_its_stream_alone(B, O, coder):
    from constriction_amd import _native as N
    n_streams, n_per, K, n, P, _ = FAIL_CASE
    lo, cdfs, sym, idx, tm = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    encode, decode = getattr(B, f"{coder}_encode_indexed"), getattr(B, f"{coder}_decode_indexed")
    victim = 40
    for t in (0, n_per // 2, n_per - 1):
        # 6. a symbol outside the support, on either side
        for value in (lo + n, lo - 1, 2**31 - 1, -2**31):
            bad = sym.copy()
            bad[victim, t] = value
            enc = encode(dev(bad), dev(idx.astype(np.uint8)), tables, (32, 64, P))
            assert enc.status[victim].item() == N.STREAM_IMPOSSIBLE_SYMBOL and enc.n_words[victim].item() == 0
            check_others(want, enc, victim)
        # 7. an index that names no table: the encoder's impossible symbol, the decoder's invalid data
        for dtype, values in ((np.uint8, (K, 255)), (np.int32, (K, -1, 2**31 - 1, 256))):
            for value in values:
                bad = idx.astype(dtype)
                bad[victim, t] = value
                enc = encode(dev(sym), dev(bad), tables, (32, 64, P))
                assert enc.status[victim].item() == N.STREAM_IMPOSSIBLE_SYMBOL and enc.n_words[victim].item() == 0
                check_others(want, enc, victim)
                d_words, d_n = slabs_of([w for w, _ in want], 64)
                dec, st = decode((d_words, d_n), dev(bad), tables, n_per)
                st, dec = st.cpu().numpy(), dec.cpu().numpy()
                assert st[victim] == N.STREAM_INVALID_DATA and (np.delete(st, victim) == 0).all()
                assert np.array_equal(np.delete(dec, victim, axis=0), np.delete(sym, victim, axis=0))
                assert np.array_equal(dec[victim, :t], sym[victim, :t])          # (what came before the index is still right)


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_a_slab_one_word_short_is_capacity_for_that_stream_alone(B, O, coder):
    from constriction_amd import _native as N
    n_streams, n_per, K, n, P, _ = FAIL_CASE
    lo, cdfs, sym, idx, _ = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    lengths = np.array([len(w) for w, _ in want])
    stride = int(lengths.max()) - 1
    guard = torch.full((n_streams + 1, stride), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = B.EncodedBatch(guard[:n_streams], torch.empty(n_streams, dtype=torch.int32, device="cuda"),
                         torch.empty(n_streams, dtype=torch.int32, device="cuda"), (32, 64, P))
    enc = getattr(B, f"{coder}_encode_indexed")(dev(sym), dev(idx), tables, (32, 64, P), out=out)
    words, n_words, status = enc.to_numpy()
    assert (lengths > stride).any() and not (lengths > stride).all()
    for s, (w, _) in enumerate(want):
        if len(w) > stride:
            assert status[s] == N.STREAM_CAPACITY and n_words[s] == 0
        else:
            assert status[s] == 0 and words[s, : n_words[s]].tolist() == w.tolist(), f"stream {s}"
    assert (guard[n_streams].cpu().numpy() == 0x5A5A5A5A).all()         # nothing behind the last slab


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_decoding_short_counts_stays_inside_the_words_present(B, O, coder):
    """n_words one shorter than written, packed back to back with words_capacity = the words present, in an allocation that goes on
    with a guard pattern: every stream decodes as the oracle decodes the shortened words, and nothing around them changes"""
    from constriction_amd import _native as N
    n_streams, n_per, K, n, P, _ = FAIL_CASE
    lo, cdfs, sym, idx, tm = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    short = [w[:-1] for w, _ in want]
    total = sum(len(w) for w in short)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in short])]).astype(np.int64)
    buf = np.full(total + 256, 0xDEADBEEF, dtype=np.uint32)
    buf[:total] = np.concatenate(short)
    d_buf = dev(buf.view(np.int32))
    d_idx = dev(idx.astype(np.uint8))
    room = torch.full((n_streams + 2, n_per), -77, dtype=torch.int32, device="cuda")
    got, status, _, _ = native_decode(B, coder, tables, d_buf, dev(offsets), 0, total, dev(np.array([len(w) for w in short], dtype=np.int32)),
                                      d_idx, out=room[1:-1])
    assert np.array_equal(d_buf.cpu().numpy().view(np.uint32), buf)
    assert (room[0].cpu().numpy() == -77).all() and (room[-1].cpu().numpy() == -77).all()
    for s in range(n_streams):
        models = [tm[k] for k in idx[s]]
        try:
            ref = (O.AnsCoder(short[s]) if coder == "ans" else O.RangeDecoder(short[s])).decode(models, P=P)
        except (ValueError, AssertionError):            # a zero last word / a quantile beyond the model
            assert status[s] == N.STREAM_INVALID_DATA, f"stream {s}"
            continue
        assert status[s] == 0 and got[s].tolist() == ref.tolist(), f"stream {s}"
    # a count or an offset that leaves the buffer is an empty stream with INVALID_DATA, as in the plain decoders
    n_bad = np.array([len(w) for w in short], dtype=np.int32)
    n_bad[7] = total + 1
    _, status, _, _ = native_decode(B, coder, tables, d_buf, dev(offsets), 0, total, dev(n_bad), d_idx)
    assert status[7] == N.STREAM_INVALID_DATA
