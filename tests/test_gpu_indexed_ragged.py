"""GPU tests of ragged indexed table coding (csrc/cst_indexed_ragged.hip; batched.{ans,range}_{encode,decode}_indexed_ragged, DESIGN.md
4.30): streams of different lengths, every symbol coded with the table its index names, plain and with jump points.

Every expected word, count, table entry and symbol comes from the CPU oracle: one oracle coder per stream, fed the model list
[TableModel(cdfs[k], lo, P) for k in indices[lo:hi]], coded chunk by chunk for the jump tables (tests/persymbol_jump_oracle.py).  No GPU
result is the reference for another; the comparison with the rectangular calls stands beside the oracle's words, not in their place.
Tables as tests/test_gpu_indexed.py makes them (make_cdfs), symbols and indices by that file's make_batch rules, stream by stream."""
import numpy as np
import pytest

from persymbol_jump_oracle import ans_table, range_table
from test_gpu_indexed import make_cdfs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, IMPOSSIBLE, CAPACITY, INVALID = 0, 1, 2, 3
# (n_streams, K, n_symbols, P, tables, jump interval): n_streams {1, 63, 64, 65, 257}, the (K, n, P) grid of tests/test_gpu_indexed.py
# (16- and 32-bit rows, one- and two-byte buckets), intervals {16, 32, 256}; each is run without jump points as well.  Under 10 000 symbols
CASES = [(1, 1, 2, 8, "hand", 16), (63, 2, 64, 12, "gauss", 32), (64, 64, 255, 16, "gauss", 256), (65, 256, 64, 16, "hand", 16),
         (257, 64, 255, 24, "gauss", 32), (65, 64, 255, 17, "gauss", 256)]
IDS = ["%dstreams-K%d-n%d-P%d-%s-I%d" % c for c in CASES]
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


def dev_indices(idx, dtype, shift=0):
    """the flat indices on the device; uint8 rows `shift` bytes into an allocation, so that the array itself starts at any byte"""
    a = np.ascontiguousarray(idx.astype(dtype))
    if dtype is not np.uint8:
        return dev(a)
    room = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
    room[shift: shift + a.size] = dev(a)
    return room[shift: shift + a.size]


def lengths_of(n_streams, every):
    """0, 1, 7 .. 33, I - 1, I, I + 1, 2 I, 3 I + 5 in turn, and one stream of about 700 symbols in a wave of short ones"""
    base = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, every - 1, every, every + 1, 2 * every, 3 * every + 5]
    if n_streams == 1:
        return [3 * every + 5]
    lengths = [base[(5 * s + s // 16) % 16] for s in range(n_streams)]
    lengths[min(20, n_streams - 1)] = 701
    return lengths


def make_ragged(lengths, K, n, P, lo, cdfs, seed):
    """tests/test_gpu_indexed.py's make_batch, stream by stream: indices in runs / changing at every position / random, with 0 and K - 1
    present; symbols half uniform, half drawn from their table, and in front of every stream the first, last, most and least probable
    symbol of the row its index names"""
    rng = np.random.default_rng(seed)
    prob = np.diff(cdfs.astype(np.int64), axis=1)
    special = [lambda k: 0, lambda k: n - 1, lambda k: int(prob[k].argmax()), lambda k: int(prob[k].argmin())]
    syms, idxs = [], []
    for s, length in enumerate(lengths):
        t = np.arange(length)
        if s % 3 == 0:
            idx = np.repeat(rng.integers(0, K, length // 5 + 1), 5)[:length]
        elif s % 3 == 1:
            idx = (rng.integers(0, K) + t * (1 + s % max(K - 1, 1))) % K
        else:
            idx = rng.integers(0, K, length)
        if length:
            idx[0 if s % 2 else -1] = (0, K - 1)[(s // 2) % 2]
        q = rng.integers(0, 1 << P, length)
        drawn = np.array([np.searchsorted(cdfs[k, :n], x, side="right") - 1 for k, x in zip(idx, q)], dtype=np.int64).reshape(length)
        sym = np.where(rng.random(length) < 0.5, rng.integers(0, n, length), drawn)
        for j in range(min(4, length)):
            sym[j] = special[(j + s) % 4 if length < 4 else j](idx[j])
        syms.append((sym + lo).astype(np.int32))
        idxs.append(idx.astype(np.int32))
    return syms, idxs


def flat(arrays, dtype=np.int32):
    return np.concatenate(arrays).astype(dtype) if sum(len(a) for a in arrays) else np.zeros(0, dtype)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


_cache = {}


def workload(O, case):
    """(lo, cdfs, lengths, syms, idxs, table models): built once per case, never modified"""
    if case not in _cache:
        n_streams, K, n, P, kind, every = case
        lo, cdfs = make_cdfs(O, K, n, P, kind)
        lengths = lengths_of(n_streams, every)
        syms, idxs = make_ragged(lengths, K, n, P, lo, cdfs, sum(case[:4]) + every)
        _cache[case] = (lo, cdfs, lengths, syms, idxs, [O.TableModel(cdfs[k], lo, P) for k in range(K)])
    return _cache[case]


def oracle_batch(O, coder, P, syms, idxs, tm, every):
    """per stream (words, jump table): one oracle coder, coded chunk by chunk (the words are the one-shot words: test_indexed_ragged_cpu.py)"""
    table_of = ans_table if coder == "ans" else range_table
    return [table_of(O, (32, 64, P), sym, [tm[k] for k in idx], every) for sym, idx in zip(syms, idxs)]


def expected(O, case, coder):
    if (case, coder) not in _cache:
        lo, cdfs, lengths, syms, idxs, tm = workload(O, case)
        _cache[(case, coder)] = oracle_batch(O, coder, case[3], syms, idxs, tm, case[5])
    return _cache[(case, coder)]


def table_set(B, case, lo, cdfs):
    if ("set", case) not in _cache:
        _cache[("set", case)] = B.TableSet.from_cdfs(cdfs, lo, case[3])
    return _cache[("set", case)]


def kernel(coder, direction, jump=False):
    return f"{coder}_{direction}_indexed_ragged_kernel" + ("<jump>" if jump else "")


def streams_of(enc):
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n_words = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n_words[s]] for s in range(len(n_words))], n_words


def assert_words(enc, want, skip=()):
    got, n_words = streams_of(enc)
    status = enc.status.cpu().numpy()
    for s, (w, _) in enumerate(want):
        if s not in skip:
            assert status[s] == OK and n_words[s] == len(w) and got[s].tolist() == w.tolist(), f"stream {s}"


def device_tables(enc):
    jump = enc.jump
    off = jump.chunk_offsets.cpu().numpy()
    cols = [jump.pos.cpu().numpy().view(np.uint32)] + [a.cpu().numpy().view(np.uint64)
                                                       for a in ([jump.state] if enc.coder == "ans" else [jump.lower, jump.range])]
    return [[tuple(int(c[k]) for c in cols) for k in range(off[s], off[s + 1])] for s in range(len(off) - 1)]


def assert_tables(B, enc, lengths, every, want, skip=()):
    jump = enc.jump
    assert isinstance(jump, B.RaggedJump if enc.coder == "ans" else B.RangeRaggedJump) and jump.interval == every
    chunks = [-(-x // every) for x in lengths]
    assert jump.chunk_offsets.cpu().tolist() == offsets_of(chunks).tolist() and jump.pos.numel() >= sum(chunks)
    for s, (g, (_, w)) in enumerate(zip(device_tables(enc), want)):
        if s not in skip:
            assert g == w, f"stream {s} ({lengths[s]} symbols): the table differs from the oracle's"


def oracle_ragged_batch(B, coder, P, want, every, pad=1):
    """the ORACLE's words packed into slabs by the test (stream s: its words and `pad` more, so slabs start at every residue mod 4), with
    the ORACLE's jump table"""
    sizes = [len(w) + pad for w, _ in want]
    word_off = offsets_of(sizes)
    words = np.full(int(word_off[-1]) + 4, 0xDEADBEEF, dtype=np.uint32)
    for s, (w, _) in enumerate(want):
        words[word_off[s]: word_off[s] + len(w)] = w
    n_words = np.array([len(w) for w, _ in want], dtype=np.int32)
    entries = [e for _, t in want for e in t] or [(0,) * (2 if coder == "ans" else 3)]
    cols = [np.array([e[i] for e in entries], dtype=np.uint64) for i in range(len(entries[0]))]
    chunk_off = dev(offsets_of([len(t) for _, t in want]))
    pos = dev(cols[0].astype(np.uint32).view(np.int32))
    rest = [dev(c.view(np.int64)) for c in cols[1:]]
    jump = B.RaggedJump(every, chunk_off, pos, *rest) if coder == "ans" else B.RangeRaggedJump(every, chunk_off, pos, *rest)
    status = torch.zeros(len(want), dtype=torch.int32, device="cuda")
    return B.RaggedBatch(dev(words.view(np.int32)), dev(word_off), dev(n_words), status, (32, 64, P), None, jump, coder)


def without_jump(B, enc):
    return B.RaggedBatch(enc.words, enc.word_offsets, enc.n_words, enc.status, enc.config, enc.order, None, enc.coder)


@pytest.mark.parametrize("dtype", list(INDEX_DTYPES))
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_words_tables_and_symbols_are_the_oracles(B, O, case, coder, dtype):
    n_streams, K, n, P, _, every = case
    lo, cdfs, lengths, syms, idxs, tm = workload(O, case)
    want = expected(O, case, coder)
    tables = table_set(B, case, lo, cdfs)
    off = offsets_of(lengths)
    assert sum(lengths) <= 25000
    if n_streams > 1:           # uint8 rows start at every byte residue
        assert {int(x) % 4 for x in off[:-1]} == {0, 1, 2, 3} and 0 in lengths and max(lengths) > 10 * sorted(lengths)[n_streams // 2]
    d_sym, d_off = dev(flat(syms)), dev(off)
    d_idx = dev_indices(flat(idxs), INDEX_DTYPES[dtype], shift=(n_streams + every // 16) % 4)
    encode, decode = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
    # 1. encode without jump points: words, counts, statuses
    plain = encode(d_sym, d_idx, d_off, tables, (32, 64, P))
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel(coder, "encode") and plain.jump is None and plain.coder == coder
    assert_words(plain, want)
    # 2. ... with: the same words, and every table entry
    enc = encode(d_sym, d_idx, d_off, tables, (32, 64, P), jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel(coder, "encode", True)
    assert_words(enc, want)
    assert_tables(B, enc, lengths, every, want)
    assert torch.equal(enc.word_offsets, plain.word_offsets) and torch.equal(enc.n_words, plain.n_words)
    got, got_plain = streams_of(enc)[0], streams_of(plain)[0]
    assert all(a.tolist() == b.tolist() for a, b in zip(got, got_plain))
    # 3. decode of the ORACLE's words with the ORACLE's table: the chunk route, then whole streams
    batch = oracle_ragged_batch(B, coder, P, want, every)
    dec, status = decode(batch, d_idx, d_off, tables)
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel(coder, "decode", True)
    assert (status.cpu().numpy() == OK).all(), status.cpu().tolist()
    assert np.array_equal(dec.cpu().numpy(), flat(syms))
    for b, order in ((batch, torch.arange(n_streams, dtype=torch.int32, device="cuda")), (without_jump(B, batch), "auto"), (without_jump(B, batch), None)):
        dec, status = decode(b, d_idx, d_off, tables, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == kernel(coder, "decode")
        assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), flat(syms))
    # 4. the device's own batch round-trips on both routes
    for b in (enc, plain):
        dec, status = decode(b, d_idx, d_off, tables)
        assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), flat(syms))


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_a_batch_of_empty_streams_only(B, O, coder):
    case = CASES[1]
    lo, cdfs, _, _, _, _ = workload(O, case)
    tables = table_set(B, case, lo, cdfs)
    n = 70
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_sym = torch.zeros(0, dtype=torch.int32, device="cuda")
    encode, decode = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
    for dtype in (torch.uint8, torch.int32):
        d_idx = torch.zeros(0, dtype=dtype, device="cuda")
        for every in (0, 16):
            enc = encode(d_sym, d_idx, d_off, tables, (32, 64, case[3]), jump_every=every)
            torch.cuda.synchronize()
            assert B.last_kernel() == kernel(coder, "encode", every > 0)
            assert enc.n_words.cpu().tolist() == [0] * n and enc.status.cpu().tolist() == [OK] * n
            dec, status = decode(enc, d_idx, d_off, tables)
            torch.cuda.synchronize()
            assert B.last_kernel() == kernel(coder, "decode", every > 0)
            assert dec.numel() == 0 and status.cpu().tolist() == [OK] * n
    # no streams at all: nothing is launched
    none = encode(d_sym, torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), tables, (32, 64, case[3]))
    assert none.n_words.numel() == 0


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_order_schedules_lanes_and_results_stay_indexed_by_stream(B, O, coder):
    case = CASES[3]
    n_streams, K, n, P, _, every = case
    lo, cdfs, lengths, syms, idxs, tm = workload(O, case)
    want = expected(O, case, coder)
    tables = table_set(B, case, lo, cdfs)
    d_sym, d_off, d_idx = dev(flat(syms)), dev(offsets_of(lengths)), dev_indices(flat(idxs), np.uint8, 3)
    encode, decode = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
    perm = np.random.default_rng(5).permutation(n_streams).astype(np.int32)
    for order in (None, "auto", "sorted", dev(perm)):
        for jump_every in (0, every):
            enc = encode(d_sym, d_idx, d_off, tables, (32, 64, P), order=order, jump_every=jump_every)
            assert_words(enc, want)
            if jump_every:
                assert_tables(B, enc, lengths, every, want)
        dec, status = decode(without_jump(B, enc), d_idx, d_off, tables, order=order)
        assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), flat(syms))
    # one entry that names no stream: the stream whose slot it took is not coded, the others are unchanged
    victim = int(perm[17])
    broken = perm.copy()
    broken[17] = n_streams + 5
    enc = encode(d_sym, d_idx, d_off, tables, (32, 64, P), order=dev(broken), jump_every=every)
    assert_words(enc, want, skip=(victim,))
    assert_tables(B, enc, lengths, every, want, skip=(victim,))
    batch = oracle_ragged_batch(B, coder, P, want, every)
    out = torch.full((sum(lengths),), -77, dtype=torch.int32, device="cuda")
    dec, status = decode(batch, d_idx, d_off, tables, out=out, order=dev(broken))
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel(coder, "decode")
    got, st, off = dec.cpu().numpy(), status.cpu().numpy(), offsets_of(lengths)
    for s in range(n_streams):
        if s == victim:
            assert (got[off[s]: off[s + 1]] == -77).all()
        else:
            assert st[s] == OK and got[off[s]: off[s + 1]].tolist() == syms[s].tolist(), f"stream {s}"


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=[IDS[1], IDS[4]])
def test_equal_lengths_give_the_rectangular_calls_words(B, O, case, coder):
    """beside the oracle, not in its place: an equal-length batch through the ragged calls gives the words of *_indexed, per stream"""
    n_streams, K, n, P, _, every = case
    lo, cdfs, _, _, _, tm = workload(O, case)
    tables = table_set(B, case, lo, cdfs)
    n_per = 41
    syms, idxs = make_ragged([n_per] * n_streams, K, n, P, lo, cdfs, 77 + n_streams)
    sym, idx = np.stack(syms), np.stack(idxs)
    for dtype in INDEX_DTYPES.values():
        rect = getattr(B, f"{coder}_encode_indexed")(dev(sym), dev(idx.astype(dtype)), tables, (32, 64, P))
        enc = getattr(B, f"{coder}_encode_indexed_ragged")(dev(sym.reshape(-1)), dev(idx.astype(dtype).reshape(-1)),
                                                            dev(offsets_of([n_per] * n_streams)), tables, (32, 64, P), jump_every=every)
        torch.cuda.synchronize()
        got, n_words = streams_of(enc)
        assert (enc.status.cpu().numpy() == OK).all() and n_words.tolist() == rect.n_words.cpu().tolist()
        for s in range(n_streams):
            assert got[s].tolist() == rect.stream(s).tolist(), f"stream {s}"
    w0 = oracle_batch(O, coder, P, syms[:1], idxs[:1], tm, every)[0][0]
    assert got[0].tolist() == w0.tolist()


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_maximum_word_rate(B, O, coder):
    """P = 24 and every coded symbol of probability 1 (24 bits each: three words per four symbols), streams of 100 and 257 symbols, a jump
    point every 16: the ring of 32 slots between two memory points is fullest here"""
    K, n, P, every = 2, 64, 24, 16
    lo = -(n // 2)
    cdfs = np.stack([O.GaussianModel(lo, lo + n - 1, m, 0.05, P).cdf_table() for m in (-3.0, 7.0)])
    prob = np.diff(cdfs.astype(np.int64), axis=1)
    assert sorted(prob[0].tolist()) == [1] * (n - 1) + [(1 << P) - (n - 1)]
    rng = np.random.default_rng(24)
    lengths = [100, 257] * 33 + [100]
    syms, idxs = [], []
    for length in lengths:
        idx = rng.integers(0, K, length)
        sym = rng.integers(0, n, length)
        sym = np.where(prob[idx, sym] == 1, sym, (sym + 1) % n)
        assert (prob[idx, sym] == 1).all()
        syms.append((sym + lo).astype(np.int32))
        idxs.append(idx.astype(np.int32))
    tm = [O.TableModel(cdfs[k], lo, P) for k in range(K)]
    want = oracle_batch(O, coder, P, syms, idxs, tm, every)
    assert max(len(w) for w, _ in want) >= 257 * P // 32
    tables = B.TableSet.from_cdfs(cdfs, lo, P)
    d_sym, d_off = dev(flat(syms)), dev(offsets_of(lengths))
    for dtype in INDEX_DTYPES.values():
        d_idx = dev_indices(flat(idxs), dtype, 1)
        for jump_every in (every, 0):
            enc = getattr(B, f"{coder}_encode_indexed_ragged")(d_sym, d_idx, d_off, tables, (32, 64, P), jump_every=jump_every)
            assert_words(enc, want)
            if jump_every:
                assert_tables(B, enc, lengths, every, want)
        batch = oracle_ragged_batch(B, coder, P, want, every)
        for b in (batch, without_jump(B, batch)):
            dec, status = getattr(B, f"{coder}_decode_indexed_ragged")(b, d_idx, d_off, tables)
            assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), flat(syms))


FAIL_CASE = (65, 2, 64, 12, "gauss", 32)


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_an_impossible_symbol_or_index_fails_its_stream_alone(B, O, coder):
    n_streams, K, n, P, _, every = FAIL_CASE
    lo, cdfs, lengths, syms, idxs, tm = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    off = offsets_of(lengths)
    encode, decode = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
    victim = 3
    assert lengths[victim] == 3 * every + 5 and K < 256
    d_off = dev(off)
    batch = oracle_ragged_batch(B, coder, P, want, every)
    for t in (0, lengths[victim] // 2, lengths[victim] - 1):
        at = off[victim] + t
        for jump_every in (0, every):
            for value in (lo + n, lo - 1):                      # a symbol outside the support, on either side
                bad = flat(syms)
                bad[at] = value
                enc = encode(dev(bad), dev_indices(flat(idxs), np.uint8, 2), d_off, tables, (32, 64, P), jump_every=jump_every)
                assert enc.status[victim].item() == IMPOSSIBLE and enc.n_words[victim].item() == 0
                assert_words(enc, want, skip=(victim,))
            for dtype, values in ((np.uint8, (K,)), (np.int32, (K, -1))):         # an index that names no table
                for value in values:
                    bad = flat(idxs).astype(dtype)
                    bad[at] = value
                    d_bad = dev_indices(bad, dtype, 1)
                    enc = encode(dev(flat(syms)), d_bad, d_off, tables, (32, 64, P), jump_every=jump_every)
                    assert enc.status[victim].item() == IMPOSSIBLE and enc.n_words[victim].item() == 0
                    assert_words(enc, want, skip=(victim,))
                    if jump_every:
                        assert_tables(B, enc, lengths, every, want, skip=(victim,))
                    # the decoders: invalid data for that stream, on the chunk route and by whole streams
                    dec, st = decode(batch if jump_every else without_jump(B, batch), d_bad, d_off, tables)
                    torch.cuda.synchronize()
                    assert B.last_kernel() == kernel(coder, "decode", jump_every > 0)
                    st, dec = st.cpu().numpy(), dec.cpu().numpy()
                    assert st[victim] == INVALID and (np.delete(st, victim) == OK).all()
                    keep = np.ones(len(dec), dtype=bool)
                    keep[off[victim]: off[victim + 1]] = False
                    assert np.array_equal(dec[keep], flat(syms)[keep])
                    assert np.array_equal(dec[off[victim]: at], flat(syms)[off[victim]: at])      # (what came before the index is still right)


def native(B, name, *args):
    from constriction_amd import _native as N
    rc = getattr(N.lib(), name)(*args)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_a_slab_one_word_short_is_capacity_for_that_stream_alone(B, O, coder):
    from constriction_amd import _native as N
    n_streams, K, n, P, _, every = FAIL_CASE
    lo, cdfs, lengths, syms, idxs, tm = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    short = {5, 31, 64}
    assert all(len(want[s][0]) > 0 for s in short)
    sizes = [len(w) - (1 if s in short else 0) for s, (w, _) in enumerate(want)]
    word_off = offsets_of(sizes)
    word_off[40], word_off[41] = word_off[41], word_off[40]                # ... and one pair of offsets that runs backwards: stream 40
    guard = torch.full((int(word_off[-1]) + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_sym, d_idx, d_off, d_woff = dev(flat(syms)), dev(flat(idxs)), dev(offsets_of(lengths)), dev(word_off)
    n_words = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    rc = native(B, f"cst_{coder}_encode_indexed_ragged", N.CoderConfig(32, 64, P), tables._h, B._ptr(d_sym), B._ptr(d_idx), 4, B._ptr(d_off), n_streams,
                None, B._ptr(guard), B._ptr(d_woff), 0, B._ptr(n_words), B._ptr(status), B._stream_ptr())
    assert rc == N.CST_OK and B.last_kernel() == kernel(coder, "encode")
    words, n_words, status = guard.cpu().numpy().view(np.uint32), n_words.cpu().numpy(), status.cpu().numpy()
    for s, (w, _) in enumerate(want):
        if s in short or s == 40:
            assert status[s] == CAPACITY and n_words[s] == 0, s
        elif s not in (39, 41):            # (the neighbours of the swapped pair have slabs of another size: whatever they report is theirs)
            assert status[s] == OK and words[word_off[s]: word_off[s] + n_words[s]].tolist() == w.tolist(), f"stream {s}"
    assert (words[int(word_off[-1]):] == 0x5A5A5A5A).all()          # nothing behind the last slab


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_tables_and_capacities_are_checked_stream_by_stream(B, O, coder):
    """a jump point beyond its stream's words, one stream's chunk offset off by one, a table shorter than its chunks: INVALID_DATA for
    exactly those streams, whose symbols stay as the caller filled them; the others decode.  The decoder derives no address from the
    table that it has not clamped or rejected first (persymbol_jump_chunks_kernel, indexed_jump_precheck_kernel)."""
    from constriction_amd import _native as N
    n_streams, K, n, P, _, every = FAIL_CASE
    lo, cdfs, lengths, syms, idxs, tm = workload(O, FAIL_CASE)
    want = expected(O, FAIL_CASE, coder)
    tables = table_set(B, FAIL_CASE, lo, cdfs)
    off = offsets_of(lengths)
    d_idx, d_off = dev_indices(flat(idxs), np.uint8, 3), dev(off)
    decode = getattr(B, f"{coder}_decode_indexed_ragged")
    chunk_off = offsets_of([len(t) for _, t in want])

    def check(batch, bad):
        out = torch.full((sum(lengths),), -77, dtype=torch.int32, device="cuda")
        dec, status = decode(batch, d_idx, d_off, tables, out=out)
        torch.cuda.synchronize()
        assert B.last_kernel() == kernel(coder, "decode", True)
        st, got = status.cpu().numpy(), dec.cpu().numpy()
        assert [s for s in range(n_streams) if st[s] != OK] == sorted(bad) and all(st[s] == INVALID for s in bad), st.tolist()
        for s in range(n_streams):
            if s in bad:
                assert (got[off[s]: off[s + 1]] == -77).all(), f"stream {s} was written"
            else:
                assert got[off[s]: off[s + 1]].tolist() == syms[s].tolist(), f"stream {s}"

    check(oracle_ragged_batch(B, coder, P, want, every), ())
    # (1) a jump point one word beyond its stream's words: chunk 1 of stream 3
    batch = oracle_ragged_batch(B, coder, P, want, every)
    assert len(want[3][1]) == 4
    batch.jump.pos[chunk_off[3] + 1] = len(want[3][0]) + 1
    check(batch, (3,))
    # (2) the chunk offset of stream 15 one too large: stream 14 is given a chunk too many, stream 15 one too few
    batch = oracle_ragged_batch(B, coder, P, want, every)
    assert lengths[14] > 0 and lengths[15] > 0
    shifted = chunk_off.copy()
    shifted[15] += 1
    batch.jump.chunk_offsets = dev(shifted)
    check(batch, (14, 15))
    # (3) n_chunks_total too small: the table arrays end two entries early, inside the last stream that has chunks
    batch = oracle_ragged_batch(B, coder, P, want, every)
    cut = int(chunk_off[-1]) - 2
    for name in ("pos", "state", "lower", "range"):
        if hasattr(batch.jump, name):
            setattr(batch.jump, name, getattr(batch.jump, name)[:cut].clone())
    cut_off = tuple(s for s in range(n_streams) if chunk_off[s + 1] > cut)          # (an empty stream behind the cut is not described either)
    assert 1 <= len(cut_off) < 8 and any(lengths[s] > 0 for s in cut_off)
    check(batch, cut_off)
    # (4) words_capacity shorter than the last slab: flagged as the plain decoders flag it, on both routes
    batch = oracle_ragged_batch(B, coder, P, want, every)
    last_w = max(s for s in range(n_streams) if len(want[s][0]) > 0)
    word_off = batch.word_offsets.cpu().numpy()
    capacity = int(word_off[last_w]) + len(want[last_w][0]) - 1
    out = torch.full((sum(lengths),), -77, dtype=torch.int32, device="cuda")
    status = torch.full((n_streams,), -1, dtype=torch.int32, device="cuda")
    cfg = N.CoderConfig(32, 64, P)
    rc = native(B, f"cst_{coder}_decode_indexed_ragged", cfg, tables._h, B._ptr(batch.words), B._ptr(batch.word_offsets), 0, capacity,
                B._ptr(batch.n_words), B._ptr(d_idx), 1, B._ptr(out), B._ptr(d_off), n_streams, None, B._ptr(status), B._stream_ptr())
    assert rc == N.CST_OK
    st = status.cpu().numpy()
    assert st[last_w] == INVALID and (np.delete(st, last_w)[: last_w] == OK).all()
    arrays = (batch.jump.pos, batch.jump.state) if coder == "ans" else (batch.jump.pos, batch.jump.lower, batch.jump.range)
    n_chunks = int(chunk_off[-1])
    scratch = torch.zeros(N.lib().cst_persymbol_ragged_jump_scratch_bytes(n_chunks), dtype=torch.uint8, device="cuda")
    status.fill_(-1)
    rc = native(B, f"cst_{coder}_decode_indexed_ragged_jump", cfg, tables._h, B._ptr(batch.words), B._ptr(batch.word_offsets), 0, capacity,
                B._ptr(batch.n_words), B._ptr(d_idx), 1, B._ptr(out), B._ptr(d_off), n_streams, every, B._ptr(batch.jump.chunk_offsets), n_chunks,
                *(B._ptr(t) for t in arrays), B._ptr(scratch), B._ptr(status), B._stream_ptr())
    assert rc == N.CST_OK and B.last_kernel() == kernel(coder, "decode", True)
    st = status.cpu().numpy()
    assert st[last_w] == INVALID and (np.delete(st, last_w)[: last_w] == OK).all()
    # no streams: CST_OK, nothing launched, with a live handle
    assert native(B, f"cst_{coder}_decode_indexed_ragged", cfg, tables._h, B._ptr(batch.words), B._ptr(batch.word_offsets), 0, capacity,
                  B._ptr(batch.n_words), B._ptr(d_idx), 1, B._ptr(out), B._ptr(d_off), 0, None, B._ptr(status), B._stream_ptr()) == N.CST_OK
    # the precision of the call is not the set's
    assert native(B, f"cst_{coder}_decode_indexed_ragged", N.CoderConfig(32, 64, P + 1), tables._h, B._ptr(batch.words), B._ptr(batch.word_offsets), 0,
                  capacity, B._ptr(batch.n_words), B._ptr(d_idx), 1, B._ptr(out), B._ptr(d_off), n_streams, None, B._ptr(status),
                  B._stream_ptr()) == N.CST_ERR_INVALID_ARGUMENT
