"""GPU tests of random access into ragged batches (`cst_{ans,range}_decode_ragged_select`, `batched.{ans,range}_decode_ragged_select`):
selected documents and ranges of documents, with and without a jump table, for both coders.  The expected symbols are always slices of
the INPUT documents (made with `O.synth_symbols` from an oracle table); no GPU result is the reference for another, except where a test
says so."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KERNEL = {"ans": "ans_decode_ragged_kernel<select>", "range": "range_decode_ragged_kernel<select>"}
CODERS = ["ans", "range"]
INVALID = 3


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


def encode(B, coder, flat, offsets, model, cfg, every):
    """a batch of `coder` with a jump point every `every` symbols (0: no table)"""
    if coder == "ans":
        enc = B.ans_encode_ragged(flat, offsets, model, cfg, jump_every=every)
    else:
        enc = B.range_encode_ragged_jump(flat, offsets, model, cfg, jump_every=every)
    assert (enc.jump is not None) == (every != 0) and int(enc.status.abs().sum()) == 0
    return enc


def select(B, coder, *args, **kwargs):
    out = getattr(B, f"{coder}_decode_ragged_select")(*args, **kwargs)
    assert B.last_kernel() == KERNEL[coder]
    return out


def decode_all(B, coder, enc, model, offsets):
    return (B.ans_decode_ragged if coder == "ans" else B.range_decode_ragged)(enc, model, offsets)


def expected(docs, queries):
    """the slices of the input documents that the queries (stream, first, count) ask for, and their offsets"""
    parts = [np.asarray(docs[s][f: f + c], dtype=np.int32) for s, f, c in queries]
    offsets = np.concatenate([[0], np.cumsum([c for _, _, c in queries])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


def check(B, coder, enc, model, offsets, docs, queries, whole=False):
    """one select call for `queries`; whole = True sends them as whole documents (first = count = None)"""
    streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int32, device="cuda")
    if whole:
        assert all(f == 0 and c == len(docs[s]) for s, f, c in queries)
        got, out_offsets, status = select(B, coder, enc, model, offsets, streams)
    else:
        got, out_offsets, status = select(B, coder, enc, model, offsets, streams, [f for _, f, _ in queries], [c for _, _, c in queries])
    want, want_offsets = expected(docs, queries)
    assert got.dtype == torch.int32 and out_offsets.dtype == torch.int64 and status.dtype == torch.int32
    assert out_offsets.cpu().tolist() == want_offsets.tolist()
    assert status.cpu().tolist() == [0] * len(queries)
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        q = int(np.searchsorted(want_offsets, k, side="right")) - 1
        raise AssertionError(f"query {q} = {queries[q]}: symbol {k - want_offsets[q]} of its slice differs")


_mixes = {}


def document_mix(B, O, P, nominal):
    """About 300 documents: lengths 0 .. 199 mostly, forty of 200 .. 2999, and the edges of a chunk of `nominal` symbols; made once
    per (precision, chunk length)"""
    if (P, nominal) not in _mixes:
        rng = np.random.default_rng(100 * P + nominal)
        n_sym, lo = 90, -17
        cdf = O.categorical_fast_cdf(rng.dirichlet(np.ones(n_sym) * 0.4), P)
        lengths = np.concatenate([rng.integers(0, 200, 250), rng.integers(200, 3000, 40),
                                  [0, 0, 1, 7, 8, 9, nominal - 1, nominal, nominal + 1, 2 * nominal, 2047]])
        rng.shuffle(lengths)
        docs = [O.synth_symbols(int(k), 0, 1, int(n), lo, cdf, P)[0] if n else np.zeros(0, np.int32) for k, n in enumerate(lengths)]
        _mixes[(P, nominal)] = (lo, cdf, lengths, docs)
    return _mixes[(P, nominal)]


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("cfg", [(32, 64, 24), (32, 64, 12), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("every", [0, 8, 64, 256])
def test_parity(B, O, coder, cfg, every):
    """Whole documents forward, reversed and repeated (empty ones among them); empty ranges; on the longest document every start and
    length around a group of eight and around a chunk; a range inside one chunk, one across three, one that ends with the document.
    Every slice is the input's, out_offsets the prefix sum of the counts, every status 0."""
    P = cfg[2]
    I = every or 64                       # (without a table: the same edges, around a chunk nobody noted)
    lo, cdf, lengths, docs = document_mix(B, O, P, I)
    model = B.Model.from_cdf(cdf, lo, P)
    flat, offsets = B.ragged(docs)
    enc = encode(B, coder, flat, offsets, model, cfg, every)
    n = len(docs)
    whole = lambda s: (s, 0, len(docs[s]))
    empties = [s for s in range(n) if len(docs[s]) == 0]
    assert len(empties) >= 2
    check(B, coder, enc, model, offsets, docs, [whole(s) for s in range(n)], whole=True)
    check(B, coder, enc, model, offsets, docs, [whole(s) for s in reversed(range(n))], whole=True)
    check(B, coder, enc, model, offsets, docs, [whole(s) for s in [5, 5, 17, 5, empties[0], 17, empties[0], n - 1, 0, n - 1]], whole=True)
    longest = int(np.argmax(lengths))
    L = len(docs[longest])
    assert L > 4 * I + 20
    queries = [(s, 0, 0) for s in empties] + [(longest, 0, 0), (longest, 5, 0), (longest, L, 0), (3, len(docs[3]), 0)]
    for first in (0, 1, 7, 8, 9, I - 1, I, I + 1):
        for count in (1, 7, 8, 9, I, I + 1, L - first):
            queries.append((longest, first, count))
    queries += [(longest, I + 2, I - 4),                   # inside one chunk
                (longest, 2 * I - 3, I + 6),               # across three chunks
                (longest, L - I - 5, I + 5), (longest, L - 1, 1), (longest, L - 9, 9)]      # ... ending at the document's last symbol
    other = int(np.argsort(lengths)[-2])
    queries += [(other, 3, len(docs[other]) - 3), (other, len(docs[other]) - 1, 1)]
    check(B, coder, enc, model, offsets, docs, queries)
    # the same queries the other way round, every second one twice: the order of the queries is the caller's
    check(B, coder, enc, model, offsets, docs, [q for k, q in enumerate(reversed(queries)) for _ in range(1 + k % 2)])


@pytest.fixture(scope="module")
def small(B, O):
    """a 40-symbol table at P = 12 and 40 documents of 50 .. 299 symbols, encoded by both coders with a table (64) and without"""
    P, lo = 12, 0
    cfg = (32, 64, P)
    cdf = O.categorical_fast_cdf(np.ones(40) / 40, P)
    model = B.Model.from_cdf(cdf, lo, P)
    lengths = np.random.default_rng(3).integers(50, 300, 40)
    docs = [O.synth_symbols(int(k), 0, 1, int(n), lo, cdf, P)[0] for k, n in enumerate(lengths)]
    flat, offsets = B.ragged(docs)
    batches = {(coder, every): encode(B, coder, flat, offsets, model, cfg, every) for coder in CODERS for every in (0, 64)}
    return model, docs, flat, offsets, batches


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("n_queries", [1, 63, 64, 65, 257])
def test_shapes_of_the_launch(B, small, coder, every, n_queries):
    """partial last waves and blocks in every pass: the queries' kernels have a thread per query, the decoder a lane per piece"""
    model, docs, flat, offsets, batches = small
    rng = np.random.default_rng(n_queries)
    queries = []
    for _ in range(n_queries):
        s = int(rng.integers(0, len(docs)))
        first = int(rng.integers(0, len(docs[s])))
        queries.append((s, first, int(rng.integers(0, len(docs[s]) - first + 1))))
    check(B, coder, batches[(coder, every)], model, offsets, docs, queries)


@pytest.mark.parametrize("coder", CODERS)
def test_a_tables_worth(B, small, coder):
    """all documents in order, whole: the flat output of the full decode of the same batch (which its own tests pin to the oracle) --
    and the input"""
    model, docs, flat, offsets, batches = small
    enc = batches[(coder, 64)]
    got, out_offsets, status = select(B, coder, enc, model, offsets, torch.arange(len(docs), device="cuda"))
    full, full_status = decode_all(B, coder, enc, model, offsets)
    assert torch.equal(got, full) and torch.equal(got, flat) and torch.equal(out_offsets, offsets)
    assert int(status.abs().sum()) == 0 and int(full_status.abs().sum()) == 0


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("cfg,n_sym", [((32, 64, 6), 40), ((16, 32, 5), 20), ((32, 64, 16), 5000), ((32, 64, 20), 20000), ((16, 32, 16), 5000),
                                       ((32, 64, 22), 1000), ((32, 64, 24), 256)],
                         ids=lambda v: "W%dS%dP%d" % v if isinstance(v, tuple) else "n%d" % v)
def test_kernel_variants(B, coder, cfg, n_sym):
    """The (preset, alphabet) pairs of test_kernel_variants (tests/test_gpu_range_ragged_jump.py): tables in LDS and too large for it,
    16-bit words, P < 8.  Twenty documents, ten queries, with a table and without."""
    W, S, P = cfg
    rng = np.random.default_rng(n_sym + P)
    lo = -3
    w = rng.gamma(0.3, 1.0, n_sym) + 1e-9
    p = np.maximum(1, np.floor(w / w.sum() * ((1 << P) - n_sym)).astype(np.int64))
    p[int(np.argmax(p))] += (1 << P) - int(p.sum())
    cdf = np.concatenate([[0], np.cumsum(p)]).astype(np.uint32)
    model = B.Model.from_cdf(cdf, lo, P)
    lengths = np.concatenate([[0, 1, 63, 64, 65, 700], rng.integers(0, 700, 14)])
    docs = [(lo + rng.choice(n_sym, size=int(n), p=p / p.sum())).astype(np.int32) for n in lengths]
    flat, offsets = B.ragged(docs)
    queries = [(5, 0, 700), (5, 699, 1), (5, 61, 140), (4, 1, 64), (3, 0, 64), (2, 62, 1), (1, 0, 1), (0, 0, 0)]
    queries += [(s, len(docs[s]) // 3, len(docs[s]) - len(docs[s]) // 3) for s in (9, 17)]
    assert len(docs) == 20 and len(queries) == 10
    for every in (64, 0):
        check(B, coder, encode(B, coder, flat, offsets, model, cfg, every), model, offsets, docs, queries)


@pytest.mark.parametrize("coder", CODERS)
def test_noncontiguous_alphabet(B, O, coder):
    """a model over arbitrary distinct symbols (Model.from_cdf_noncontiguous): the indices come back as symbols"""
    P, cfg = 12, (32, 64, 12)
    rng = np.random.default_rng(11)
    alphabet = np.sort(rng.choice(np.arange(-5000, 5000), size=30, replace=False)).astype(np.int32)
    rng.shuffle(alphabet)
    cdf = O.categorical_fast_cdf(rng.dirichlet(np.ones(30)), P)
    model = B.Model.from_cdf_noncontiguous(alphabet, cdf, P)
    docs = [alphabet[O.synth_symbols(int(k), 0, 1, int(n), 0, cdf, P)[0]] if n else np.zeros(0, np.int32)
            for k, n in enumerate([300, 0, 77, 64, 129])]
    flat, offsets = B.ragged(docs)
    enc = encode(B, coder, flat, offsets, model, cfg, 64)
    check(B, coder, enc, model, offsets, docs, [(4, 60, 69), (0, 1, 299), (2, 0, 77), (1, 0, 0), (3, 63, 1), (0, 130, 3)])


# ---- the C calls themselves: caller data gone wrong ----

FILL, MARGIN = 77, 512


def raw_select(B, coder, enc, model, offsets, queries, sizes=None, pieces=None):
    """The C call with hand-made arrays: `queries` are (stream, first, count) of unsigned integers sent as they are; every query owns
    sizes[q] (default: count) symbols of an output that is pre-filled with FILL and lies between two margins of FILL; `pieces` are
    the piece counts behind d_piece_offsets (default: the Python layer's formula).  Returns (output without its margins, both margins,
    out_offsets on the host, status on the host)."""
    from constriction_amd import _native as N
    L = N.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u64 = lambda values: np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)
    nq = len(queries)
    streams = dev(np.array([s for s, _, _ in queries], dtype=np.uint32).view(np.int32))
    first, count = dev(u64(f for _, f, _ in queries)), dev(u64(c for _, _, c in queries))
    sizes = [c for _, _, c in queries] if sizes is None else sizes
    interval = enc.jump.interval if enc.jump is not None else 0
    if pieces is None:
        pieces = B._select_piece_counts(torch.tensor([f % (1 << 62) for _, f, _ in queries]), torch.tensor(sizes), interval).tolist()
    out_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    piece_offsets = np.concatenate([[0], np.cumsum(pieces)]).astype(np.int64)
    total, n_pieces = int(out_offsets[-1]), int(piece_offsets[-1]) + 3          # (an upper bound of the pieces)
    guard = torch.full((total + 2 * MARGIN,), FILL, dtype=torch.int32, device="cuda")
    body = guard[MARGIN: MARGIN + total]
    status = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    d_out_offsets, d_piece_offsets = dev(out_offsets), dev(piece_offsets)
    p = lambda t: C.c_void_p(t.data_ptr())
    j = enc.jump
    head = (model._h, N.CoderConfig(*enc.config), p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words), p(offsets),
            offsets.numel() - 1)
    tail = (p(streams), p(first), p(count), nq, p(d_piece_offsets), n_pieces, p(body) if total else p(guard), p(d_out_offsets))
    if coder == "ans":
        table = (interval, p(j.chunk_offsets), j.pos.numel(), p(j.pos), p(j.state)) if j is not None else (0, None, 0, None, None)
        scratch = torch.empty(L.cst_ragged_select_scratch_bytes(n_pieces), dtype=torch.uint8, device="cuda")
        N.check(L.cst_ans_decode_ragged_select(*head, *table, *tail, p(scratch), p(status), None), "cst_ans_decode_ragged_select")
    else:
        table = (interval, p(j.chunk_offsets), j.pos.numel(), p(j.pos), p(j.lower), p(j.range)) if j is not None else (0, None, 0, None, None, None)
        scratch = torch.empty(L.cst_range_ragged_select_scratch_bytes(n_pieces), dtype=torch.uint8, device="cuda")
        N.check(L.cst_range_decode_ragged_select(*head, *table, *tail, p(scratch), p(status), None), "cst_range_decode_ragged_select")
    assert B.last_kernel() == KERNEL[coder]
    torch.cuda.synchronize()
    return body.cpu().numpy(), torch.cat([guard[:MARGIN], guard[MARGIN + total:]]).cpu().numpy(), out_offsets, status.cpu().numpy()


def check_raw(result, docs, queries, bad):
    """queries in `bad` report INVALID_DATA and their slices still hold FILL; the others hold the input's slices; the margins hold FILL"""
    body, margins, out_offsets, status = result
    assert (margins == FILL).all()
    assert status.tolist() == [INVALID if q in bad else 0 for q in range(len(queries))]
    for q, (s, f, c) in enumerate(queries):
        piece = body[out_offsets[q]: out_offsets[q + 1]]
        if q in bad:
            assert (piece == FILL).all(), f"query {q} = {queries[q]} was refused and wrote"
        else:
            assert piece.tolist() == docs[s][f: f + c].tolist(), f"query {q} = {queries[q]}"


def with_table(B, enc, **changed):
    """the batch with some arrays of its jump table replaced"""
    import dataclasses
    return dataclasses.replace(enc, jump=dataclasses.replace(enc.jump, **changed))


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("every", [0, 64])
def test_bad_queries(B, small, coder, every):
    """streams that are none, ranges beyond their documents, a 64-bit wrap, piece counts that are off, table entries beyond the stream's
    words, a table slice that is too short: INVALID_DATA for exactly those queries, which write nothing; the others decode; nothing
    outside the output is touched.  None of this is a fault: every bad input is refused by an index check."""
    model, docs, flat, offsets, batches = small
    enc = batches[(coder, every)]
    n = len(docs)
    T = next(s for s in range(1, n - 1) if len(docs[s]) >= 140)              # the stream the bad queries are about: three chunks or more
    far = int(np.argmax([len(d) for d in docs]))
    L7 = len(docs[T])
    assert len(docs[far]) >= 200
    others = [s for s in range(n) if s not in (T, T + 1)][:3]
    good = [(others[0], 0, len(docs[others[0]])), (T, 5, 20), (far, 70, 130), (T, L7 - 1, 1), (0, 0, 0)]
    queries = list(good)
    bad = set()
    for q in [(n, 0, 5), (0xffffffff, 0, 5), (n + 1000, 0, 0),             # no such document (an empty range of it included)
              (T, L7 - 3, 4), (T, L7, 1), (T, L7 + 1, 0),                   # one past the end
              (T, (1 << 64) - 1, 2),                                       # first + count wraps to 1
              (T, 2, (1 << 64) - 1), (T, 1 << 63, 1 << 63)]:
        bad.add(len(queries))
        queries.append(q)
        queries.append(good[len(queries) % len(good)])                     # good ones in between
    sizes = [min(c, 6) if q in bad else c for q, (_, _, c) in enumerate(queries)]
    check_raw(raw_select(B, coder, enc, model, offsets, queries, sizes=sizes), docs, queries, bad)
    # an output slice that is not `count` long: the query alone is refused
    sizes = [c for _, _, c in good]
    sizes[1] -= 1
    check_raw(raw_select(B, coder, enc, model, offsets, good, sizes=sizes), docs, good, {1})
    # d_piece_offsets with one query's count off by one, either way
    interval = every
    right = B._select_piece_counts(torch.tensor([f for _, f, _ in good]), torch.tensor([c for _, _, c in good]), interval).tolist()
    for q, delta in ((1, 1), (2, -1), (4, 1)):
        wrong = list(right)
        wrong[q] += delta
        check_raw(raw_select(B, coder, enc, model, offsets, good, pieces=wrong), docs, good, {q})
    if not every:
        return
    # a jump_pos entry above its stream's n_words: the queries that touch that entry, and they alone
    co = enc.jump.chunk_offsets.cpu().numpy()
    assert co[T + 1] - co[T] >= 3
    pos = enc.jump.pos.clone()
    pos[int(co[T]) + 1] = int(enc.n_words[T]) + 1
    queries = [(T, 0, 64), (T, 0, 65), (T, 64, 1), (T, 10, L7 - 10), (T, 63, 1), (others[1], 0, len(docs[others[1]])), (T, 0, 10),
               (T, 128, L7 - 128)]
    check_raw(raw_select(B, coder, with_table(B, enc, pos=pos), model, offsets, queries), docs, queries, {1, 2, 3})
    # a truncated chunk_offsets slice for stream T (stream T + 1's then has an entry too many): the queries on those two
    short = enc.jump.chunk_offsets.clone()
    short[T + 1] -= 1
    queries = [(others[0], 0, len(docs[others[0]])), (T, 0, 1), (T, 0, 0), (T + 1, 3, 4), (others[1], 0, len(docs[others[1]])), (others[2], 9, 9)]
    check_raw(raw_select(B, coder, with_table(B, enc, chunk_offsets=short), model, offsets, queries), docs, queries, {1, 2, 3})


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("every", [0, 64])
def test_corrupt_counts(B, small, coder, every):
    """n_words of one stream halved (the ragged tests' idea): queries on that stream report what the full decode of the same batch
    reports for the stream, the queries on other streams are correct."""
    import dataclasses
    model, docs, flat, offsets, batches = small
    enc = batches[(coder, every)]
    victim = int(np.argmax([len(d) for d in docs]))
    n_words = enc.n_words.clone()
    n_words[victim] //= 2
    broken = dataclasses.replace(enc, n_words=n_words)
    _, full_status = decode_all(B, coder, broken, model, offsets)
    full_status = full_status.cpu().tolist()
    assert all(st == 0 for s, st in enumerate(full_status) if s != victim)
    a, b, c = [s for s in range(len(docs)) if s != victim][:3]
    queries = [(s, 0, len(docs[s])) for s in (a, victim, b, victim, c)]
    guard = torch.full((sum(c for _, _, c in queries) + 2 * MARGIN,), FILL, dtype=torch.int32, device="cuda")
    got, out_offsets, status = select(B, coder, broken, model, offsets, [s for s, _, _ in queries], out=guard[MARGIN: -MARGIN])
    assert status.cpu().tolist() == [full_status[victim] if s == victim else 0 for s, _, _ in queries]
    assert bool((guard[:MARGIN] == FILL).all()) and bool((guard[-MARGIN:] == FILL).all())
    got, oo = got.cpu().numpy(), out_offsets.cpu().numpy()
    for q, (s, f, c) in enumerate(queries):
        if s != victim:
            assert got[oo[q]: oo[q + 1]].tolist() == docs[s].tolist()


@pytest.mark.parametrize("coder", CODERS)
def test_refusals_with_a_model(B, small, coder):
    """the refusals of tests/test_ragged_select_cpu.py with a real model (HOST buffers behind the pointers of calls that must be refused),
    and the calls that launch nothing"""
    from constriction_amd import _native as N
    model, docs, flat, offsets, batches = small
    L, cc = N.lib(), N.CoderConfig(32, 64, 12)
    host = np.zeros(64, dtype=np.float64)
    h = C.c_void_p(host.ctypes.data)
    fn = L.cst_ans_decode_ragged_select if coder == "ans" else L.cst_range_decode_ragged_select
    n_table = 3 if coder == "ans" else 4

    def call(cfg=cc, interval=64, table=None, first=h, count=h, n_queries=1, n_pieces=8, n_chunks=8, word_offsets=h, sym_offsets=h, n_words=h,
             stream=h, piece_offsets=h, out_offsets=h, scratch=h, status=h):
        table = [h] * n_table if table is None else table
        return fn(model._h, cfg, h, word_offsets, 0, 64, n_words, sym_offsets, 1, interval, table[0], n_chunks, *table[1:], stream, first, count,
                  n_queries, piece_offsets, n_pieces, h, out_offsets, scratch, status, None)

    bad = N.CST_ERR_INVALID_ARGUMENT
    for n_queries in (0, 1):
        assert call(cfg=N.CoderConfig(32, 64, 24), n_queries=n_queries) == bad          # not the model's precision
        for interval in (4, 12, 1 << 31):
            assert call(interval=interval, n_queries=n_queries) == bad
        for k in range(n_table):
            assert call(table=[None if i == k else h for i in range(n_table)], n_queries=n_queries) == bad
            assert call(interval=0, table=[h if i == k else None for i in range(n_table)], n_queries=n_queries) == bad
        assert call(interval=0, n_queries=n_queries) == bad and call(table=[None] * n_table, n_queries=n_queries) == bad
        assert call(first=None, n_queries=n_queries) == bad and call(count=None, n_queries=n_queries) == bad
        assert call(n_pieces=1 << 32, n_queries=n_queries) == bad and call(n_chunks=1 << 32, n_queries=n_queries) == bad
        assert call(sym_offsets=None, n_queries=n_queries) == bad and call(n_words=None, n_queries=n_queries) == bad
        if coder == "range":
            assert call(word_offsets=None, n_queries=n_queries) == bad                  # no offsets and no stride
    for name in ("stream", "piece_offsets", "out_offsets", "scratch", "status"):
        assert call(**{name: None}) == bad, name
    # no queries: nothing is launched, with a table, without one, and whatever hides behind the query pointers
    assert call(n_queries=0) == N.CST_OK
    assert call(n_queries=0, interval=0, table=[None] * n_table, first=None, count=None) == N.CST_OK
    assert call(n_queries=0, stream=None, piece_offsets=None, out_offsets=None, scratch=None, status=None) == N.CST_OK
    got, out_offsets, status = select_nothing(B, coder, batches[(coder, 64)], model, offsets)
    assert got.numel() == 0 and out_offsets.cpu().tolist() == [0] and status.numel() == 0


def select_nothing(B, coder, enc, model, offsets):
    return getattr(B, f"{coder}_decode_ragged_select")(enc, model, offsets, torch.zeros(0, dtype=torch.int64, device="cuda"))
