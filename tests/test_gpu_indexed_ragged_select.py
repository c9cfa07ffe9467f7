"""GPU tests of random access into ragged indexed batches (csrc/cst_indexed_ragged.hip, MODE kRgSelect;
batched.{ans,range}_decode_indexed_ragged_select): a query (stream, first, count) decodes symbols [first, first + count)
of one stream and nothing else, from the jump point in front of `first` where the batch has jump points.

Expected values are the INPUT symbols, except where the oracle's words and the oracle's table are decoded (the batches of
tests/test_gpu_indexed_ragged.py, imported).  Tables, symbols and indices by that file's rules; the (K, n, P) combinations are taken
from the grid of tests/test_gpu_indexed.py: (2, 64, 12) and (64, 255, 16) with 16-bit rows, (64, 255, 24) and (2, 64, 24) with 32-bit
rows; K < 256 with uint8 indices throughout.  Shapes sit on the kernel's edges: the eight-index group, the 16-symbol tile, the jump
interval, the four byte residues of a uint8 row."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_gpu_indexed import make_cdfs
from test_gpu_indexed_ragged import (CASES as RAGGED_CASES, INDEX_DTYPES, dev, dev_indices, expected as oracle_expected, flat, make_ragged, offsets_of,
                                     oracle_ragged_batch, table_set, without_jump, workload)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, IMPOSSIBLE, CAPACITY, INVALID = 0, 1, 2, 3
FILL, MARGIN = -77777, 64
G12, G16, G24 = (2, 64, 12, "gauss"), (64, 255, 16, "gauss"), (64, 255, 24, "gauss")
FORMS = [(coder, dtype) for coder in ("ans", "range") for dtype in INDEX_DTYPES]
form_id = lambda f: "-".join(f)


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


def kernel(coder):
    return f"{coder}_decode_indexed_ragged_kernel<select>"


@dataclasses.dataclass
class Batch:
    coder: str
    dtype: str
    every: int
    K: int
    syms: list
    idxs: list
    d_idx: object
    d_off: object
    tables: object
    enc: object


_BATCHES, _SETS = {}, {}


def tables_of(B, O, grid):
    if grid not in _SETS:
        K, n, P, kind = grid
        lo, cdfs = make_cdfs(O, K, n, P, kind)
        _SETS[grid] = (lo, cdfs, B.TableSet.from_cdfs(cdfs, lo, P))
    return _SETS[grid]


def batch(B, O, grid, form, lengths, every, seed=0):
    """streams of `lengths` by make_ragged, encoded by the device's encoder with a jump point every `every` symbols (0: none); built
    once, never modified"""
    key = (grid, form, tuple(lengths), every, seed)
    if key not in _BATCHES:
        K, n, P, _ = grid
        coder, dtype = form
        lo, cdfs, tables = tables_of(B, O, grid)
        syms, idxs = make_ragged(lengths, K, n, P, lo, cdfs, 900 + seed + P + len(lengths))
        d_idx, d_off = dev_indices(flat(idxs), INDEX_DTYPES[dtype]), dev(offsets_of(lengths))
        enc = getattr(B, f"{coder}_encode_indexed_ragged")(dev(flat(syms)), d_idx, d_off, tables, (32, 64, P), jump_every=every)
        assert (enc.jump is not None) == (every != 0) and int(enc.status.abs().sum()) == 0
        _BATCHES[key] = Batch(coder, dtype, every, K, syms, idxs, d_idx, d_off, tables, enc)
    return _BATCHES[key]


def select(B, bt, queries, whole=False, idx=None, enc=None, out=None):
    """one select call; queries = [(stream, first, count)]; whole = True sends them as whole streams (first = count = None)"""
    sel = getattr(B, f"{bt.coder}_decode_indexed_ragged_select")
    streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int64, device="cuda")
    args = (bt.enc if enc is None else enc, bt.d_idx if idx is None else idx, bt.d_off, bt.tables, streams)
    if whole:
        assert all(f == 0 and c == len(bt.syms[s]) for s, f, c in queries)
        got = sel(*args, out=out)
    else:
        got = sel(*args, [f for _, f, _ in queries], [c for _, _, c in queries], out=out)
    if queries:
        assert B.last_kernel() == kernel(bt.coder)
    return got


def expected(syms, queries):
    parts = [np.asarray(syms[s][f: f + c], dtype=np.int32) for s, f, c in queries]
    offsets = np.concatenate([[0], np.cumsum([c for _, _, c in queries])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


def check(B, bt, queries, syms=None, **kw):
    got, out_offsets, status = select(B, bt, queries, **kw)
    want, want_offsets = expected(bt.syms if syms is None else syms, queries)
    assert got.dtype == torch.int32 and out_offsets.dtype == torch.int64 and status.dtype == torch.int32
    assert out_offsets.cpu().tolist() == want_offsets.tolist()
    status = status.cpu().numpy()
    assert (status == OK).all(), f"query {int(np.flatnonzero(status)[0])} = {queries[int(np.flatnonzero(status)[0])]}: status {status[status != 0][0]}"
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        q = int(np.searchsorted(want_offsets, k, side="right")) - 1
        raise AssertionError(f"query {q} = {queries[q]}: symbol {k - want_offsets[q]} of its slice differs")
    return got


def random_queries(rng, syms, n_queries):
    queries = []
    for _ in range(n_queries):
        s = int(rng.integers(0, len(syms)))
        first = int(rng.integers(0, len(syms[s]) + 1))
        queries.append((s, first, int(rng.integers(0, len(syms[s]) - first + 1))))
    return queries


# ---- 1. every range of one document ----

@pytest.mark.parametrize("grid,L,every", [(G12, 38, 0), (G24, 38, 16), (G16, 70, 32)], ids=["K2-P12-L38-I0", "K64-P24-L38-I16", "K64-P16-L70-I32"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_every_range_of_one_document(B, O, form, grid, L, every):
    """EVERY (first, count) with count >= 1 of one document, shuffled, in one call (741 resp. 2485 queries), and a few empty ranges.  The
    document sits behind a stream of 5 + r symbols, r = 0 .. 3: its uint8 row starts at byte residues 1, 2, 3, 0, and with it every
    piece's.  `skip` and `skip + count` take every residue mod 4, 8 and 16; pieces are a chunk's head, a whole chunk and a tail."""
    for r in range(4):
        bt = batch(B, O, grid, form, [5 + r, L, 1, 0], every)
        assert int(bt.d_off[1]) % 4 == (1 + r) % 4 and bt.d_idx.data_ptr() % 4 == 0
        queries = [(1, first, count) for first in range(L) for count in range(1, L - first + 1)]
        assert len(queries) == L * (L + 1) // 2
        order = np.random.default_rng(every + r).permutation(len(queries))
        check(B, bt, [queries[k] for k in order])
        check(B, bt, [(2, 0, 1), (3, 0, 0), (2, 1, 0), (1, L, 0), (1, 17, 0), (0, 0, 5 + r), (1, 0, L), (0, 3, 0)])


# ---- 2. the oracle's words and the oracle's table ----

@pytest.mark.parametrize("case", [RAGGED_CASES[1], RAGGED_CASES[4]], ids=["K2-n64-P12-I32", "K64-n255-P24-I32"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_the_oracles_words_and_the_oracles_table(B, O, form, case):
    """words, counts and jump table of the CPU restatement (one oracle coder per stream, coded chunk by chunk), packed by
    tests/test_gpu_indexed_ragged.py: whole streams, ranges that start mid-chunk, with and without the table"""
    coder, dtype = form
    n_streams, K, n, P, _, every = case
    lo, cdfs, lengths, syms, idxs, tm = workload(O, case)
    want = oracle_expected(O, case, coder)
    tables = table_set(B, case, lo, cdfs)
    d_idx = dev_indices(flat(idxs), INDEX_DTYPES[dtype], shift=3)
    enc = oracle_ragged_batch(B, coder, P, want, every)
    bt = Batch(coder, dtype, every, K, syms, idxs, d_idx, dev(offsets_of(lengths)), tables, enc)
    rng = np.random.default_rng(n_streams)
    whole = [(s, 0, lengths[s]) for s in range(n_streams)]
    mid = []
    for s in range(n_streams):
        if lengths[s] >= 2:
            first = int(rng.integers(1, lengths[s]))
            first += 1 if first % every == 0 and first + 1 < lengths[s] else 0
            mid.append((s, first, int(rng.integers(1, lengths[s] - first + 1))))
    assert sum(f % every != 0 for _, f, _ in mid) >= len(mid) - 4 and any(f // every != (f + c - 1) // every for _, f, c in mid)
    for e in (enc, without_jump(B, enc)):
        check(B, bt, whole, whole=True, enc=e)
        check(B, bt, mid, enc=e)


# ---- the C calls themselves ----

def raw_select(B, bt, queries, sizes=None, pieces=None, enc=None, slabs=False, capacity_short=0, idx=None):
    """The C call with hand-made arrays: `queries` are (stream, first, count) of unsigned integers sent as they are; query q owns
    sizes[q] (default: count) symbols of an output pre-filled with FILL between two margins of FILL; `pieces`: the piece counts behind
    d_piece_offsets (default: the Python layer's formula).  slabs: the words re-packed into slabs `stride` words apart (d_word_offsets =
    NULL, stride the largest word count), words_capacity exact less `capacity_short`.
    Returns (output without margins, both margins, out_offsets on the host, status on the host)."""
    from constriction_amd import _native as N
    L = N.lib()
    enc = bt.enc if enc is None else enc
    idx = bt.d_idx if idx is None else idx
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
    total, n_pieces = int(out_offsets[-1]), int(piece_offsets.max()) + 3          # (an upper bound of the pieces)
    guard = torch.full((total + 2 * MARGIN,), FILL, dtype=torch.int32, device="cuda")
    body = guard[MARGIN: MARGIN + total]
    status = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    d_out_offsets, d_piece_offsets = dev(out_offsets), dev(piece_offsets)
    p = lambda t: C.c_void_p(t.data_ptr())
    n = bt.d_off.numel() - 1
    if slabs:
        w, wo, nw = enc.words.cpu().numpy(), enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
        stride = int(nw.max())
        packed = np.full(n * stride, 0x5A5A5A5A, dtype=np.int32)
        for s in range(n):
            packed[s * stride: s * stride + nw[s]] = w[wo[s]: wo[s] + nw[s]]
        words = dev(packed)
        words_block = (p(words), None, stride, words.numel() - capacity_short, p(enc.n_words))
    else:
        words_block = (p(enc.words), p(enc.word_offsets), 0, enc.words.numel() - capacity_short, p(enc.n_words))
    j = enc.jump
    if j is None:
        table = (0, None, 0, None, None) if bt.coder == "ans" else (0, None, 0, None, None, None)
    else:
        arrays = (j.pos, j.state) if bt.coder == "ans" else (j.pos, j.lower, j.range)
        table = (interval, p(j.chunk_offsets), j.pos.numel(), *(p(t) for t in arrays))
    name = f"cst_{bt.coder}_decode_indexed_ragged_select"
    scratch = torch.empty(L.cst_persymbol_ragged_select_scratch_bytes(n_pieces), dtype=torch.uint8, device="cuda")
    N.check(getattr(L, name)(N.CoderConfig(*enc.config), bt.tables._h, *words_block, p(idx), idx.element_size(), p(bt.d_off), n, *table,
                             p(streams), p(first), p(count), nq, p(d_piece_offsets), n_pieces, p(body) if total else p(guard), p(d_out_offsets),
                             p(scratch), p(status), None), name)
    assert B.last_kernel() == kernel(bt.coder)
    torch.cuda.synchronize()
    return body.cpu().numpy(), torch.cat([guard[:MARGIN], guard[MARGIN + total:]]).cpu().numpy(), out_offsets, status.cpu().numpy()


def check_raw(result, syms, queries, bad=()):
    """queries in `bad` report INVALID_DATA and their slices still hold FILL; the others hold the input's slices; the margins hold FILL"""
    body, margins, out_offsets, status = result
    assert (margins == FILL).all()
    assert status.tolist() == [INVALID if q in bad else OK for q in range(len(queries))]
    for q, (s, f, c) in enumerate(queries):
        piece = body[out_offsets[q]: out_offsets[q + 1]]
        if q in bad:
            assert (piece == FILL).all(), f"query {q} = {queries[q]} was refused and wrote"
        else:
            assert piece.tolist() == syms[s][f: f + c].tolist(), f"query {q} = {queries[q]}"


SMALL_LENGTHS = [int(x) for x in np.random.default_rng(3).integers(50, 300, 12)]


# ---- 3. nothing outside a query's slice ----

@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_nothing_outside_a_querys_slice(B, O, form, every):
    """An `out` 64 elements longer than the total keeps its tail; through the C call, every refused query between two accepted ones
    leaves its slice untouched while its neighbours are exact: no such stream, first + count beyond the stream, a 64-bit wrap, an output
    slice or a piece count of the wrong length, piece offsets that run backwards, a jump_pos beyond the stream's words, a table slice that
    does not describe its stream."""
    bt = batch(B, O, G16, form, SMALL_LENGTHS, every)
    syms, n = bt.syms, len(bt.syms)
    good = [(0, 0, len(syms[0])), (3, 5, 20), (5, 33, 17), (3, len(syms[3]) - 1, 1), (1, 0, 0), (7, 49, 1)]
    total = sum(c for _, _, c in good)
    out = torch.full((total + 64,), FILL, dtype=torch.int32, device="cuda")
    got, _, _ = select(B, bt, good, out=out)
    assert got.cpu().tolist() == expected(syms, good)[0].tolist() and bool((out[total:] == FILL).all())
    T = next(s for s in range(1, n - 1) if len(syms[s]) >= 140)
    LT = len(syms[T])
    queries, bad = [good[0]], set()
    for q in [(n, 0, 5), (0xffffffff, 0, 5), (T, LT + 1, 0), (T, LT, 1), (T, LT - 3, 4), (T, (1 << 64) - 1, 2), (T, 2, (1 << 64) - 1),
              (T, 1 << 63, 1 << 63)]:
        bad.add(len(queries))
        queries.append(q)
        queries.append(good[len(queries) % len(good)])
    sizes = [min(c, 6) if q in bad else c for q, (_, _, c) in enumerate(queries)]
    check_raw(raw_select(B, bt, queries, sizes=sizes), syms, queries, bad)
    # an output slice that is not `count` long; a piece count that is off by one, either way
    sizes = [c for _, _, c in good]
    sizes[1] -= 1
    check_raw(raw_select(B, bt, good, sizes=sizes), syms, good, {1})
    right = B._select_piece_counts(torch.tensor([f for _, f, _ in good]), torch.tensor([c for _, _, c in good]), every).tolist()
    for q, delta in ((1, 1), (2, -1), (4, 1)):
        wrong = list(right)
        wrong[q] += delta
        check_raw(raw_select(B, bt, good, pieces=wrong), syms, good, {q})
    # piece offsets that do not ascend: the last query's end lies in front of its start (behind it no query's pieces are displaced)
    wrong = list(right)
    wrong[-1] = -1
    check_raw(raw_select(B, bt, good, pieces=wrong), syms, good, {len(good) - 1})
    if every:
        # a jump_pos entry above its stream's n_words: the queries that touch that entry, and they alone
        co = bt.enc.jump.chunk_offsets.cpu().numpy()
        assert co[T + 1] - co[T] >= 3
        pos = bt.enc.jump.pos.clone()
        pos[int(co[T]) + 1] = int(bt.enc.n_words[T]) + 1
        broken = dataclasses.replace(bt.enc, jump=dataclasses.replace(bt.enc.jump, pos=pos))
        queries = [(T, 0, 64), (T, 0, 65), (T, 64, 1), (T, 10, LT - 10), (T, 63, 1), (0, 0, len(syms[0])), (T, 0, 10), (T, 128, LT - 128)]
        check_raw(raw_select(B, bt, queries, enc=broken), syms, queries, {1, 2, 3})
        # the chunk offset of stream T + 1 one too large: stream T is given a chunk too many, stream T + 1 one too few -- their
        # queries are refused whatever they ask for, the others decode
        shifted = bt.enc.jump.chunk_offsets.clone()
        shifted[T + 1] += 1
        broken = dataclasses.replace(bt.enc, jump=dataclasses.replace(bt.enc.jump, chunk_offsets=shifted))
        others = [s for s in range(n) if s not in (T, T + 1)]
        U, V = others[0], others[-1]
        queries = [(U, 1, 40), (T, 0, 10), (V, 3, 30), (T + 1, 5, 1), (U, 0, len(syms[U])), (T, 70, 3), (V, 0, len(syms[V]))]
        check_raw(raw_select(B, bt, queries, enc=broken), syms, queries, {1, 3, 5})


# ---- 4. only the touched indices matter ----

@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_only_the_touched_indices_matter(B, O, form, every):
    """An index that names no table (uint8: 255; int32: a large value and -1) everywhere outside [the jump point in front of first,
    first + count) of the queries, behind a query's end in the same chunk and group too: the same symbols, status OK.  One such index
    INSIDE the dropped part of one query, then inside its stored part: that query alone reports INVALID_DATA, and nothing outside its
    slice has changed."""
    coder, dtype = form
    bt = batch(B, O, G24 if every else G12, form, SMALL_LENGTHS, every)
    syms = bt.syms
    assert bt.K < 255
    rng = np.random.default_rng(17 + every)
    queries = [(1, 23, 9), (4, 0, 0), (6, 37, 0)]
    for s in (2, 3, 5, 8, 8, 9, 10):
        first = int(rng.integers(1, len(syms[s]) - 1))
        queries.append((s, first, int(rng.integers(1, min(40, len(syms[s]) - first) + 1))))
    offs = bt.d_off.cpu().numpy()
    start = lambda f: f // every * every if every else 0
    touched = np.zeros(int(offs[-1]), dtype=bool)
    for s, f, c in queries:
        if c > 0:
            touched[offs[s] + start(f): offs[s] + f + c] = True
    assert 0 < touched.sum() < touched.size and not touched[0]
    mask = dev(~touched)
    clean = check(B, bt, queries)
    s, f, c = queries[0]
    assert f - start(f) >= 2 and all(q[0] != s for q in queries[1:])
    want, want_offsets = expected(syms, queries)
    for value in ((255,) if dtype == "u8" else (0x7fffffff, -1, bt.K)):
        idx = torch.where(mask, torch.full_like(bt.d_idx, value), bt.d_idx)
        assert check(B, bt, queries, idx=idx).tolist() == clean.tolist()
        # ... and one in what query 0 decodes and drops, then in what it stores (its neighbours in the list do not touch stream 1)
        for at in (start(f) + (f - start(f)) // 2, f + c // 2):
            idx2 = idx.clone()
            idx2[int(offs[s]) + at] = value
            out = torch.full((want.size + 64,), FILL, dtype=torch.int32, device="cuda")
            got, out_offsets, status = select(B, bt, queries, idx=idx2, out=out)
            assert status.cpu().tolist() == [INVALID] + [OK] * (len(queries) - 1), at
            assert out_offsets.cpu().tolist() == want_offsets.tolist()
            assert out[c:want.size].cpu().tolist() == want[c:].tolist() and bool((out[want.size:] == FILL).all())


# ---- 5. shapes of the launch ----

SHAPE_LENGTHS = [0, 200, 1, 199] + [int(x) for x in np.random.default_rng(5).integers(0, 60, 35)] + [701]


@pytest.mark.parametrize("n_queries", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_shapes_of_the_launch(B, O, form, every, n_queries):
    """partial last waves and workgroups in every pass (a thread per query, a lane per piece), one long stream among short ones and a
    stream of length 0, neighbouring lanes with very different skip + len, repeats and overlaps"""
    bt = batch(B, O, G16 if form[0] == "ans" else G24, form, SHAPE_LENGTHS, every)
    rng = np.random.default_rng(n_queries + every)
    queries = random_queries(rng, bt.syms, n_queries)
    queries[n_queries // 2] = (len(SHAPE_LENGTHS) - 1, 3, 690)
    check(B, bt, queries)


# ---- 6. whole streams ----

WHOLE_LENGTHS = [1, 600, 255, 256, 257, 512, 513] + [int(x) for x in np.random.default_rng(6).integers(1, 601, 17)]


@pytest.mark.parametrize("every", [0, 256])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_whole_streams(B, O, form, every):
    """first = count = None: every stream equals its row of the full decode of the same batch (and the input); all streams in order are
    the full decode's flat output"""
    bt = batch(B, O, G16, form, WHOLE_LENGTHS, every)
    full, full_status = getattr(B, f"{bt.coder}_decode_indexed_ragged")(bt.enc, bt.d_idx, bt.d_off, bt.tables)
    assert int(full_status.abs().sum()) == 0 and np.array_equal(full.cpu().numpy(), flat(bt.syms))
    n = len(bt.syms)
    order = [int(s) for s in np.random.default_rng(1).permutation(n)] + [1, 1]
    got, out_offsets, status = select(B, bt, [(s, 0, len(bt.syms[s])) for s in order], whole=True)
    assert int(status.abs().sum()) == 0
    got, oo, offs = got.cpu().numpy(), out_offsets.cpu().numpy(), bt.d_off.cpu().numpy()
    full = full.cpu().numpy()
    for q, s in enumerate(order):
        assert np.array_equal(got[oo[q]: oo[q + 1]], full[offs[s]: offs[s + 1]]), f"stream {s}"
    got, out_offsets, status = select(B, bt, [(s, 0, len(bt.syms[s])) for s in range(n)], whole=True)
    assert np.array_equal(got.cpu().numpy(), full) and torch.equal(out_offsets, bt.d_off) and int(status.abs().sum()) == 0


# ---- 7. the same queries with and without the table ----

@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_independence_from_the_table(B, O, form):
    """the same queries on the same words with and without `encoded.jump`: identical symbols"""
    bt = batch(B, O, G24, form, SHAPE_LENGTHS, 64)
    queries = random_queries(np.random.default_rng(9), bt.syms, 100)
    with_table = check(B, bt, queries)
    without = check(B, bt, queries, enc=without_jump(B, bt.enc))
    assert np.array_equal(with_table, without)


# ---- 8. the C ABI: slabs, and a capacity one word short ----

@pytest.mark.parametrize("every", [0, 32])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_c_abi_with_slabs_and_a_short_capacity(B, O, form, every):
    """the C entry points with d_word_offsets = NULL: stream s owns words[s * stride_words .. + stride_words), words_capacity exact;
    then one word short: the last stream fills its slab, its slice leaves the capacity and its queries report INVALID_DATA, the others
    are exact.  cst_last_kernel_name is the coder's (asserted in raw_select)."""
    lengths = [0, 1, 31, 32, 33, 64, 65, 96, 17, 200]
    bt = batch(B, O, G24, form, lengths, every)
    nw = bt.enc.n_words.cpu().numpy()
    assert nw[9] == nw.max() and (nw[:9] < nw[9]).all()
    queries = [(9, 0, 200), (9, 199, 1), (9, 31, 70), (6, 1, 64), (5, 0, 64), (4, 32, 1), (1, 0, 1), (0, 0, 0), (7, 95, 1), (8, 3, 14), (2, 30, 1)]
    check_raw(raw_select(B, bt, queries, slabs=True), bt.syms, queries)
    check_raw(raw_select(B, bt, queries, slabs=True, capacity_short=1), bt.syms, queries, {0, 1, 2})
    # the same with offsets: the last slab of the packed words ends where the buffer ends, or the check has nothing to say
    wo = bt.enc.word_offsets.cpu().numpy()
    last = max(s for s in range(len(lengths)) if nw[s] > 0)
    short = bt.enc.words.numel() - int(wo[last] + nw[last]) + 1
    hit = {q for q, (s, _, _) in enumerate(queries) if s == last}
    check_raw(raw_select(B, bt, queries, capacity_short=short), bt.syms, queries, hit)


# ---- 9. maximum word rate ----

@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_maximum_word_rate(B, O, form):
    """P = 24 and every coded symbol of probability 1 (24 bits each: three words per four symbols), a jump point every 16; ranges that
    start at 16 k + 15 and span three chunks: fifteen dropped symbols take eleven words before the first stored one, and the range
    coder's seek re-reads its point at the jump point.  The word window's lookahead runs at its fullest."""
    coder, dtype = form
    K, n, P, every = 2, 64, 24, 16
    lo = -(n // 2)
    cdfs = np.stack([O.GaussianModel(lo, lo + n - 1, m, 0.05, P).cdf_table() for m in (-3.0, 7.0)])
    prob = np.diff(cdfs.astype(np.int64), axis=1)
    assert sorted(prob[0].tolist()) == [1] * (n - 1) + [(1 << P) - (n - 1)]
    rng = np.random.default_rng(24)
    lengths = [100, 257] * 8 + [100]
    syms, idxs = [], []
    for length in lengths:
        idx = rng.integers(0, K, length)
        sym = rng.integers(0, n, length)
        sym = np.where(prob[idx, sym] == 1, sym, (sym + 1) % n)
        assert (prob[idx, sym] == 1).all()
        syms.append((sym + lo).astype(np.int32))
        idxs.append(idx.astype(np.int32))
    tables = B.TableSet.from_cdfs(cdfs, lo, P)
    d_idx, d_off = dev_indices(flat(idxs), INDEX_DTYPES[dtype], 1), dev(offsets_of(lengths))
    enc = getattr(B, f"{coder}_encode_indexed_ragged")(dev(flat(syms)), d_idx, d_off, tables, (32, 64, P), jump_every=every)
    assert int(enc.status.abs().sum()) == 0 and int(enc.n_words.max()) >= 257 * P // 32
    bt = Batch(coder, dtype, every, K, syms, idxs, d_idx, d_off, tables, enc)
    queries = []
    for s, length in enumerate(lengths):
        for k in range((length - 15) // 16):
            first = 16 * k + 15
            count = min(int(rng.integers(18, 34)), length - first)
            if count >= 18:
                assert first // 16 + 2 == (first + count - 1) // 16
                queries.append((s, first, count))
    assert len(queries) > 100
    with_table = check(B, bt, queries)
    assert np.array_equal(with_table, check(B, bt, queries, enc=without_jump(B, enc)))
