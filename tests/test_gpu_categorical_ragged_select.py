"""GPU tests of random access into ragged per-symbol Categorical batches, both quantisers and both coders:
batched.{ans,range}_decode_categorical[_perfect]_ragged_select and the C entry points behind them.

The expected symbols are always slices of the INPUT symbols (exact integers, no tolerance): the batches are encoded with
batched.*_categorical[_perfect]_ragged(jump_every=...), whose words and tables tests/test_gpu_categorical_ragged.py and
tests/test_gpu_categorical_perfect_ragged.py pin to the CPU oracle.  No GPU result is the reference for another, except where a test
says that two GPU calls must agree.  The workloads are those two files' (only the symbols and the rows: no oracle model is built here;
every table is strictly increasing -- queries on and next to degenerate and refused rows are in tests/test_gpu_categorical_extremes.py);
a batch is encoded once per (coder, quantiser, preset, lengths, K, dtype, interval)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import test_gpu_categorical_perfect_ragged as TP
import test_gpu_categorical_ragged as TF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CODERS = ["ans", "range"]
CONFIGS = [(32, 64, 24), (16, 32, 12)]
QUANTISERS = ["fast", "perfect"]
OK, IMPOSSIBLE, CAPACITY, INVALID = 0, 1, 2, 3
FILL, MARGIN = 7777, 64                      # no symbol equals FILL: K <= 257
dev, offsets_of = TF.dev, TF.offsets_of
cfg_id = lambda c: "W%dS%dP%d" % c
WORKLOADS = {"fast": TF.workload, "perfect": TP.R.workload}
DTYPES = TF.DTYPES


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from constriction_amd import batched
    return batched


def calls(B, coder, quant):
    """(encode, full decode, select, the select call's kernel name)"""
    word = "categorical_perfect" if quant == "perfect" else "categorical"
    name = (f"{coder}_decode_categorical_perfect_ragged_by_rows<select>" if quant == "perfect"
            else f"{coder}_decode_categorical_ragged_kernel<select>")
    return (getattr(B, f"{coder}_encode_{word}_ragged"), getattr(B, f"{coder}_decode_{word}_ragged"),
            getattr(B, f"{coder}_decode_{word}_ragged_select"), name)


@dataclasses.dataclass
class Batch:
    coder: str
    quant: str
    cfg: tuple
    k: int
    every: int
    syms: list              # the input, per stream
    flat: object
    offsets: object
    probs: object
    enc: object


_BATCHES = {}


def batch(B, coder, quant, cfg, lengths, k, dtype, every):
    """the workload of the quantiser's own test file for `lengths`, encoded with a jump point every `every` symbols (0: none); built once"""
    key = (coder, quant, cfg, tuple(lengths), k, dtype, every)
    if key not in _BATCHES:
        sym, probs = WORKLOADS[quant](lengths, k, DTYPES[dtype], 31 * k + cfg[2] + len(lengths))
        off = offsets_of(lengths)
        flat, offsets, d_probs = dev(sym), dev(off), dev(probs)
        enc = calls(B, coder, quant)[0](flat, offsets, d_probs, cfg, jump_every=every)
        assert (enc.jump is not None) == (every != 0) and int(enc.status.abs().sum()) == 0
        _BATCHES[key] = Batch(coder, quant, cfg, k, every, [sym[off[s]: off[s + 1]] for s in range(len(lengths))], flat, offsets, d_probs, enc)
    return _BATCHES[key]


def select(B, bt, queries, whole=False, probs=None, enc=None, out=None):
    """one select call; queries = [(stream, first, count)]; whole = True sends them as whole streams (first = count = None)"""
    _, _, sel, name = calls(B, bt.coder, bt.quant)
    streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int64, device="cuda")
    args = (bt.enc if enc is None else enc, bt.offsets, bt.probs if probs is None else probs, streams)
    if whole:
        assert all(f == 0 and c == len(bt.syms[s]) for s, f, c in queries)
        got = sel(*args, out=out)
    else:
        got = sel(*args, [f for _, f, _ in queries], [c for _, _, c in queries], out=out)
    if queries:
        assert B.last_kernel() == name
    return got


def expected(syms, queries):
    parts = [np.asarray(syms[s][f: f + c], dtype=np.int32) for s, f, c in queries]
    offsets = np.concatenate([[0], np.cumsum([c for _, _, c in queries])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


def check(B, bt, queries, **kw):
    got, out_offsets, status = select(B, bt, queries, **kw)
    want, want_offsets = expected(bt.syms, queries)
    assert got.dtype == torch.int32 and out_offsets.dtype == torch.int64 and status.dtype == torch.int32
    assert out_offsets.cpu().tolist() == want_offsets.tolist()
    status = status.cpu().numpy()
    assert (status == OK).all(), f"query {int(np.flatnonzero(status)[0])} = {queries[int(np.flatnonzero(status)[0])]}: status {status[status != 0][0]}"
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        q = int(np.searchsorted(want_offsets, i, side="right")) - 1
        raise AssertionError(f"query {q} = {queries[q]}: symbol {i - want_offsets[q]} of its slice differs")
    return got


def random_queries(rng, syms, n):
    queries = []
    for _ in range(n):
        s = int(rng.integers(0, len(syms)))
        first = int(rng.integers(0, len(syms[s]) + 1))
        queries.append((s, first, int(rng.integers(0, len(syms[s]) - first + 1))))
    return queries


# fast: one column, a full staging chunk of 64, one over, three chunks; perfect: both sides of the quantiser's 64- and 256-slot
# capacities.  The dtypes alternate.  Interval 48 (pieces that are no power of two) once for the perfect quantiser: a wave tabulates a row.
SWEEP = ([("fast", k, dtype, every) for k, dtype in ((2, "f32"), (64, "f64"), (65, "f32"), (129, "f64")) for every in (0, 16, 48)] +
         [("perfect", k, dtype, every) for k, dtype in ((2, "f64"), (64, "f32"), (65, "f64"), (257, "f32")) for every in (0, 16)] +
         [("perfect", 65, "f64", 48)])


@pytest.mark.parametrize("quant,k,dtype,every", SWEEP, ids=lambda v: str(v))
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", CODERS)
def test_every_range_of_one_document(B, coder, cfg, quant, k, dtype, every):
    """Three documents of 2 I + 5, 1 and 0 symbols (I = 16 where there is no table) and EVERY (first, count) with first + count <= len
    of the long one, empty ranges and first == len included, shuffled, in one call: 741 / 741 / 5253 queries.  `skip` and `skip + count`
    take every value a chunk allows; pieces are a chunk's head, a whole chunk and a tail."""
    I = every or 16
    L = 2 * I + 5
    bt = batch(B, coder, quant, cfg, [L, 1, 0], k, dtype, every)
    queries = [(0, first, count) for first in range(L + 1) for count in range(L - first + 1)]
    assert len(queries) == (741 if I == 16 else 5253)
    order = np.random.default_rng(every + k).permutation(len(queries))
    check(B, bt, [queries[i] for i in order])
    check(B, bt, [(1, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 0), (0, 0, L)])


@pytest.mark.parametrize("n_queries", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_many_pieces_per_wave_and_per_group(B, knob, coder, quant, every, n_queries):
    """70 streams of 0 .. 300 symbols, random ranges: partial last waves and workgroups in every pass (a thread per query, a lane or a
    wave per piece), neighbouring pieces with very different skip + len, repeats and overlaps.  The perfect pair twice more under a
    CST_PERFECT_RAGGED_BUDGET (words of tabulated rows per step; the host fills it with units first, then with positions): all pieces
    in steps of 7 positions -- coders parked between the steps, step ends inside `skip` -- and groups of 40 pieces in steps of one
    position."""
    k = 65
    bt = batch(B, coder, quant, (32, 64, 24), TP.PARITY_LENGTHS, k, "f32", every)
    queries = random_queries(np.random.default_rng(n_queries + every), bt.syms, n_queries)
    default = check(B, bt, queries)
    if quant == "perfect":
        # the units of the call: the Python layer's upper bound of the pieces
        n_units = sum(c for _, _, c in queries) // every + 2 * n_queries if every else n_queries
        for budget in (7 * n_units * (k + 1), 40 * (k + 1)):
            knob(CST_PERFECT_RAGGED_BUDGET=budget)
            assert np.array_equal(check(B, bt, queries), default), budget


SMALL_LENGTHS = [int(x) for x in np.random.default_rng(3).integers(50, 300, 12)]


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_only_the_touched_rows_matter(B, coder, quant, every):
    """NaN in every row outside [the jump point in front of first, first + count) of the queries: the same symbols and statuses.  Then
    one bad row INSIDE the dropped part of one query: that query reports IMPOSSIBLE_SYMBOL, its neighbours are exact, and the guard
    words in front of and behind the output are untouched (the slices lie back to back: the neighbours are the guards of each other)."""
    k = 9
    bt = batch(B, coder, quant, (32, 64, 24), SMALL_LENGTHS, k, "f64", every)
    syms = bt.syms
    rng = np.random.default_rng(17 + every)
    queries = [(4, 0, 0), (6, 37, 0)]
    for s in (2, 3, 5, 8, 8, 9, 10):
        first = int(rng.integers(1, len(syms[s]) - 1))
        queries.append((s, first, int(rng.integers(1, min(40, len(syms[s]) - first) + 1))))
    spoiled = 4
    queries.insert(spoiled, (1, 23, 9))
    offs = bt.offsets.cpu().numpy()
    start = lambda f: f // every * every if every else 0
    touched = np.zeros(int(offs[-1]), dtype=bool)
    for s, f, c in queries:
        if c > 0:
            touched[offs[s] + start(f): offs[s] + f + c] = True
    assert 0 < touched.sum() < touched.size and not touched[0]
    nan_rows = torch.where(dev(~touched)[:, None], torch.full_like(bt.probs, float("nan")), bt.probs)
    clean = check(B, bt, queries)
    assert check(B, bt, queries, probs=nan_rows).tolist() == clean.tolist()
    # ... and one bad row in what query `spoiled` decodes and drops (no other query touches its stream): a NaN, a negative entry
    s, f, c = queries[spoiled]
    assert f - start(f) >= 2 and all(q[0] != s for i, q in enumerate(queries) if i != spoiled)
    want, want_offsets = expected(syms, queries)
    lo, hi = int(want_offsets[spoiled]), int(want_offsets[spoiled + 1])
    for value in (float("nan"), -1.0):
        rows = nan_rows.clone()
        rows[int(offs[s]) + start(f) + (f - start(f)) // 2, k // 2] = value
        guard = torch.full((MARGIN + want.size + MARGIN,), FILL, dtype=torch.int32, device="cuda")
        got, out_offsets, status = select(B, bt, queries, probs=rows, out=guard[MARGIN:])
        assert status.cpu().tolist() == [IMPOSSIBLE if q == spoiled else OK for q in range(len(queries))]
        assert out_offsets.cpu().tolist() == want_offsets.tolist()
        body = guard[MARGIN: MARGIN + want.size].cpu().numpy()
        assert body[:lo].tolist() == want[:lo].tolist() and body[hi:].tolist() == want[hi:].tolist()
        assert bool((guard[:MARGIN] == FILL).all()) and bool((guard[MARGIN + want.size:] == FILL).all())


# ---- the C calls themselves ----

def raw_select(B, bt, queries, sizes=None, enc=None, slabs=False, n_total=None, max_piece=None):
    """The C call with hand-made arrays: `queries` are (stream, first, count) of unsigned integers sent as they are; query q owns
    sizes[q] (default: count) symbols of an output pre-filled with FILL between two margins of FILL.  slabs: the words re-packed into
    slabs `stride` words apart (d_word_offsets = NULL), words_capacity exact.  n_total: the rows the call is told of (default: all);
    max_piece: the perfect pair's max_piece_len (default: the interval, or the longest document).
    Returns (output without margins, both margins, out_offsets on the host, status on the host)."""
    from constriction_amd import _native as N
    L = N.lib()
    coder, perfect = bt.coder, bt.quant == "perfect"
    enc = bt.enc if enc is None else enc
    u64 = lambda values: np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)
    nq = len(queries)
    streams = dev(np.array([s for s, _, _ in queries], dtype=np.uint32).view(np.int32))
    first, count = dev(u64(f for _, f, _ in queries)), dev(u64(c for _, _, c in queries))
    sizes = [c for _, _, c in queries] if sizes is None else sizes
    interval = enc.jump.interval if enc.jump is not None else 0
    pieces = B._select_piece_counts(torch.tensor([f % (1 << 62) for _, f, _ in queries]), torch.tensor(sizes), interval).tolist()
    out_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    piece_offsets = np.concatenate([[0], np.cumsum(pieces)]).astype(np.int64)
    total, n_pieces = int(out_offsets[-1]), int(piece_offsets[-1]) + 3          # (an upper bound of the pieces)
    guard = torch.full((total + 2 * MARGIN,), FILL, dtype=torch.int32, device="cuda")
    body = guard[MARGIN: MARGIN + total]
    status = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    d_out_offsets, d_piece_offsets = dev(out_offsets), dev(piece_offsets)
    p = lambda t: C.c_void_p(t.data_ptr())
    n = bt.offsets.numel() - 1
    if slabs:
        w, wo, nw = enc.words.cpu().numpy(), enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
        stride = int(nw.max()) + 1
        packed = np.full(n * stride, 0x5A5A5A5A, dtype=np.int32)
        for s in range(n):
            packed[s * stride: s * stride + nw[s]] = w[wo[s]: wo[s] + nw[s]]
        words = dev(packed)
        words_block = (p(words), None, stride, words.numel(), p(enc.n_words))
    else:
        words_block = (p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words))
    j = enc.jump
    if j is None:
        table = (0, None, 0, None, None) if coder == "ans" else (0, None, 0, None, None, None)
    else:
        arrays = (j.pos, j.state) if coder == "ans" else (j.pos, j.lower, j.range)
        table = (interval, p(j.chunk_offsets), j.pos.numel(), *(p(t) for t in arrays))
    model = (p(bt.probs), bt.probs.element_size(), bt.k, int(bt.probs.shape[0]) if n_total is None else n_total)
    if perfect:
        model += ((interval or max(len(s) for s in bt.syms)) if max_piece is None else max_piece,)
    name = f"cst_{coder}_decode_categorical_{'perfect_' if perfect else ''}ragged_select"
    scratch = torch.empty(L.cst_persymbol_ragged_select_scratch_bytes(n_pieces), dtype=torch.uint8, device="cuda")
    N.check(getattr(L, name)(N.CoderConfig(*enc.config), *words_block, *model, p(bt.offsets), n, *table, p(streams), p(first), p(count), nq,
                             p(d_piece_offsets), n_pieces, p(body) if total else p(guard), p(d_out_offsets), p(scratch), p(status), None), name)
    assert B.last_kernel() == calls(B, coder, bt.quant)[3]
    torch.cuda.synchronize()
    return body.cpu().numpy(), torch.cat([guard[:MARGIN], guard[MARGIN + total:]]).cpu().numpy(), out_offsets, status.cpu().numpy()


def check_raw(result, syms, queries, bad=None):
    """queries in `bad` ({query: status}) report that status and their slices still hold FILL; the others hold the input's slices; the
    margins hold FILL"""
    bad = bad or {}
    body, margins, out_offsets, status = result
    assert (margins == FILL).all()
    assert status.tolist() == [bad.get(q, OK) for q in range(len(queries))]
    for q, (s, f, c) in enumerate(queries):
        piece = body[out_offsets[q]: out_offsets[q + 1]]
        if q in bad:
            assert (piece == FILL).all(), f"query {q} = {queries[q]} was refused and wrote"
        else:
            assert piece.tolist() == syms[s][f: f + c].tolist(), f"query {q} = {queries[q]}"


@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_refused_queries_between_accepted_ones(B, coder, quant, every):
    """Behind a guarded output, every refused query between two accepted ones gets its own status and leaves its slice untouched while
    its neighbours are exact: no such stream, first > len, count > len - first, a 64-bit wrap; a stream whose rows reach beyond
    n_total; for the perfect pair a piece above max_piece_len."""
    bt = batch(B, coder, quant, (32, 64, 24), SMALL_LENGTHS, 9, "f64", every)
    syms, n = bt.syms, len(bt.syms)
    good = [(0, 0, len(syms[0])), (3, 5, 20), (5, 33, 17), (3, len(syms[3]) - 1, 1), (1, 0, 0), (7, 49, 1)]
    T = next(s for s in range(1, n - 1) if len(syms[s]) >= 140)
    LT = len(syms[T])

    def between(refused, good=good):
        queries, bad = [good[0]], {}
        for q, status in refused:
            bad[len(queries)] = status
            queries.append(q)
            queries.append(good[len(queries) % len(good)])
        return queries, bad, [min(c, 6) if q in bad else c for q, (_, _, c) in enumerate(queries)]

    queries, bad, sizes = between([(q, INVALID) for q in [(n, 0, 5), (0xffffffff, 0, 5), (T, LT + 1, 0), (T, LT, 1), (T, LT - 3, 4),
                                                          (T, (1 << 64) - 1, 2), (T, 2, (1 << 64) - 1), (T, 1 << 63, 1 << 63)]])
    check_raw(raw_select(B, bt, queries, sizes=sizes), syms, queries, bad)
    # the matrix is told to be one row short: the last stream's rows reach beyond it, wherever in that stream a query lies (its first
    # chunk is inside the rows there are); every other stream decodes
    last, n_total = n - 1, int(bt.offsets[-1]) - 1
    assert len(syms[last]) > 70 and all(q[0] != last for q in good)
    queries, bad, sizes = between([(q, INVALID) for q in [(last, 0, 3), (last, len(syms[last]) - 2, 2), (last, 10, 0), (last, 0, len(syms[last]))]])
    sizes = [c for _, _, c in queries]
    check_raw(raw_select(B, bt, queries, sizes=sizes, n_total=n_total), syms, queries, bad)
    if quant == "perfect":
        # max_piece_len 40: without a table a piece is first + count symbols; with one (I = 64) it is first % I + count, or I for a
        # query that goes on into the next chunk -- refused as a whole, the pieces that would fit included
        over = [(T, 10, 31), (T, 0, 41), (T, 40, 1)] if every == 0 else [(T, 64 + 10, 31), (T, 64, 41), (T, 60, 10), (T, 0, 100)]
        fits = [(T, 10, 30), (T, 0, 40), (T, 39, 1)] if every == 0 else [(T, 64 + 10, 30), (T, 64, 40), (T, 64 + 39, 1)]
        fits.append((T, 100, 0))                      # (an empty query has no piece, however deep it lies)
        queries, bad, _ = between([(q, CAPACITY) for q in over], [(0, 0, 40), (3, 5, 20), (5, 33, 7), (1, 0, 0), (7, 39, 1)])
        queries += fits
        check_raw(raw_select(B, bt, queries, max_piece=40), syms, queries, bad)


WHOLE_LENGTHS = [1, 300, 255, 256, 257, 0, 64, 65] + [int(x) for x in np.random.default_rng(6).integers(1, 301, 12)]


@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_whole_documents(B, coder, quant):
    """first = count = None: every document is the input's; and, GPU against GPU, the full ragged decode's -- all documents in order are
    the full decode's flat output"""
    bt = batch(B, coder, quant, (32, 64, 24), WHOLE_LENGTHS, 5, "f32", 64)
    full, full_status = calls(B, coder, quant)[1](bt.enc, bt.offsets, bt.probs)
    assert int(full_status.abs().sum()) == 0 and torch.equal(full, bt.flat)
    n = len(bt.syms)
    order = [int(s) for s in np.random.default_rng(1).permutation(n)] + [1, 1]
    check(B, bt, [(s, 0, len(bt.syms[s])) for s in order], whole=True)
    got, out_offsets, status = select(B, bt, [(s, 0, len(bt.syms[s])) for s in range(n)], whole=True)
    assert torch.equal(got, full) and torch.equal(out_offsets, bt.offsets) and int(status.abs().sum()) == 0


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_independence_from_the_table(B, coder, quant, cfg):
    """the same queries on the same words with and without `encoded.jump`: the input's symbols both times"""
    bt = batch(B, coder, quant, cfg, TP.PARITY_LENGTHS, 17, "f32", 64)
    queries = random_queries(np.random.default_rng(9), bt.syms, 100)
    with_table = check(B, bt, queries)
    without = check(B, bt, queries, enc=dataclasses.replace(bt.enc, jump=None))
    assert np.array_equal(with_table, without)


@pytest.mark.parametrize("slabs", [False, True], ids=["word_offsets", "slabs"])
@pytest.mark.parametrize("every", [0, 32])
@pytest.mark.parametrize("quant", QUANTISERS)
@pytest.mark.parametrize("coder", CODERS)
def test_c_abi(B, coder, quant, every, slabs):
    """the C entry points with d_word_offsets, and with d_word_offsets = NULL: stream s owns words[s * stride_words .. + stride_words),
    words_capacity exact; cst_last_kernel_name is the quantiser's and the coder's (asserted in raw_select)"""
    bt = batch(B, coder, quant, (32, 64, 24), [0, 1, 31, 32, 33, 64, 65, 200, 96, 17], 65, "f64", every)
    queries = [(7, 0, 200), (7, 199, 1), (7, 31, 70), (6, 1, 64), (5, 0, 64), (4, 32, 1), (1, 0, 1), (0, 0, 0), (8, 95, 1), (9, 3, 14), (2, 30, 1)]
    check_raw(raw_select(B, bt, queries, slabs=slabs), bt.syms, queries)
