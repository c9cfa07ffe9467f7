"""GPU tests of random access into ragged per-symbol batches: batched.{ans,range}_decode_{gaussian,laplace,cauchy,family}_ragged_select
and the C entry points cst_{ans,range}_decode_{gaussian,family}_ragged_select.

The expected symbols are always slices of the INPUT symbols (exact integers, no tolerance): the batches are encoded with
batched.*_{gaussian,laplace,cauchy}_ragged(jump_every=...), whose words and tables tests/test_gpu_persymbol_ragged_jump.py pins to the
CPU oracle.  No GPU result is the reference for another, except where a test says that two GPU calls must agree.  Workload helpers are
those of tests/test_gpu_ragged_per_symbol_forms.py, as in the jump tests; a batch is built once per (form, preset, lengths, interval)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import test_gpu_ragged_per_symbol_forms as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = [(coder, family) for coder in ("ans", "range") for family in ("gaussian", "laplace", "cauchy")]
form_id, cfg_id = F.form_id, F.cfg_id
OK, IMPOSSIBLE, INVALID = 0, 1, 3
FILL, MARGIN = 7777, 64                      # no symbol of any support here equals FILL


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from constriction_amd import batched
    return batched


def calls(B, form):
    coder, family = form
    return (getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged"),
            getattr(B, f"{coder}_decode_{family}_ragged_select"), f"{coder}_decode_{family}_ragged_kernel<select>")


@dataclasses.dataclass
class Batch:
    form: tuple
    cfg: tuple
    every: int
    syms: list              # the input, per stream
    flat: object
    offsets: object
    a: object
    b: object
    enc: object
    lo: int
    hi: int


_BATCHES = {}


def batch(B, form, cfg, lengths, every, seed=0):
    """the streams of F.workload for `lengths`, encoded by `form` with a jump point every `every` symbols (0: none); built once"""
    key = (form, cfg, tuple(lengths), every, seed)
    if key not in _BATCHES:
        lo, hi = F.support(cfg[2])
        syms, locs, scales = F.workload(form[1], lengths, lo, hi, 4000 + seed + cfg[2] + len(lengths))
        flat, offsets, a, b = F.flatten(B, syms, locs, scales)
        enc = calls(B, form)[0](flat, offsets, lo, hi, a, b, cfg, jump_every=every)
        assert (enc.jump is not None) == (every != 0) and int(enc.status.abs().sum()) == 0
        _BATCHES[key] = Batch(form, cfg, every, syms, flat, offsets, a, b, enc, lo, hi)
    return _BATCHES[key]


def select(B, bt, queries, whole=False, a=None, b=None, enc=None, out=None):
    """one select call; queries = [(stream, first, count)]; whole = True sends them as whole streams (first = count = None)"""
    _, _, sel, name = calls(B, bt.form)
    streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int64, device="cuda")
    args = (bt.enc if enc is None else enc, bt.offsets, bt.lo, bt.hi, bt.a if a is None else a, bt.b if b is None else b, streams)
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
        k = int(np.flatnonzero(got != want)[0])
        q = int(np.searchsorted(want_offsets, k, side="right")) - 1
        raise AssertionError(f"query {q} = {queries[q]}: symbol {k - want_offsets[q]} of its slice differs")
    return got


SWEEP = [(form, (32, 64, 24)) for form in FORMS] + [((coder, "gaussian"), cfg) for coder in ("ans", "range") for cfg in ((32, 64, 12), (16, 32, 12))]


@pytest.mark.parametrize("every", [0, 16, 48])
@pytest.mark.parametrize("form,cfg", SWEEP, ids=lambda v: form_id(v) if isinstance(v[0], str) else cfg_id(v))
def test_every_range_of_one_document(B, form, cfg, every):
    """Three documents of 2 I + 5, 1 and 0 symbols (I = 16 where there is no table) and EVERY (first, count) with first + count <= len
    of the long one, empty ranges and first == len included, shuffled, in one call: 741 / 741 / 5253 queries.  `skip` and `skip + count`
    take every residue mod 4, 8 and 16; pieces are a chunk's head, a whole chunk and a tail."""
    I = every or 16
    L = 2 * I + 5
    bt = batch(B, form, cfg, [L, 1, 0], every)
    queries = [(0, first, count) for first in range(L + 1) for count in range(L - first + 1)]
    assert len(queries) == (741 if I == 16 else 5253)
    order = np.random.default_rng(every).permutation(len(queries))
    check(B, bt, [queries[k] for k in order])
    check(B, bt, [(1, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 0), (0, 0, L)])


# ---- the C calls themselves ----

def raw_select(B, bt, queries, sizes=None, pieces=None, enc=None, slabs=False):
    """The C call with hand-made arrays (tests/test_gpu_ragged_select.py::raw_select for the per-symbol calls): `queries` are (stream,
    first, count) of unsigned integers sent as they are; query q owns sizes[q] (default: count) symbols of an output pre-filled with
    FILL between two margins of FILL; `pieces`: the piece counts behind d_piece_offsets (default: the Python layer's formula).
    slabs: the words re-packed into slabs `stride` words apart (d_word_offsets = NULL), words_capacity exact.
    Returns (output without margins, both margins, out_offsets on the host, status on the host)."""
    from constriction_amd import _native as N
    L = N.lib()
    coder, family = bt.form
    enc = bt.enc if enc is None else enc
    u64 = lambda values: np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)
    nq = len(queries)
    streams = F.dev(np.array([s for s, _, _ in queries], dtype=np.uint32).view(np.int32))
    first, count = F.dev(u64(f for _, f, _ in queries)), F.dev(u64(c for _, _, c in queries))
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
    d_out_offsets, d_piece_offsets = F.dev(out_offsets), F.dev(piece_offsets)
    p = lambda t: C.c_void_p(t.data_ptr())
    n = bt.offsets.numel() - 1
    if slabs:
        w, wo, nw = enc.words.cpu().numpy(), enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
        stride = int(nw.max()) + 1
        packed = np.full(n * stride, 0x5A5A5A5A, dtype=np.int32)
        for s in range(n):
            packed[s * stride: s * stride + nw[s]] = w[wo[s]: wo[s] + nw[s]]
        words = F.dev(packed)
        words_block = (p(words), None, stride, words.numel(), p(enc.n_words))
    else:
        words_block = (p(enc.words), p(enc.word_offsets), 0, enc.words.numel(), p(enc.n_words))
    j = enc.jump
    if j is None:
        table = (0, None, 0, None, None) if coder == "ans" else (0, None, 0, None, None, None)
    else:
        arrays = (j.pos, j.state) if coder == "ans" else (j.pos, j.lower, j.range)
        table = (interval, p(j.chunk_offsets), j.pos.numel(), *(p(t) for t in arrays))
    fam = () if family == "gaussian" else (B.FAMILIES[family],)
    name = f"cst_{coder}_decode_{'gaussian' if family == 'gaussian' else 'family'}_ragged_select"
    scratch = torch.empty(L.cst_persymbol_ragged_select_scratch_bytes(n_pieces), dtype=torch.uint8, device="cuda")
    N.check(getattr(L, name)(N.CoderConfig(*enc.config), *fam, bt.lo, bt.hi, *words_block, p(bt.a), p(bt.b), p(bt.offsets), n, *table,
                             p(streams), p(first), p(count), nq, p(d_piece_offsets), n_pieces, p(body) if total else p(guard), p(d_out_offsets),
                             p(scratch), p(status), None), name)
    assert B.last_kernel() == f"{coder}_decode_{family}_ragged_kernel<select>"
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


@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_nothing_outside_a_querys_slice(B, coder, every):
    """An `out` 64 elements longer than the total keeps its tail; through the C call, every refused query between two accepted ones
    leaves its slice untouched while its neighbours are correct: no such stream, first > len, count > len - first, a 64-bit wrap, an
    output slice or a piece count of the wrong length, a jump_pos beyond the stream's words."""
    bt = batch(B, (coder, "gaussian"), (32, 64, 24), SMALL_LENGTHS, every)
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
    if every:
        # a jump_pos entry above its stream's n_words: the queries that touch that entry, and they alone
        co = bt.enc.jump.chunk_offsets.cpu().numpy()
        assert co[T + 1] - co[T] >= 3
        pos = bt.enc.jump.pos.clone()
        pos[int(co[T]) + 1] = int(bt.enc.n_words[T]) + 1
        broken = dataclasses.replace(bt.enc, jump=dataclasses.replace(bt.enc.jump, pos=pos))
        queries = [(T, 0, 64), (T, 0, 65), (T, 64, 1), (T, 10, LT - 10), (T, 63, 1), (0, 0, len(syms[0])), (T, 0, 10), (T, 128, LT - 128)]
        check_raw(raw_select(B, bt, queries, enc=broken), syms, queries, {1, 2, 3})


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_only_the_touched_parameters_matter(B, coder, every):
    """NaN in means / stds everywhere outside [the jump point in front of first, first + count) of the queries: the same symbols and
    statuses.  A NaN INSIDE the skipped part of one query: that query reports IMPOSSIBLE_SYMBOL, the others are right, and nothing
    outside its slice has changed."""
    bt = batch(B, (coder, "gaussian"), (32, 64, 24), SMALL_LENGTHS, every)
    syms = bt.syms
    rng = np.random.default_rng(17 + every)
    queries = [(1, 23, 9), (4, 0, 0), (6, 37, 0)]
    for s in (2, 3, 5, 8, 8, 9, 10):
        first = int(rng.integers(1, len(syms[s]) - 1))
        queries.append((s, first, int(rng.integers(1, min(40, len(syms[s]) - first) + 1))))
    offs = bt.offsets.cpu().numpy()
    start = lambda f: f // every * every if every else 0
    touched = np.zeros(int(offs[-1]), dtype=bool)
    for s, f, c in queries:
        if c > 0:
            touched[offs[s] + start(f): offs[s] + f + c] = True
    assert 0 < touched.sum() < touched.size and not touched[0]
    mask = F.dev(~touched)
    nan = torch.full_like(bt.a, float("nan"))
    a, b = torch.where(mask, nan, bt.a), torch.where(mask, nan, bt.b)
    clean = check(B, bt, queries)
    assert check(B, bt, queries, a=a, b=b).tolist() == clean.tolist()
    # ... and one NaN in what query 0 decodes and drops (its neighbours in the list do not touch stream 1)
    s, f, c = queries[0]
    assert f - start(f) >= 2 and all(q[0] != s for q in queries[1:])
    for arr in ("a", "b"):
        a2, b2 = a.clone(), b.clone()
        (a2 if arr == "a" else b2)[int(offs[s]) + start(f) + (f - start(f)) // 2] = float("nan")
        want, want_offsets = expected(syms, queries)
        out = torch.full((want.size + 64,), FILL, dtype=torch.int32, device="cuda")
        got, out_offsets, status = select(B, bt, queries, a=a2, b=b2, out=out)
        assert status.cpu().tolist() == [IMPOSSIBLE] + [OK] * (len(queries) - 1)
        assert out_offsets.cpu().tolist() == want_offsets.tolist()
        assert out[c:want.size].cpu().tolist() == want[c:].tolist() and bool((out[want.size:] == FILL).all())


SHAPE_LENGTHS = [0, 200, 1, 199] + [int(x) for x in np.random.default_rng(5).integers(0, 201, 36)]


@pytest.mark.parametrize("n_queries", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("every", [0, 64])
@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "laplace")], ids=form_id)
def test_shapes_of_the_launch(B, form, every, n_queries):
    """partial last waves and workgroups in every pass (a thread per query, a lane per piece), neighbouring lanes with very different
    skip + len, repeats and overlaps"""
    bt = batch(B, form, (32, 64, 24), SHAPE_LENGTHS, every)
    rng = np.random.default_rng(n_queries + every)
    queries = []
    for _ in range(n_queries):
        s = int(rng.integers(0, len(bt.syms)))
        first = int(rng.integers(0, len(bt.syms[s]) + 1))
        queries.append((s, first, int(rng.integers(0, len(bt.syms[s]) - first + 1))))
    check(B, bt, queries)


WHOLE_LENGTHS = [1, 600, 255, 256, 257, 512, 513] + [int(x) for x in np.random.default_rng(6).integers(1, 601, 17)]


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_whole_documents(B, form):
    """first = count = None: every document equals its row of the full decode of the same batch (and the input); all documents in order
    are the full decode's flat output"""
    bt = batch(B, form, (32, 64, 24), WHOLE_LENGTHS, 256)
    full, full_status = calls(B, form)[1](bt.enc, bt.offsets, bt.lo, bt.hi, bt.a, bt.b)
    assert int(full_status.abs().sum()) == 0 and torch.equal(full, bt.flat)
    n = len(bt.syms)
    order = [int(s) for s in np.random.default_rng(1).permutation(n)] + [1, 1]
    got, out_offsets, status = select(B, bt, [(s, 0, len(bt.syms[s])) for s in order], whole=True)
    assert int(status.abs().sum()) == 0
    got, oo, offs = got.cpu().numpy(), out_offsets.cpu().numpy(), bt.offsets.cpu().numpy()
    full = full.cpu().numpy()
    for q, s in enumerate(order):
        assert np.array_equal(got[oo[q]: oo[q + 1]], full[offs[s]: offs[s + 1]]), f"document {s}"
    got, out_offsets, status = select(B, bt, [(s, 0, len(bt.syms[s])) for s in range(n)], whole=True)
    assert np.array_equal(got.cpu().numpy(), full) and torch.equal(out_offsets, bt.offsets) and int(status.abs().sum()) == 0


@pytest.mark.parametrize("every", [0, 32])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_c_abi_with_slabs(B, form, every):
    """the C entry points with d_word_offsets = NULL: stream s owns words[s * stride_words .. + stride_words), words_capacity exact;
    cst_last_kernel_name is the family's and the coder's (asserted in raw_select)"""
    bt = batch(B, form, (32, 64, 24), [0, 1, 31, 32, 33, 64, 65, 200, 96, 17], every)
    queries = [(7, 0, 200), (7, 199, 1), (7, 31, 70), (6, 1, 64), (5, 0, 64), (4, 32, 1), (1, 0, 1), (0, 0, 0), (8, 95, 1), (9, 3, 14), (2, 30, 1)]
    check_raw(raw_select(B, bt, queries, slabs=True), bt.syms, queries)


@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "gaussian"), ("ans", "cauchy"), ("range", "laplace")], ids=form_id)
def test_independence_from_the_table(B, form):
    """the same queries on the same words with and without `encoded.jump`: identical symbols"""
    bt = batch(B, form, (32, 64, 24), SHAPE_LENGTHS, 64)
    rng = np.random.default_rng(9)
    queries = []
    for _ in range(100):
        s = int(rng.integers(0, len(bt.syms)))
        first = int(rng.integers(0, len(bt.syms[s]) + 1))
        queries.append((s, first, int(rng.integers(0, len(bt.syms[s]) - first + 1))))
    with_table = check(B, bt, queries)
    without = check(B, bt, queries, enc=dataclasses.replace(bt.enc, jump=None))
    assert np.array_equal(with_table, without)
