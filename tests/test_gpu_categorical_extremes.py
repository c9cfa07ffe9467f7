"""GPU tests of every per-symbol Categorical kernel -- both quantisers; ANS and range; rows, rectangular, ragged, jump points, select, the
drop-in coders -- on the ZOO of tests/categorical_extremes.py: rows whose sum is the smallest normal number, subnormal, just below
finfo.max or overflowing in the last column; rows whose scale is infinite (tables with EMPTY intervals, which stay non-decreasing) or
finite near finfo.max; mass in one column; negative zeros; entries over the whole exponent range; an empty last interval; and NaN,
negative and infinite entries in the first column, the first column of the second chunk and the last one.

The degenerate cases that the Dirichlet recipe of tests/test_gpu_categorical_{batch,ragged,ragged_select}.py keeps out are here.  Every
expected row, word, count, status and jump table comes from the CPU oracle (tests/categorical_extremes.py; tests/
test_categorical_extremes_cpu.py checks the zoo and the oracle's side without a GPU).  No GPU result is the reference for another:
where two GPU routes decode the same words, both must return the oracle's symbols.  What a stream that failed decodes to is not
specified and not asserted.  Bad rows and impossible symbols are in-band statuses and every buffer is sized by max_words /
range_max_words: nothing here can fault."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import categorical_extremes as Z
import categorical_perfect_rows as R
import test_gpu_per_symbol_extremes as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, IMPOSSIBLE = Z.OK, Z.IMPOSSIBLE
CODERS = ["ans", "range"]
QUANTS = [("fast", m) for m in Z.MODELS] + [("perfect", m) for m in Z.PERFECT_MODELS]
quant_id = lambda q: "%s-K%d-%s" % (q[0], *q[1])
LAYOUTS = ["stream_major", "symbol_major"]
FAST_ROUTES = {"fused": "{coder}_decode_categorical_lane_kernel", "rows": "decode_categorical_by_rows"}
dev, host_batch, host_ragged = X.dev, X.host_batch, X.host_ragged
NO_WORDS = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from constriction_amd import batched
    return batched


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native
    return _native.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------- a. the rows kernels

def device_rows(lib, quant, probs, P):
    """the raw entry points, so that a bad row comes back in-band: (rows, codes, moves or None)"""
    n, k = probs.shape
    d_probs = dev(probs)
    rows = torch.zeros((n, k + 1), dtype=torch.int32, device="cuda")
    bad = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    moves = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    if quant == "fast":
        rc = lib.cst_categorical_fast_cdf_rows(P, _ptr(d_probs), probs.itemsize, n, k, _ptr(rows), _ptr(bad), None)
    else:
        rc = lib.cst_categorical_perfect_cdf_rows(P, _ptr(d_probs), probs.itemsize, n, k, _ptr(rows), _ptr(bad), _ptr(moves), None)
    assert rc == 0
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint32), bad.cpu().numpy(), (moves.cpu().numpy().view(np.uint32) if quant == "perfect" else None)


@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [2, 5, 64, 65, 257, 300])
@pytest.mark.parametrize("quant", ["fast", "perfect"])
def test_rows_kernels_give_the_oracles_rows_and_codes(B, lib, quant, k, dtype, P):
    """every kind of the zoo, four times over (a whole wave of rows and a partial one; for the perfect quantiser a wave each): valid and
    degenerate rows are the oracle's, a refused row reads 0xffffffff, 2^P, ... with code 1 (and no moves); the moves are the host twin's"""
    z = Z.zoo(quant, k, dtype, P)
    kinds = list(z.rows) * 4
    assert len(kinds) > 64 and len(kinds) % 64
    probs = np.stack([z.rows[kind] for kind in kinds])
    rows, codes, moves = device_rows(lib, quant, probs, P)
    if quant == "perfect":
        assert B.last_kernel() == "categorical_perfect_kernel"
        _, _, want_moves = R.host_perfect(lib, probs, P)
    bad_row = [0xFFFFFFFF] + [1 << P] * k
    for r, kind in enumerate(kinds):
        refused = z.classes[kind] == "refused"
        assert codes[r] == (1 if refused else 0), (r, kind)
        assert rows[r].tolist() == (bad_row if refused else z.tables[kind].tolist()), (r, kind)
        if moves is not None:
            assert moves[r] == want_moves[r] and (moves[r] == 0 or not refused), (r, kind)
    # the Python call raises for the same rows, and tabulates the rest
    with pytest.raises(ValueError, match="not normalizable"):
        B.categorical_cdf_rows(dev(probs), P, perfect=quant == "perfect")
    accepted = [kind for kind in z.accepted]
    got = B.categorical_cdf_rows(dev(np.stack([z.rows[kind] for kind in accepted])), P, perfect=quant == "perfect")
    assert np.array_equal(got.cpu().numpy().view(np.uint32), np.stack([z.tables[kind] for kind in accepted]))


@pytest.mark.parametrize("k", [5, 64, 257])
def test_the_perfect_quantiser_refuses_in_f64_what_it_accepts_in_f32(lib, k):
    """min_normal_sum, inf_scale_equal, inf_scale_gaps: the f64 rows leave the quantiser through `extra > left` (a share beyond the weight
    that is left), the f32 rows of the same kinds are widened to f64 and are ordinary rows -- the oracle's"""
    kinds = ["min_normal_sum", "inf_scale_equal", "inf_scale_gaps"]
    for dtype, code in (("f32", 0), ("f64", 1)):
        z = Z.zoo("perfect", k, dtype, 24)
        rows, codes, moves = device_rows(lib, "perfect", np.stack([z.rows[kind] for kind in kinds]), 24)
        assert codes.tolist() == [code] * 3 and [z.classes[kind] == "refused" for kind in kinds] == [bool(code)] * 3
        for r, kind in enumerate(kinds):
            assert rows[r].tolist() == ([0xFFFFFFFF] + [1 << 24] * k if code else z.tables[kind].tolist()), (dtype, kind)


def test_device_log1p_at_the_perfect_quantisers_arguments(lib):
    """The perfect quantiser compares gains p log1p(1 / w) with losses -p log1p(-1 / w): log1p as the DEVICE evaluates it, at every
    argument a weight up to 2^16 gives and at 4096 larger ones up to 2^24, is the oracle's to the bit.  Its polynomial is the one
    place in the Categorical kernels where a product is followed by an addition, so this is what notices a build that lets the
    compiler contract them (the fast quantiser converts `cum * scale` and adds an INTEGER: nothing there can be fused)."""
    from oracle import oracle as O
    log1p = O.load().cst_oracle_log1p
    w = np.concatenate([np.arange(1, (1 << 16) + 1), np.random.default_rng(5).integers(1 << 16, (1 << 24) + 1, 4096)]).astype(np.float64)
    x = np.ascontiguousarray(np.concatenate([1.0 / w, -1.0 / w[1:]]))
    d_x = dev(x)
    out = torch.empty_like(d_x)
    assert lib.cst_debug_family_fn(1, _ptr(d_x), _ptr(out), x.size, None) == 0
    torch.cuda.synchronize()
    want = np.array([log1p(float(v)) for v in x])
    differ = np.flatnonzero(out.cpu().numpy().view(np.uint64) != want.view(np.uint64))
    assert differ.size == 0, f"{differ.size} of {x.size} arguments, the first: {x[differ[0]]!r}"


# ---------------------------------------------------------------------------------------------- b. the rectangular coders

def slab_words(B, coder, n_per, cfg):
    return (B.max_words if coder == "ans" else B.range_max_words)(n_per, cfg)


def in_layout(layout, *arrays):
    if layout == "symbol_major":
        return [dev(np.swapaxes(a, 0, 1)) for a in arrays]
    return [dev(a) for a in arrays]


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=Z.cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("quant", QUANTS, ids=quant_id)
def test_rectangular_coders(B, quant, coder, cfg, knob):
    """(70, 20), both layouts.  Encoder: exactly the streams that hold a refused row or code an empty interval report
    IMPOSSIBLE_SYMBOL, every other stream has the oracle's count and words.  Decoders: every route, on the encoder's batch and on slabs
    built on the host from the oracle's words -- status 0 and the input symbols for every stream that codes."""
    quant, (k, dtype) = quant
    perfect = quant == "perfect"
    bt, want = Z.expected("rect", quant, k, dtype, cfg)
    want = want[coder]
    sym, probs = bt.rect()
    good = np.array(bt.good)
    encode, decode = getattr(B, f"{coder}_encode_categorical"), getattr(B, f"{coder}_decode_categorical")
    host = host_batch(B, cfg, [NO_WORDS if w is None else w for w in want], slab_words(B, coder, Z.N_PER, cfg))
    routes = {"": "decode_categorical_perfect_by_rows"} if perfect else FAST_ROUTES
    for layout in LAYOUTS:
        d_sym, d_probs = in_layout(layout, sym, probs)
        enc = encode(d_sym, d_probs, cfg, layout, perfect=perfect)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_encode_categorical_{'perfect_' if perfect else ''}two_pass"
        words, n_words, status = enc.to_numpy()
        assert status.tolist() == bt.expected_status(), layout
        for s in bt.good:
            assert n_words[s] == len(want[s]) and words[s, : n_words[s]].tolist() == want[s].tolist(), f"stream {s} ({layout})"
        for route, name in routes.items():
            knob(CST_CATEGORICAL_ROUTE=route)
            for source, batch in (("encoder", enc), ("oracle", host)):
                dec, dstatus = decode(batch, d_probs, layout, perfect=perfect)
                torch.cuda.synchronize()
                assert B.last_kernel() == name.format(coder=coder)
                what = f"{layout}, route {route or 'by rows'}, the {source}'s words"
                dstatus = dstatus.cpu().numpy()
                assert (dstatus[good] == OK).all(), f"{what}: statuses {dstatus[good].tolist()}"
                got = dec.cpu().numpy()
                got = got.T if layout == "symbol_major" else got
                for s in bt.good:
                    assert got[s].tolist() == sym[s].tolist(), f"{what}: stream {s}"


# ---------------------------------------------------------------------------------------------- c. the ragged coders

def ragged_names(coder, perfect):
    if perfect:
        return f"{coder}_encode_categorical_perfect_ragged_two_pass", f"{coder}_decode_categorical_perfect_ragged_by_rows"
    return f"{coder}_encode_categorical_ragged_two_pass", f"{coder}_decode_categorical_ragged_kernel"


def ragged_calls(B, coder, perfect):
    word = "categorical_perfect" if perfect else "categorical"
    return (getattr(B, f"{coder}_encode_{word}_ragged"), getattr(B, f"{coder}_decode_{word}_ragged"),
            getattr(B, f"{coder}_decode_{word}_ragged_select"))


def batch_streams(enc):
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n[s]] for s in range(len(n))], n


def device_tables(enc):
    """the batch's jump table, per stream, as the oracle helpers give it: [(pos, state)] or [(pos, lower, range)]"""
    jump = enc.jump
    off = jump.chunk_offsets.cpu().numpy()
    cols = [jump.pos.cpu().numpy().view(np.uint32)] + [a.cpu().numpy().view(np.uint64) for a in
                                                        ([jump.state] if enc.coder == "ans" else [jump.lower, jump.range])]
    return [[tuple(int(c[i]) for c in cols) for i in range(off[s], off[s + 1])] for s in range(len(off) - 1)]


def assert_good_streams_decode(bt, dec, status, what):
    dec, status = dec.cpu().numpy(), status.cpu().numpy()
    for s in bt.good:
        assert status[s] == OK, f"{what}: stream {s} has status {status[s]}"
        assert dec[bt.offsets[s]: bt.offsets[s + 1]].tolist() == bt.syms[s].tolist(), f"{what}: stream {s}"


@pytest.mark.parametrize("every", [0, Z.JUMP_EVERY])
@pytest.mark.parametrize("cfg", Z.PRESETS, ids=Z.cfg_id)
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("quant", QUANTS, ids=quant_id)
def test_ragged_coders(B, quant, coder, cfg, every):
    """70 streams of 0 .. 300 symbols, hard rows on both sides of the jump points 16 and 32.  A stream that holds a refused row or codes an
    empty interval fails alone; every other container is its oracle coder's words, the jump table the oracle's positions; the encoder's
    batch decodes with the table and without it, and so do the oracle's containers with the oracle's table (the streams that code,
    packed into a batch of their own)."""
    quant, (k, dtype) = quant
    perfect = quant == "perfect"
    bt, want = Z.expected("ragged", quant, k, dtype, cfg, every)
    want = want[coder]
    words_of = lambda s: want[s][0] if every else want[s]
    encode, decode, _ = ragged_calls(B, coder, perfect)
    enc_name, dec_name = ragged_names(coder, perfect)
    sym, probs = bt.flat()
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(bt.offsets)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == enc_name + ("<jump>" if every else "")
    assert enc.status.cpu().tolist() == bt.expected_status()
    got, n_words = batch_streams(enc)
    for s in bt.good:
        assert n_words[s] == len(words_of(s)) and got[s].tolist() == words_of(s).tolist(), f"stream {s}: {n_words[s]} words"
    if every:
        tables = device_tables(enc)
        for s in bt.good:
            assert tables[s] == want[s][1], f"stream {s} ({bt.lengths[s]} symbols): the table differs from the oracle's"
    # the encoder's batch, through the chunks of its table and as whole streams
    for batch in ((enc, dataclasses.replace(enc, jump=None)) if every else (enc,)):
        dec, status = decode(batch, d_off, d_probs)
        torch.cuda.synchronize()
        assert B.last_kernel() == dec_name + ("<jump>" if batch.jump is not None else "")
        assert_good_streams_decode(bt, dec, status, "the encoder's words" + (", no table" if every and batch.jump is None else ""))
    # the oracle's containers and the oracle's table: the streams that code
    lengths = [bt.lengths[s] for s in bt.good]
    g_sym, g_probs = np.concatenate([bt.syms[s] for s in bt.good]), np.ascontiguousarray(np.concatenate([bt.probs[s] for s in bt.good]))
    g_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    host = host_ragged(B, cfg, coder, [words_of(s) for s in bt.good], lengths, [want[s][1] for s in bt.good] if every else None, every)
    d_gsym, d_gprobs, d_goff = dev(g_sym), dev(g_probs), dev(g_off)
    for batch in ((host, dataclasses.replace(host, jump=None)) if every else (host,)):
        dec, status = decode(batch, d_goff, d_gprobs)
        torch.cuda.synchronize()
        assert B.last_kernel() == dec_name + ("<jump>" if batch.jump is not None else "")
        assert status.cpu().tolist() == [OK] * len(lengths)
        assert torch.equal(dec, d_gsym)


# ---------------------------------------------------------------------------------------------- d. select

@pytest.mark.parametrize("every", [0, Z.JUMP_EVERY])
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("quant", [("fast", (65, "f32")), ("fast", (257, "f64")), ("perfect", (65, "f32")), ("perfect", (64, "f64"))], ids=quant_id)
def test_select(B, quant, coder, every):
    """queries that start and end on and next to every hard row of three long streams (1-symbol ranges among them), every stream that
    codes as a whole, and -- in the same call -- queries that reach a refused row: those fail alone, every other slice is the input's"""
    quant, (k, dtype) = quant
    perfect, cfg = quant == "perfect", (32, 64, 24)
    bt = Z.ragged_batch(quant, k, dtype, cfg[2])
    encode, _, select = ragged_calls(B, coder, perfect)
    sym, probs = bt.flat()
    d_sym, d_probs, d_off = dev(sym), dev(probs), dev(bt.offsets)
    enc = encode(d_sym, d_off, d_probs, cfg, order=None, jump_every=every)          # (its words and table: test_ragged_coders)
    assert enc.status.cpu().tolist() == bt.expected_status()
    long_ones = [s for s in bt.good if bt.lengths[s] > Z.HARD_SPAN][:2] + [s for s in bt.good if bt.lengths[s] == 33][:1]
    assert len(long_ones) == 3 and any(bt.lengths[s] == 300 for s in long_ones)
    queries = []
    for s in long_ones:
        n = bt.lengths[s]
        for j in range(min(n, Z.HARD_SPAN)):
            queries += [(s, j, 1), (s, max(j - 1, 0), 2), (s, j, min(2, n - j)), (s, 0, j + 1), (s, j, n - j)]
    queries += [(s, 0, bt.lengths[s]) for s in bt.good]
    # a refused row: the whole stream, the row alone, and a range that ends on it (without a table every query decodes from the start)
    bad = {}
    for s, col in list(bt.refused.items())[:6]:
        for q in ((s, 0, bt.lengths[s]), (s, col, 1), (s, 0, col + 1)):
            bad[len(queries)] = q
            queries.append(q)
            queries.append((long_ones[0], len(queries) % 30, 3))
    order = np.random.default_rng(k + every).permutation(len(queries))
    bad = {int(np.flatnonzero(order == i)[0]) for i in bad}
    queries = [queries[i] for i in order]
    streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int64, device="cuda")
    got, out_offsets, status = select(enc, d_off, d_probs, streams, [f for _, f, _ in queries], [c for _, _, c in queries])
    torch.cuda.synchronize()
    word = "categorical_perfect_ragged_by_rows" if perfect else "categorical_ragged_kernel"
    assert B.last_kernel() == f"{coder}_decode_{word}<select>"
    out_offsets, status, got = out_offsets.cpu().numpy(), status.cpu().numpy(), got.cpu().numpy()
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum([c for _, _, c in queries])]).tolist()
    for q, (s, first, count) in enumerate(queries):
        if q in bad:
            assert status[q] != OK, f"query {q} = {queries[q]} reaches a refused row and reports no failure"
        else:
            assert status[q] == OK, f"query {q} = {queries[q]}: status {status[q]}"
            assert got[out_offsets[q]: out_offsets[q + 1]].tolist() == bt.syms[s][first: first + count].tolist(), f"query {q} = {queries[q]}"
    # whole streams in the call's own form (first = count = None), a refused one among them
    whole = bt.good[::-1] + [next(iter(bt.refused))] + bt.good[:3]
    got, out_offsets, status = select(enc, d_off, d_probs, torch.tensor(whole, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    out_offsets, status, got = out_offsets.cpu().numpy(), status.cpu().numpy(), got.cpu().numpy()
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum([bt.lengths[s] for s in whole])]).tolist()
    for q, s in enumerate(whole):
        assert (status[q] != OK) == (s in bt.refused), f"stream {s}: status {status[q]}"
        if s not in bt.refused:
            assert got[out_offsets[q]: out_offsets[q + 1]].tolist() == bt.syms[s].tolist(), f"stream {s} as a whole"


# ---------------------------------------------------------------------------------------------- e. the drop-in coders

def one_stream(quant, k, dtype):
    """the first six streams of the rectangular batch that code, as ONE stream: valid and degenerate rows, every kind several times"""
    bt = Z.rect_batch(quant, k, dtype, 24)
    first = bt.good[:6]
    return (np.concatenate([bt.syms[s] for s in first]), np.ascontiguousarray(np.concatenate([bt.probs[s] for s in first])),
            [m for s in first for m in bt.models(s)], bt)


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("which", ["fast_f32", "lazy_f64", "perfect_f32"])
def test_drop_in(B, which, coder, knob):
    """stream.stack.AnsCoder / stream.queue.Range{Encoder,Decoder} with Categorical(perfect=False), Categorical(lazy=True) and
    Categorical(perfect=True) over one stream of valid and degenerate zoo rows: the oracle's words, and a round trip in two decode
    calls through every route"""
    import constriction_amd
    from constriction_amd import stream  # noqa: F401
    mod, stack, queue = constriction_amd.stream.model, constriction_amd.stream.stack, constriction_amd.stream.queue
    quant, k, dtype, model = {"fast_f32": ("fast", 65, "f32", mod.Categorical(perfect=False)),
                              "lazy_f64": ("fast", 64, "f64", mod.Categorical(lazy=True)),
                              "perfect_f32": ("perfect", 300, "f32", mod.Categorical(perfect=True))}[which]
    sym, probs, models, bt = one_stream(quant, k, dtype)
    classes = {bt.zoo.classes[kind] for s in bt.good[:6] for kind in bt.kinds[s] if kind is not None}
    assert classes == ({"valid"} if quant == "perfect" else {"valid", "degenerate"})
    want = Z.oracle_words(coder, (32, 64, 24), sym, models)
    routes = {"": "decode_categorical_perfect_by_rows"} if quant == "perfect" else FAST_ROUTES
    for route, name in routes.items():
        knob(CST_CATEGORICAL_ROUTE=route)
        if coder == "ans":
            enc = stack.AnsCoder()
            enc.encode_reverse(sym, model, probs)
            words = enc.get_compressed()
            dec = stack.AnsCoder(words)
        else:
            enc = queue.RangeEncoder()
            enc.encode(sym, model, probs)
            words = enc.get_compressed()
            dec = queue.RangeDecoder(words)
        assert B.last_kernel() == f"{coder}_encode_categorical_{'perfect_' if quant == 'perfect' else ''}two_pass"
        assert words.tolist() == want.tolist()
        first = dec.decode(model, probs[:51])
        assert B.last_kernel() == name.format(coder=coder)
        second = dec.decode(model, probs[51:])
        assert np.concatenate([first, second]).tolist() == sym.tolist(), route
