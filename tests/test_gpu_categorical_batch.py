"""GPU tests of the BATCHED per-symbol Categorical calls (constriction_amd.batched.*_categorical, categorical_cdf_rows) and of the
drop-in coders that use them: `encode_reverse(symbols, Categorical(perfect=False), probabilities)` /
`decode(Categorical(lazy=True), probabilities)` (src/pybindings/stream/model/internals.rs:399-514) for many coders at once, with the
probability rows quantised inside the coder kernels.

Every expected word and symbol comes from the CPU oracle: one tabulated model per symbol over oracle.categorical_fast_cdf (f32 rows
in f32, f64 rows in f64), fed to one oracle coder per stream.  No GPU result is the reference for another.  The rows are
Dirichlet(0.3) draws with exact zeros inside and a last entry of at least 1e-3 of the sum: every table here is strictly increasing
(an f32 row that ENDS in a zero can have an empty last interval: that case is tested on its own below).  The degenerate tables --
tiny sums with an infinite scale, sums at the edges of the normal range -- and every other hard row go through these kernels in
tests/test_gpu_categorical_extremes.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 64                  # kCatChunk of csrc/cst_persymbol_categorical.hip: columns of a row staged at a time
ROUTES = {"fused": "{coder}_decode_categorical_lane_kernel", "rows": "decode_categorical_by_rows"}
# (n_streams, n_per_stream, K): every n_streams of {1, 3, 63, 64, 65, 130}, every n_per_stream of {1, 31, 64, 65, 100} and every K of
# {2, 5, 64, 65, 257, 1031} + {C - 1, C, C + 1, 2 C + 1} appears, and every case runs through both routes of the decoder
CASES = [(1, 100, 5), (3, 65, 64), (63, 31, 257), (64, 64, 65), (65, 1, 1031), (130, 100, 2), (64, 31, CHUNK - 1), (3, 64, 2 * CHUNK + 1),
         (65, 65, 5), (1, 31, 1031)]
DTYPES = {"f32": np.float32, "f64": np.float64}


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


def workload(n_streams, n_per, k, dtype, seed):
    """probabilities [n_streams, n_per, k] and symbols: uniform draws (so they sit on exact-zero entries too), with symbol 0 and symbol
    k - 1 in front of every stream (alternating over the streams where a stream has one symbol)"""
    rng = np.random.default_rng(seed)
    probs = rng.dirichlet(np.full(k, 0.3), size=(n_streams, n_per))
    if k > 2:
        probs[..., 1:-1][rng.random((n_streams, n_per, k - 2)) < 0.3] = 0.0
    probs[..., -1] = np.maximum(probs[..., -1], 2e-3)           # (the sum stays below 1.002: at least 1e-3 of it)
    probs *= np.exp(rng.uniform(-3.0, 3.0, (n_streams, n_per, 1)))   # not normalised
    probs = np.ascontiguousarray(probs.astype(dtype))
    sym = rng.integers(0, k, (n_streams, n_per)).astype(np.int32)
    if n_per >= 2:
        sym[:, 0], sym[:, 1] = 0, k - 1
    else:
        sym[:, 0] = np.where(np.arange(n_streams) % 2 == 0, k - 1, 0)
    return sym, probs


def models_of(O, probs_of_stream, P):
    return [O.TableModel(O.categorical_fast_cdf(row, P), 0, P) for row in probs_of_stream]


def oracle_words(O, coder, cfg, sym, models):
    W, S, P = cfg
    if coder == "ans":
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return c.get_compressed()


_expected = {}


def expected(O, case, dtype, coder, cfg):
    key = (case, dtype, coder, cfg)
    if key not in _expected:
        n_streams, n_per, k = case
        mkey = (case, dtype, cfg[2])
        if mkey not in _expected:
            sym, probs = workload(n_streams, n_per, k, DTYPES[dtype], sum(case) + cfg[2])
            _expected[mkey] = (sym, probs, [models_of(O, probs[s], cfg[2]) for s in range(n_streams)])
        sym, probs, models = _expected[mkey]
        _expected[key] = (sym, probs, [oracle_words(O, coder, cfg, sym[s], models[s]) for s in range(n_streams)])
    return _expected[key]


def in_layout(layout, sym, probs):
    if layout == "symbol_major":
        return dev(sym.T), dev(probs.transpose(1, 0, 2))
    return dev(sym), dev(probs)


@pytest.mark.parametrize("cfg", [(32, 64, 24), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dxK%d" % c)
def test_categorical_batch_parity(B, O, case, dtype, coder, cfg, knob):
    n_streams, n_per, k = case
    sym, probs, want = expected(O, case, dtype, coder, cfg)
    for layout in ("stream_major", "symbol_major"):
        d_sym, d_probs = in_layout(layout, sym, probs)
        enc = getattr(B, f"{coder}_encode_categorical")(d_sym, d_probs, cfg, layout)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_encode_categorical_two_pass"
        words, n_words, status = enc.to_numpy()
        assert (status == 0).all()
        assert n_words.tolist() == [len(w) for w in want]
        for s in range(n_streams):
            assert words[s, : n_words[s]].tolist() == want[s].tolist(), f"stream {s} ({layout})"
        for route, name in ROUTES.items():
            knob(CST_CATEGORICAL_ROUTE=route)
            dec, dstatus = getattr(B, f"{coder}_decode_categorical")(enc, d_probs, layout)
            torch.cuda.synchronize()
            assert B.last_kernel() == name.format(coder=coder)
            assert (dstatus.cpu().numpy() == 0).all(), (layout, route)
            got = dec.cpu().numpy()
            assert np.array_equal(got.T if layout == "symbol_major" else got, sym), (layout, route)
        knob(CST_CATEGORICAL_ROUTE="")


def test_default_route_follows_the_number_of_streams(B, O):
    for case, route in (((63, 31, 257), "rows"), ((64, 64, 65), "fused"), ((1, 100, 5), "rows"), ((130, 100, 2), "fused")):
        sym, probs, _ = expected(O, case, "f32", "ans", (32, 64, 24))
        enc = B.ans_encode_categorical(dev(sym), dev(probs))
        dec, st = B.ans_decode_categorical(enc, dev(probs))
        torch.cuda.synchronize()
        assert B.last_kernel() == ROUTES[route].format(coder="ans")
        assert (st.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [2, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 257, 1031])
def test_cdf_rows_equal_the_oracle(B, O, k, dtype, P):
    _, probs = workload(7, 10, k, DTYPES[dtype], k + P)          # 70 rows: a whole wave and a partial one
    rows = B.categorical_cdf_rows(dev(probs), P)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (7, 10, k + 1)
    rows = rows.cpu().numpy().view(np.uint32)
    for s in range(7):
        for t in range(10):
            assert rows[s, t].tolist() == O.categorical_fast_cdf(probs[s, t], P).tolist(), (s, t)
    bad = probs.copy()
    bad[3, 4, k - 1] = np.nan
    with pytest.raises(ValueError, match="not normalizable"):
        B.categorical_cdf_rows(dev(bad), P)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_one_call_equals_two_continued_calls(B, O, coder, dtype):
    """CST_FLAG_RAW_STATE: the coders of a batch continue from the state a first call left -- the two halves of every stream by two
    calls give the words and the state of one call over the whole stream (and, for ANS, the oracle's words)"""
    from constriction_amd import _native as N
    case, cfg = (65, 65, 5), (32, 64, 24)
    n_streams, n_per, k = case
    sym, probs, want = expected(O, case, dtype, coder, cfg)
    half, stride = 33, B.max_words(n_per, cfg) + 8
    fn = getattr(N.lib(), f"cst_{coder}_encode_categorical_batch")

    def fresh_state():
        if coder == "ans":
            return torch.zeros(n_streams, dtype=torch.int64, device="cuda")
        st = np.zeros((n_streams, 5), dtype=np.uint64)            # cst_range_state: lower, range, point, (inverted_n, inverted_first), position
        st[:, 1] = 0xFFFFFFFFFFFFFFFF
        return dev(st.view(np.int64))

    def run(d_sym, d_probs, n, state):
        words = torch.zeros((n_streams, stride), dtype=torch.int32, device="cuda")
        n_words = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
        status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
        N.check(fn(N.CoderConfig(*cfg), _ptr(d_sym), _ptr(d_probs), probs.itemsize, k, n_streams, n, N.LAYOUT_STREAM_MAJOR, _ptr(words), stride,
                   _ptr(n_words), _ptr(state), _ptr(status), N.FLAG_RAW_STATE, None), "raw")
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        n_words = n_words.cpu().numpy()
        return [words[s, : n_words[s]].cpu().numpy().view(np.uint32).tolist() for s in range(n_streams)]

    st_one = fresh_state()
    one = run(dev(sym), dev(probs), n_per, st_one)
    # ANS codes backwards (the second half of a stream first), the range coder forwards
    parts = [(sym[:, half:], probs[:, half:]), (sym[:, :half], probs[:, :half])]
    if coder == "range":
        parts.reverse()
    st_two = fresh_state()
    a = run(dev(parts[0][0]), dev(parts[0][1]), parts[0][0].shape[1], st_two)
    b = run(dev(parts[1][0]), dev(parts[1][1]), parts[1][0].shape[1], st_two)
    assert np.array_equal(st_one.cpu().numpy(), st_two.cpu().numpy())
    state = st_one.cpu().numpy().view(np.uint64)
    for s in range(n_streams):
        assert a[s] + b[s] == one[s], s
        if coder == "ans":
            tail = [int(state[s]) & 0xFFFFFFFF, int(state[s]) >> 32]
            while tail and tail[-1] == 0:
                tail.pop()
            assert one[s] + tail == want[s].tolist(), s


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_a_slab_that_is_too_small_reports_capacity(B, O, coder):
    sym, probs, want = expected(O, (130, 100, 2), "f32", coder, (32, 64, 24))
    assert min(len(w) for w in want) > 2
    sentinel = 0x5A5A5A5A
    enc = B.EncodedBatch(torch.full((130, 2), sentinel, dtype=torch.int32, device="cuda"), torch.zeros(130, dtype=torch.int32, device="cuda"),
                         torch.zeros(130, dtype=torch.int32, device="cuda"), (32, 64, 24))
    getattr(B, f"{coder}_encode_categorical")(dev(sym), dev(probs), out=enc)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == 2).all() and (enc.n_words.cpu().numpy() == 0).all()      # CST_STREAM_CAPACITY


def _overflowing(dtype):
    return np.finfo(dtype).max


@pytest.mark.parametrize("k", [7, 257])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_failures_stay_in_their_stream(B, O, coder, dtype, k, knob):
    """a NaN, negative, all-zero or overflowing row and a symbol outside [0, K) give CST_STREAM_IMPOSSIBLE_SYMBOL for their stream
    only: every other stream still has the oracle's words, and decodes"""
    cfg = (32, 64, 24)
    n_streams, n_per = 70, 20
    sym, probs = workload(n_streams, n_per, k, DTYPES[dtype], 5 * k)
    want = {s: oracle_words(O, coder, cfg, sym[s], models_of(O, probs[s], 24)) for s in range(0, n_streams, 3)}
    bad_p, bad_s = probs.copy(), sym.copy()
    bad_p[4, 3, k // 2] = np.nan
    bad_p[11, 19, 0] = -0.125
    bad_p[23, 0, :] = 0.0
    bad_p[38, 7, :2] = _overflowing(DTYPES[dtype])
    bad_s[50, 5] = -1
    bad_s[65, 19] = k
    rows_bad, syms_bad = [4, 11, 23, 38], [50, 65]
    enc = getattr(B, f"{coder}_encode_categorical")(dev(bad_s), dev(bad_p), cfg)
    torch.cuda.synchronize()
    words, n_words, status = enc.to_numpy()
    assert status[rows_bad + syms_bad].tolist() == [1] * 6 and (np.delete(status, rows_bad + syms_bad) == 0).all()
    for s, w in want.items():
        if s not in rows_bad + syms_bad:
            assert words[s, : n_words[s]].tolist() == w.tolist(), s
    good = getattr(B, f"{coder}_encode_categorical")(dev(sym), dev(probs), cfg)
    for route in ROUTES:
        knob(CST_CATEGORICAL_ROUTE=route)
        dec, st = getattr(B, f"{coder}_decode_categorical")(good, dev(bad_p))
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        assert st[rows_bad].tolist() == [1] * 4 and (np.delete(st, rows_bad) == 0).all(), route
        assert np.array_equal(np.delete(dec.cpu().numpy(), rows_bad, axis=0), np.delete(sym, rows_bad, axis=0)), route
        # what was decoded in front of the bad row stands
        assert np.array_equal(dec.cpu().numpy()[11, :19], sym[11, :19]), route


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_empty_last_interval_of_a_trailing_zero_f32_row(B, O, coder):
    """an f32 row whose last entry is exactly 0 can have cdf[K - 1] == 2^P in the reference: encoding symbol K - 1 with it is an
    impossible symbol, every other symbol of the row codes as the oracle codes it"""
    cfg, k, n_streams, n_per = (32, 64, 24), 5, 66, 6
    rng = np.random.default_rng(3)
    sym, probs = workload(n_streams, n_per, k, np.float32, 17)
    while True:
        row = rng.dirichlet(np.full(k, 0.3)).astype(np.float32)
        row[-1] = 0.0
        if O.categorical_fast_cdf(row, 24)[k - 1] == 1 << 24:
            break
    probs[9, 2], probs[40, 4] = row, row
    sym[9, 2], sym[40, 4] = k - 1, k - 2                    # stream 9: the empty interval; stream 40: its neighbour, a valid symbol
    enc = getattr(B, f"{coder}_encode_categorical")(dev(sym), dev(probs), cfg)
    torch.cuda.synchronize()
    words, n_words, status = enc.to_numpy()
    assert status[9] == 1 and (np.delete(status, 9) == 0).all()
    for s in (8, 10, 40, 65):
        assert words[s, : n_words[s]].tolist() == oracle_words(O, coder, cfg, sym[s], models_of(O, probs[s], 24)).tolist(), s
    dec, st = getattr(B, f"{coder}_decode_categorical")(enc, dev(probs))
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert (np.delete(st, 9) == 0).all()
    assert np.array_equal(np.delete(dec.cpu().numpy(), 9, axis=0), np.delete(sym, 9, axis=0))


def test_arguments_are_checked_like_the_family_calls(B):
    sym, probs = workload(4, 6, 5, np.float32, 1)
    with pytest.raises(ValueError):
        B.ans_encode_categorical(dev(sym), dev(probs[:, :5]))                  # not the symbols' shape
    with pytest.raises(TypeError):
        B.ans_encode_categorical(dev(sym), dev(probs.astype(np.float16)))
    with pytest.raises(ValueError):
        B.ans_encode_categorical(dev(sym), torch.from_numpy(probs))            # not in device memory
    with pytest.raises(ValueError):
        B.range_encode_categorical(dev(sym), dev(probs[..., :1]))              # K < 2
    with pytest.raises(TypeError):
        B.range_encode_categorical(dev(sym.astype(np.int64)), dev(probs))
    enc = B.ans_encode_categorical(dev(sym), dev(probs))
    with pytest.raises(ValueError):
        B.ans_decode_categorical(enc, dev(probs[:3]))                          # not the number of streams
    with pytest.raises(ValueError):
        B.ans_decode_categorical(enc, dev(probs[0]))                           # not 3-d


@pytest.mark.parametrize("route", ["fused", "rows"])
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("which", ["fast_f32", "lazy_f64", "bernoulli"])
def test_drop_in(B, O, which, coder, route, knob):
    """stream.stack.AnsCoder / stream.queue.Range{Encoder,Decoder} with Categorical(perfect=False), Categorical(lazy=True) and
    Bernoulli(perfect=False) and per-symbol parameters take the new calls: the oracle's words, and a round trip in two decode calls"""
    import constriction_amd
    from constriction_amd import stream  # noqa: F401
    mod, stack, queue = constriction_amd.stream.model, constriction_amd.stream.stack, constriction_amd.stream.queue
    rng = np.random.default_rng(41)
    n = 700
    if which == "bernoulli":
        ps = rng.uniform(0.0, 1.0, n)
        ps[:2] = (0.0, 1.0)
        probs = np.stack([1.0 - ps, ps], axis=1)
        sym = (rng.random(n) < ps).astype(np.int32)
        model, params = mod.Bernoulli(perfect=False), ps
    else:
        sym, probs = workload(1, n, 300 if which == "fast_f32" else 12, np.float32 if which == "fast_f32" else np.float64, 9)
        sym, probs = sym[0], probs[0]
        model, params = (mod.Categorical(perfect=False) if which == "fast_f32" else mod.Categorical(lazy=True)), probs
    knob(CST_CATEGORICAL_ROUTE=route)
    if coder == "ans":
        enc = stack.AnsCoder()
        enc.encode_reverse(sym, model, params)
        words = enc.get_compressed()
        dec = stack.AnsCoder(words)
    else:
        enc = queue.RangeEncoder()
        enc.encode(sym, model, params)
        words = enc.get_compressed()
        dec = queue.RangeDecoder(words)
    assert B.last_kernel() == f"{coder}_encode_categorical_two_pass"
    assert words.tolist() == oracle_words(O, coder, (32, 64, 24), sym, models_of(O, probs, 24)).tolist()
    first = dec.decode(model, params[:301])
    assert B.last_kernel() == ROUTES[route].format(coder=coder)
    second = dec.decode(model, params[301:])
    assert np.array_equal(np.concatenate([first, second]), sym)


def test_drop_in_refuses_an_invalid_matrix(B):
    import constriction_amd
    from constriction_amd import stream  # noqa: F401
    mod, stack, queue = constriction_amd.stream.model, constriction_amd.stream.stack, constriction_amd.stream.queue
    sym, probs = workload(1, 8, 5, np.float64, 2)
    sym, probs = sym[0], probs[0]
    for spoil in (np.nan, -0.5, np.inf):
        bad = probs.copy()
        bad[3, 2] = spoil
        for model in (mod.Categorical(perfect=False), mod.Categorical(lazy=True)):
            with pytest.raises(ValueError, match="not normalizable"):
                stack.AnsCoder().encode_reverse(sym, model, bad)
            with pytest.raises(ValueError, match="not normalizable"):
                queue.RangeEncoder().encode(sym, model, bad)
    zero = probs.copy()
    zero[5, :] = 0.0
    with pytest.raises(ValueError, match="not normalizable"):
        stack.AnsCoder().encode_reverse(sym, mod.Categorical(perfect=False), zero)
    with pytest.raises(ValueError, match="`p` must be"):
        stack.AnsCoder().encode_reverse(sym, mod.Bernoulli(perfect=False), np.linspace(-0.1, 0.9, 8))
