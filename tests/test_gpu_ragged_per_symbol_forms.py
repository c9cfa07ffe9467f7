"""GPU parity tests of the ragged per-symbol calls beyond ANS x Gaussian (batched.{ans,range}_{encode,decode}_{gaussian,laplace,
cauchy}_ragged, cst_range_*_gaussian_ragged and cst_{ans,range}_*_family_ragged): every stream's words against ONE CPU oracle coder
for that stream alone -- the reference's `AnsCoder.encode_reverse(symbols, Model(lo, hi), a, b)` or `RangeEncoder.encode(...)` +
`get_compressed()` -- and the decode round trip.  Every stream of every batch is compared; no GPU result is the reference for
another, except where a test says that two GPU calls must agree.

The models of a batch are built once per precision and shared between its ANS and its range oracle.  The shapes are those of
tests/test_gpu_gaussian_ragged.py: the smallest that cross every boundary of the two kernels (16-symbol encoder tiles, 8-symbol
parameter tiles, 16-symbol output tiles, 32 / 64 streams per wave, 128 / 256 per workgroup)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CONFIGS = [(32, 64, 24), (32, 64, 12), (16, 32, 12)]
EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 700, 0]
# (coder, family): the five forms that the ragged ANS x Gaussian pair left open
FORMS = [("ans", "laplace"), ("ans", "cauchy"), ("range", "gaussian"), ("range", "laplace"), ("range", "cauchy")]
form_id = lambda f: "%s-%s" % f
cfg_id = lambda c: "W%dS%dP%d" % c


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


def support(P):
    return (-100, 100) if P == 24 else (-60, 60)


def draw(rng, family, loc, scale):
    """tests/test_gpu_family_batch.py::draw, and the Gaussian of tests/test_gpu_gaussian_ragged.py::workload"""
    if family == "gaussian":
        return loc + scale * rng.standard_normal(loc.shape)
    return rng.laplace(loc, scale) if family == "laplace" else loc + scale * rng.standard_cauchy(loc.shape)


def workload(family, lengths, lo, hi, seed, thin_every=5):
    """per stream: location uniform in 0.6 [lo, hi], scale log-uniform in 0.3 .. 40, symbols drawn from the model and clipped, lo and
    hi themselves in front; every `thin_every`-th non-empty stream is needle-thin (scale 1e-3 at 0.6 lo, uniform symbols): about P
    bits per symbol, the most a stream can need"""
    rng = np.random.default_rng(seed)
    syms, locs, scales, non_empty = [], [], [], 0
    for n in lengths:
        n = int(n)
        a = rng.uniform(lo * 0.6, hi * 0.6, n)
        b = np.exp(rng.uniform(np.log(0.3), np.log(40.0), n))
        sym = np.clip(np.rint(draw(rng, family, a, b)), lo, hi).astype(np.int32)
        sym[:2] = np.array([lo, hi])[: min(2, n)]
        if n > 0:
            non_empty += 1
            if thin_every and non_empty % thin_every == 0:
                a = np.full(n, 0.6 * lo)
                b = np.full(n, 1e-3)
                sym = rng.integers(lo, hi + 1, n).astype(np.int32)
        syms.append(sym); locs.append(a); scales.append(b)
    return syms, locs, scales


def flatten(B, syms, locs, scales, dtype=np.float64):
    flat, offsets = B.ragged(syms)
    cat = lambda xs: np.concatenate(xs).astype(dtype) if len(xs) else np.zeros(0, dtype)
    return flat, offsets, dev(cat(locs)), dev(cat(scales))


def models_of(O, family, lo, hi, a, b, P):
    """one oracle model per symbol of a stream"""
    if family == "gaussian":
        return [O.GaussianModel(lo, hi, float(x), float(y), P) for x, y in zip(a, b)]
    fam = O.FAMILY_LAPLACE if family == "laplace" else O.FAMILY_CAUCHY
    return [O.TableModel(O.leaky_family_cdf(fam, lo, hi, float(x), float(y), P), lo, P) for x, y in zip(a, b)]


def batch_models(O, family, P, locs, scales):
    lo, hi = support(P)
    return [models_of(O, family, lo, hi, a, b, P) for a, b in zip(locs, scales)]


def oracle_streams(O, coder, cfg, syms, models):
    """get_compressed() of one oracle coder per stream (a zero-length stream: no words from either coder)"""
    W, S, P = cfg
    want = []
    for sym, m in zip(syms, models):
        if coder == "ans":
            if len(sym) == 0:
                want.append(np.zeros(0, np.uint32))
                continue
            c = O.AnsCoder(W=W, S=S)
            c.encode_reverse(sym, m, P)
        else:
            c = O.RangeEncoder(W=W, S=S)        # (no symbols: get_compressed() of a fresh RangeEncoder, which is empty)
            c.encode(sym, m, P)
        want.append(np.asarray(c.get_compressed()))
    return want


def calls(B, form):
    coder, family = form
    return (getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged"),
            f"{coder}_encode_{family}_ragged_kernel", f"{coder}_decode_{family}_ragged_kernel")


def batch_streams(enc):
    """every stream's words of a RaggedBatch, with one copy to the host"""
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n[s]] for s in range(len(n))], n


def assert_streams_equal(got, n_words, want, what=""):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert n_words[s] == len(w) and g.tolist() == w.tolist(), f"{what}stream {s}: {n_words[s]} words, the oracle has {len(w)}"


_BATCHES = {}       # (family, P) -> (lengths, syms, locs, scales, models): the 300-stream batch, built once, never modified
_WANT = {}          # (form, cfg) -> oracle words of that batch


def big_batch(O, form, cfg):
    coder, family = form
    P = cfg[2]
    if (family, P) not in _BATCHES:
        lo, hi = support(P)
        rng = np.random.default_rng(1000 + P)
        lengths = EDGE_LENGTHS + rng.integers(0, 120, 286).tolist()
        syms, locs, scales = workload(family, lengths, lo, hi, 77 + P)
        _BATCHES[(family, P)] = (lengths, syms, locs, scales, batch_models(O, family, P, locs, scales))
    lengths, syms, locs, scales, models = _BATCHES[(family, P)]
    if (form, cfg) not in _WANT:
        _WANT[(form, cfg)] = oracle_streams(O, coder, cfg, syms, models)
    return lengths, syms, locs, scales, _WANT[(form, cfg)]


def check_against_oracle(B, form, cfg, syms, locs, scales, want, **kw):
    lo, hi = support(cfg[2])
    encode, decode, enc_name, dec_name = calls(B, form)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg, **kw)
    torch.cuda.synchronize()
    assert B.last_kernel() == enc_name
    assert enc.jump is None and enc.coder == form[0]
    assert (enc.status.cpu().numpy() == 0).all(), enc.status.cpu().tolist()
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = decode(enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert B.last_kernel() == dec_name
    assert (status.cpu().numpy() == 0).all(), status.cpu().tolist()
    assert torch.equal(dec, flat)
    return enc


def slab_bound(form, cfg, lengths):
    """min(n, ceil(n P / W)) words, plus the S / W words of the ANS state or the 2 words that seal a range coder"""
    W, S, P = cfg
    n = np.asarray(lengths)
    return np.minimum(n, (n * P + W - 1) // W) + (S // W if form[0] == "ans" else 2)


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_every_stream_equals_its_oracle_coder(B, O, form, cfg):
    """300 streams of 0 .. 700 symbols, every fifth non-empty one needle-thin (about P bits per symbol): statuses, counts and
    words of every stream are the oracle's, decoding returns the flat input, and the slabs are the stated bound"""
    lengths, syms, locs, scales, want = big_batch(O, form, cfg)
    assert len(lengths) == 300 and len(want) == 300
    enc = check_against_oracle(B, form, cfg, syms, locs, scales, want)
    bound = slab_bound(form, cfg, lengths)
    assert np.diff(enc.word_offsets.cpu().numpy()).tolist() == ((bound + 3) // 4 * 4).tolist()
    assert (enc.n_words.cpu().numpy() <= bound).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("lengths", [[37], list(range(33))], ids=["one_stream", "33_streams"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_one_stream_and_the_encoder_wave_boundary(B, O, form, lengths, cfg):
    """a single stream; 33 streams of 0 .. 32 symbols: a zero-length stream first and one stream in a second encoder wave"""
    lo, hi = support(cfg[2])
    syms, locs, scales = workload(form[1], lengths, lo, hi, 5 + len(lengths) + cfg[2])
    models = batch_models(O, form[1], cfg[2], locs, scales)
    check_against_oracle(B, form, cfg, syms, locs, scales, oracle_streams(O, form[0], cfg, syms, models))


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_same_words_as_the_rectangular_call(B, form):
    """96 streams of 40 symbols each: the ragged call and the form's rectangular call (no jump points) give every stream the same
    words"""
    coder, family = form
    cfg, lo, hi = (32, 64, 24), -100, 100
    syms, locs, scales = workload(family, [40] * 96, lo, hi, 4040)
    kw = {"jump_points": 0} if family == "gaussian" else {}
    rect = getattr(B, f"{coder}_encode_{family}")(dev(np.stack(syms)), lo, hi, dev(np.stack(locs)), dev(np.stack(scales)), cfg, **kw)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    enc = calls(B, form)[0](flat, offsets, lo, hi, a, b, cfg)
    torch.cuda.synchronize()
    words, n_words, status = rect.to_numpy()
    assert (status == 0).all() and (enc.status.cpu().numpy() == 0).all()
    got, n = batch_streams(enc)
    assert_streams_equal(got, n, [words[s, : n_words[s]].view(np.uint32) for s in range(96)])


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_a_bad_stream_does_not_touch_its_neighbours(B, O, form):
    """scale = 0 in stream 1, a NaN location in stream 3, a symbol above the support in stream 4: exactly those streams are
    flagged (no words), streams 0 and 2 are the oracle's, and the good streams alone encode to the same words and decode"""
    coder, family = form
    cfg, lo, hi = (32, 64, 24), -100, 100
    encode, decode, _, _ = calls(B, form)
    syms, locs, scales = workload(family, (5, 64, 0, 300, 17), lo, hi, 31, thin_every=0)
    keep = (0, 2)
    good = oracle_streams(O, coder, cfg, [syms[s] for s in keep],
                          batch_models(O, family, 24, [locs[s] for s in keep], [scales[s] for s in keep]))
    scales[1][40] = 0.0
    locs[3][123] = np.nan
    syms[4][9] = hi + 1
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [0, 1, 0, 1, 1]
    got, n_words = batch_streams(enc)
    assert [int(n_words[s]) for s in (1, 3, 4)] == [0, 0, 0]
    for s, w in zip(keep, good):
        assert n_words[s] == len(w) and got[s].tolist() == w.tolist()
    # the same batch without the bad streams
    flat2, offsets2, a2, b2 = flatten(B, [syms[s] for s in keep], [locs[s] for s in keep], [scales[s] for s in keep])
    enc2 = encode(flat2, offsets2, lo, hi, a2, b2, cfg)
    dec, status = decode(enc2, offsets2, lo, hi, a2, b2)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and torch.equal(dec, flat2)
    got2, n2 = batch_streams(enc2)
    assert_streams_equal(got2, n2, good)


@pytest.mark.parametrize("form", [("range", "gaussian"), ("ans", "laplace")], ids=form_id)
def test_corrupt_word_metadata(B, form):
    """decoder: a count of 2^30 and an offset of 2^40 (both leave the buffer whose numel is the call's words_capacity) give those
    streams status 3 and leave the others as they were; encoder: word offsets that run backwards give that stream
    CST_STREAM_CAPACITY and nothing is written outside the other streams' slabs.  Both are refusals by the bounds check in front
    of every access: a status, never a fault"""
    from constriction_amd import _native as N
    coder, family = form
    cfg, lo, hi = (32, 64, 24), -100, 100
    encode, decode, _, _ = calls(B, form)
    syms, locs, scales = workload(family, (5, 64, 300, 17), lo, hi, 32, thin_every=0)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg)
    ref, status = decode(enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0] and torch.equal(ref, flat)
    enc.n_words[1] = 1 << 30
    enc.word_offsets[2] = 1 << 40
    dec, status = decode(enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 3, 3, 0]
    off = offsets.cpu().numpy()
    assert torch.equal(dec[: off[1]], ref[: off[1]]) and torch.equal(dec[off[3]: off[4]], ref[off[3]: off[4]])

    n = len(syms)
    woff = torch.tensor([0, 64, 32, 512, 1024], dtype=torch.int64, device="cuda")      # stream 1: [64, 32)
    words = torch.full((2048,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    name = "cst_range_encode_gaussian_ragged" if family == "gaussian" else f"cst_{coder}_encode_family_ragged"
    fam = () if family == "gaussian" else (B.FAMILIES[family],)
    N.check(getattr(N.lib(), name)(N.CoderConfig(*cfg), *fam, lo, hi, p(flat), p(a), p(b), p(offsets), n, None, p(words), p(woff), 0,
                                   p(n_words), p(status), None), name)
    torch.cuda.synchronize()
    st, nw, w = status.cpu().tolist(), n_words.cpu().numpy(), words.cpu().numpy()
    assert st == [0, 2, 0, 0] and nw[1] == 0
    # slabs: stream 0 = [0, 64), stream 2 = [32, 512), stream 3 = [512, 1024); nothing else is written
    assert (w[1024:] == 0x5A5A5A5A).all()
    assert (w[nw[0]: 32] == 0x5A5A5A5A).all() and (w[32 + nw[2]: 512] == 0x5A5A5A5A).all() and (w[512 + nw[3]: 1024] == 0x5A5A5A5A).all()
    # (streams 0 and 2 overlap in [32, 64) by this construction: stream 0 has fewer than 32 words)
    assert nw[0] <= 32


@pytest.mark.parametrize("form", [("range", "gaussian"), ("ans", "cauchy")], ids=form_id)
def test_results_do_not_depend_on_the_schedule(B, O, form):
    """the parity batch at (32,64,24) with no schedule, sorted, reversed and shuffled: words, counts and statuses are the same
    per stream, and so are the decoded symbols"""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    encode, decode, enc_name, dec_name = calls(B, form)
    lengths, syms, locs, scales, want = big_batch(O, form, cfg)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    n = len(lengths)
    rng = np.random.default_rng(9)
    schedules = [None, "sorted", dev(np.arange(n - 1, -1, -1).astype(np.int32)), dev(rng.permutation(n).astype(np.int32))]
    for order in schedules:
        enc = encode(flat, offsets, lo, hi, a, b, cfg, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == enc_name
        assert (enc.status.cpu().numpy() == 0).all()
        assert (enc.order is None) == (order is None)
        got, n_words = batch_streams(enc)
        assert_streams_equal(got, n_words, want, what=f"order {order if order is None or isinstance(order, str) else 'tensor'}: ")
        dec, status = decode(enc, offsets, lo, hi, a, b, order=order if order is None else "auto")
        torch.cuda.synchronize()
        assert B.last_kernel() == dec_name
        assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
    # ... and a decoder schedule keyed on the word counts, on a batch encoded without one
    enc = encode(flat, offsets, lo, hi, a, b, cfg, order=None)
    dec, status = decode(enc, offsets, lo, hi, a, b, order="sorted")
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_float32_parameters_are_widened(B, O, form):
    """float32 parameters: the models are those of the widened values (as the reference's Python API casts them)"""
    coder, family = form
    cfg, lo, hi = (32, 64, 24), -100, 100
    encode, decode, _, _ = calls(B, form)
    syms, locs, scales = workload(family, [0, 3, 50, 16, 129, 1], lo, hi, 66, thin_every=0)
    locs = [x.astype(np.float32) for x in locs]
    scales = [x.astype(np.float32) for x in scales]
    models = batch_models(O, family, 24, [x.astype(np.float64) for x in locs], [x.astype(np.float64) for x in scales])
    want = oracle_streams(O, coder, cfg, syms, models)
    flat, offsets, a32, b32 = flatten(B, syms, locs, scales, dtype=np.float32)
    assert a32.dtype == torch.float32 and b32.dtype == torch.float32
    enc = encode(flat, offsets, lo, hi, a32, b32, cfg)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == 0).all()
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = decode(enc, offsets, lo, hi, a32, b32)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_shape_mismatches_are_refused_in_python(B, form):
    lo, hi = -100, 100
    encode, decode, _, _ = calls(B, form)
    syms, locs, scales = workload(form[1], [4, 6], lo, hi, 1, thin_every=0)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    with pytest.raises(ValueError):
        encode(flat, offsets, lo, hi, a[:-1], b)
    with pytest.raises(ValueError):
        encode(flat.reshape(2, 5), offsets, lo, hi, a, b)
    with pytest.raises(ValueError):
        encode(flat, offsets, lo, hi, a.reshape(2, 5), b.reshape(2, 5))
    enc = encode(flat, offsets, lo, hi, a, b)
    with pytest.raises(ValueError):
        decode(enc, offsets[:-1], lo, hi, a, b)
    with pytest.raises(ValueError):
        decode(enc, offsets, lo, hi, a, b[:-1])


def test_an_unknown_family_is_refused_in_python(B):
    lo, hi = -100, 100
    syms, locs, scales = workload("laplace", [4, 6], lo, hi, 1, thin_every=0)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    enc = B.ans_encode_laplace_ragged(flat, offsets, lo, hi, a, b)
    renc = B.range_encode_laplace_ragged(flat, offsets, lo, hi, a, b)
    for family in ("gaussian", "binomial", 0, 3, 99):
        for fn in (B.ans_encode_family_ragged, B.range_encode_family_ragged):
            with pytest.raises(ValueError):
                fn(family, flat, offsets, lo, hi, a, b)
        with pytest.raises(ValueError):
            B.ans_decode_family_ragged(family, enc, offsets, lo, hi, a, b)
        with pytest.raises(ValueError):
            B.range_decode_family_ragged(family, renc, offsets, lo, hi, a, b)


def test_a_batch_of_the_other_coder_is_refused(B):
    """a RaggedBatch says which coder wrote it; the decoders of the other coder refuse it, the shared-model ragged decoder included"""
    lo, hi = -100, 100
    syms, locs, scales = workload("gaussian", [4, 6], lo, hi, 1, thin_every=0)
    flat, offsets, a, b = flatten(B, syms, locs, scales)
    by_ans = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, a, b)
    by_range = B.range_encode_gaussian_ragged(flat, offsets, lo, hi, a, b)
    assert by_ans.coder == "ans" and by_range.coder == "range"
    assert B.ans_encode_laplace_ragged(flat, offsets, lo, hi, a, b).coder == "ans"
    assert B.range_encode_cauchy_ragged(flat, offsets, lo, hi, a, b).coder == "range"
    for decode in (B.range_decode_gaussian_ragged, B.range_decode_laplace_ragged, B.range_decode_cauchy_ragged):
        with pytest.raises(ValueError):
            decode(by_ans, offsets, lo, hi, a, b)
    for decode in (B.ans_decode_gaussian_ragged, B.ans_decode_laplace_ragged, B.ans_decode_cauchy_ragged):
        with pytest.raises(ValueError):
            decode(by_range, offsets, lo, hi, a, b)
    model = B.Model.quantized_gaussian(lo, hi, 0.0, 10.0, 24)
    with pytest.raises(ValueError):
        B.ans_decode_ragged(by_range, model, offsets)
