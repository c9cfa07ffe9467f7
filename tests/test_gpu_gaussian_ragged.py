"""GPU parity tests of per-symbol Gaussian coding for streams of DIFFERENT lengths (batched.ans_{encode,decode}_gaussian_ragged,
cst_ans_{encode,decode}_gaussian_ragged): every stream's words against one CPU oracle coder for that stream alone -- the
reference's `encode_reverse(symbols, QuantizedGaussian(lo, hi), means, stds)` + `get_compressed()` -- and the decode round trip.
Every stream of every batch is compared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CONFIGS = [(32, 64, 24), (32, 64, 12), (16, 32, 12)]
# more than one encoder workgroup (128 streams), several decoder waves and a partial last wave; lengths around the encoder's
# 16-symbol tiles and the decoder's 8-symbol tiles and 16-symbol output tiles, empty streams at both ends of a wave's slots
EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 700, 0]


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


def workload(lengths, lo, hi, seed, thin_every=5):
    """per stream what tests/test_gpu_per_symbol_batch.py::workload draws per row: mu uniform in 0.6 [lo, hi], sd log-uniform in
    0.3 .. 40, symbols clipped draws plus lo and hi themselves; every `thin_every`-th non-empty stream is needle-thin (sd = 1e-3 at
    mu = 0.6 lo, uniform symbols): about P bits per symbol, the most a stream can need"""
    rng = np.random.default_rng(seed)
    syms, mus, sds, non_empty = [], [], [], 0
    for n in lengths:
        n = int(n)
        mu = rng.uniform(lo * 0.6, hi * 0.6, n)
        sd = np.exp(rng.uniform(np.log(0.3), np.log(40.0), n))
        sym = np.clip(np.rint(mu + sd * rng.standard_normal(n)), lo, hi).astype(np.int32)
        sym[:2] = np.array([lo, hi])[: min(2, n)]
        if n > 0:
            non_empty += 1
            if thin_every and non_empty % thin_every == 0:
                mu = np.full(n, 0.6 * lo)
                sd = np.full(n, 1e-3)
                sym = rng.integers(lo, hi + 1, n).astype(np.int32)
        syms.append(sym); mus.append(mu); sds.append(sd)
    return syms, mus, sds


def flatten(B, syms, mus, sds, dtype=np.float64):
    flat, offsets = B.ragged(syms)
    cat = lambda xs: np.concatenate(xs).astype(dtype) if len(xs) else np.zeros(0, dtype)
    return flat, offsets, dev(cat(mus)), dev(cat(sds))


def oracle_streams(O, cfg, lo, hi, syms, mus, sds):
    """get_compressed() of one oracle AnsCoder per stream (a zero-length stream: no words)"""
    W, S, P = cfg
    want = []
    for sym, mu, sd in zip(syms, mus, sds):
        if len(sym) == 0:
            want.append(np.zeros(0, np.uint32))
            continue
        c = O.AnsCoder(W=W, S=S)
        c.encode_gaussian_reverse(sym, lo, hi, np.asarray(mu, np.float64), np.asarray(sd, np.float64), P, 32 if W == 32 else 16)
        want.append(np.asarray(c.get_compressed()))
    return want


def batch_streams(enc):
    """every stream's words of a RaggedBatch, with one copy to the host"""
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n[s]] for s in range(len(n))], n


def assert_streams_equal(got, n_words, want, what=""):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert n_words[s] == len(w) and g.tolist() == w.tolist(), f"{what}stream {s}: {n_words[s]} words, the oracle has {len(w)}"


_BIG = {}


def big_batch(O, cfg):
    """the 300-stream batch of the parity test and its oracle words: computed once per configuration, never modified"""
    if cfg not in _BIG:
        lo, hi = support(cfg[2])
        rng = np.random.default_rng(1000 + cfg[2] + cfg[0])
        lengths = EDGE_LENGTHS + rng.integers(0, 120, 286).tolist()
        syms, mus, sds = workload(lengths, lo, hi, 77 + cfg[2] + cfg[0])
        _BIG[cfg] = (lengths, syms, mus, sds, oracle_streams(O, cfg, lo, hi, syms, mus, sds))
    return _BIG[cfg]


def check_against_oracle(B, O, cfg, syms, mus, sds, want, **kw):
    lo, hi = support(cfg[2])
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg, **kw)
    torch.cuda.synchronize()
    assert B.last_kernel() == "ans_encode_gaussian_ragged_kernel"
    assert enc.jump is None
    assert (enc.status.cpu().numpy() == 0).all(), enc.status.cpu().tolist()
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd)
    torch.cuda.synchronize()
    assert B.last_kernel() == "ans_decode_gaussian_ragged_kernel"
    assert (status.cpu().numpy() == 0).all(), status.cpu().tolist()
    assert torch.equal(dec, flat)
    return enc


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "W%dS%dP%d" % c)
def test_every_stream_equals_its_oracle_coder(B, O, cfg):
    """300 streams of 0 .. 700 symbols, every fifth non-empty one needle-thin (about P bits per symbol): statuses, counts
    and words of every stream are the oracle's, and decoding returns the flat input"""
    lengths, syms, mus, sds, want = big_batch(O, cfg)
    assert len(lengths) == 300
    enc = check_against_oracle(B, O, cfg, syms, mus, sds, want)
    # the slabs are min(n, ceil(n P / W)) + S / W words rounded up to 4, and (all statuses being 0) no stream needed more; on the
    # oracle the thin streams of this input come within S / W .. S / W + 2 words of that bound
    slabs = np.diff(enc.word_offsets.cpu().numpy())
    W, S, P = cfg
    n = np.asarray(lengths)
    bound = np.minimum(n, (n * P + W - 1) // W) + S // W
    assert slabs.tolist() == ((bound + 3) // 4 * 4).tolist()
    assert (enc.n_words.cpu().numpy() <= bound).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("lengths", [[37], list(range(33))], ids=["one_stream", "33_streams"])
def test_one_stream_and_the_encoder_wave_boundary(B, O, cfg, lengths):
    """a single stream; 33 streams of 0 .. 32 symbols: a zero-length stream first and one stream in a second encoder wave"""
    lo, hi = support(cfg[2])
    syms, mus, sds = workload(lengths, lo, hi, 5 + len(lengths) + cfg[2])
    check_against_oracle(B, O, cfg, syms, mus, sds, oracle_streams(O, cfg, lo, hi, syms, mus, sds))


def test_same_words_as_the_rectangular_call(B):
    """96 streams of 40 symbols each: the ragged call and ans_encode_gaussian (no jump points) give every stream the same words"""
    cfg, lo, hi = (32, 64, 24), -100, 100
    syms, mus, sds = workload([40] * 96, lo, hi, 4040)
    rect = B.ans_encode_gaussian(dev(np.stack(syms)), lo, hi, dev(np.stack(mus)), dev(np.stack(sds)), cfg, jump_points=0)
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg)
    torch.cuda.synchronize()
    words, n_words, status = rect.to_numpy()
    assert (status == 0).all() and (enc.status.cpu().numpy() == 0).all()
    got, n = batch_streams(enc)
    assert_streams_equal(got, n, [words[s, : n_words[s]].view(np.uint32) for s in range(96)])


def test_a_bad_stream_does_not_touch_its_neighbours(B, O):
    """sd = 0 in stream 1, a NaN mean in stream 3, a symbol above the support in stream 4: exactly those streams are flagged
    (no words), streams 0 and 2 are the oracle's, and the good streams decode"""
    cfg, lo, hi = (32, 64, 24), -100, 100
    syms, mus, sds = workload((5, 64, 0, 300, 17), lo, hi, 31, thin_every=0)
    good = oracle_streams(O, cfg, lo, hi, syms, mus, sds)
    sds[1][40] = 0.0
    mus[3][123] = np.nan
    syms[4][9] = hi + 1
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [0, 1, 0, 1, 1]
    got, n_words = batch_streams(enc)
    assert [int(n_words[s]) for s in (1, 3, 4)] == [0, 0, 0]
    for s in (0, 2):
        assert n_words[s] == len(good[s]) and got[s].tolist() == good[s].tolist()
    # the same batch without the bad streams
    keep = (0, 2)
    flat2, offsets2, mu2, sd2 = flatten(B, [syms[s] for s in keep], [mus[s] for s in keep], [sds[s] for s in keep])
    enc2 = B.ans_encode_gaussian_ragged(flat2, offsets2, lo, hi, mu2, sd2, cfg)
    dec, status = B.ans_decode_gaussian_ragged(enc2, offsets2, lo, hi, mu2, sd2)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and torch.equal(dec, flat2)
    got2, n2 = batch_streams(enc2)
    assert_streams_equal(got2, n2, [good[s] for s in keep])


def test_corrupt_word_metadata(B):
    """decoder: a count of 2^30 and an offset of 2^40 (both leave the buffer whose numel is the call's words_capacity) give those
    streams status 3 and leave the others as they were; encoder: word offsets that run backwards give that stream
    CST_STREAM_CAPACITY and nothing is written outside the other streams' slabs"""
    from constriction_amd import _native as N
    cfg, lo, hi = (32, 64, 24), -100, 100
    syms, mus, sds = workload((5, 64, 300, 17), lo, hi, 32, thin_every=0)
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg)
    ref, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0] and torch.equal(ref, flat)
    enc.n_words[1] = 1 << 30
    enc.word_offsets[2] = 1 << 40
    dec, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd)
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
    N.check(N.lib().cst_ans_encode_gaussian_ragged(N.CoderConfig(*cfg), lo, hi, p(flat), p(mu), p(sd), p(offsets), n, None, p(words), p(woff), 0,
                                                   p(n_words), p(status), None), "cst_ans_encode_gaussian_ragged")
    torch.cuda.synchronize()
    st, nw, w = status.cpu().tolist(), n_words.cpu().numpy(), words.cpu().numpy()
    assert st == [0, 2, 0, 0] and nw[1] == 0
    # slabs: stream 0 = [0, 64), stream 2 = [32, 512), stream 3 = [512, 1024); nothing else is written
    assert (w[1024:] == 0x5A5A5A5A).all()
    assert (w[nw[0]: 32] == 0x5A5A5A5A).all() and (w[32 + nw[2]: 512] == 0x5A5A5A5A).all() and (w[512 + nw[3]: 1024] == 0x5A5A5A5A).all()
    # (streams 0 and 2 overlap in [32, 64) by this construction: stream 0 has fewer than 32 words)
    assert nw[0] <= 32


def test_results_do_not_depend_on_the_schedule(B, O):
    """the parity batch at (32,64,24) with no schedule, sorted, reversed and shuffled: words, counts and statuses are the same
    per stream, and so are the decoded symbols"""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    lengths, syms, mus, sds, want = big_batch(O, cfg)
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    n = len(lengths)
    rng = np.random.default_rng(9)
    schedules = [None, "sorted", dev(np.arange(n - 1, -1, -1).astype(np.int32)), dev(rng.permutation(n).astype(np.int32))]
    for order in schedules:
        enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg, order=order)
        torch.cuda.synchronize()
        assert B.last_kernel() == "ans_encode_gaussian_ragged_kernel"
        assert (enc.status.cpu().numpy() == 0).all()
        assert (enc.order is None) == (order is None)
        got, n_words = batch_streams(enc)
        assert_streams_equal(got, n_words, want, what=f"order {order if order is None or isinstance(order, str) else 'tensor'}: ")
        dec, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd, order=order if order is None else "auto")
        torch.cuda.synchronize()
        assert B.last_kernel() == "ans_decode_gaussian_ragged_kernel"
        assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
    # ... and a decoder schedule keyed on the word counts, on a batch encoded without one
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd, cfg, order=None)
    dec, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd, order="sorted")
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


def test_float32_parameters_are_widened(B, O):
    """float32 means / stds: the models are those of the widened values (as the reference's Python API casts them)"""
    cfg, lo, hi = (32, 64, 24), -100, 100
    lengths = [0, 3, 50, 16, 129, 1]
    syms, mus, sds = workload(lengths, lo, hi, 66, thin_every=0)
    mus = [m.astype(np.float32) for m in mus]
    sds = [s.astype(np.float32) for s in sds]
    want = oracle_streams(O, cfg, lo, hi, syms, [m.astype(np.float64) for m in mus], [s.astype(np.float64) for s in sds])
    flat, offsets, mu32, sd32 = flatten(B, syms, mus, sds, dtype=np.float32)
    assert mu32.dtype == torch.float32 and sd32.dtype == torch.float32
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu32, sd32, cfg)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == 0).all()
    got, n_words = batch_streams(enc)
    assert_streams_equal(got, n_words, want)
    dec, status = B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu32, sd32)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


def test_shape_mismatches_are_refused_in_python(B):
    lo, hi = -100, 100
    syms, mus, sds = workload([4, 6], lo, hi, 1, thin_every=0)
    flat, offsets, mu, sd = flatten(B, syms, mus, sds)
    with pytest.raises(ValueError):
        B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu[:-1], sd)
    with pytest.raises(ValueError):
        B.ans_encode_gaussian_ragged(flat.reshape(2, 5), offsets, lo, hi, mu, sd)
    with pytest.raises(ValueError):
        B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu.reshape(2, 5), sd.reshape(2, 5))
    enc = B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, mu, sd)
    with pytest.raises(ValueError):
        B.ans_decode_gaussian_ragged(enc, offsets[:-1], lo, hi, mu, sd)
    with pytest.raises(ValueError):
        B.ans_decode_gaussian_ragged(enc, offsets, lo, hi, mu, sd[:-1])
