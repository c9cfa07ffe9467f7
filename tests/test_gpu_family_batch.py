"""GPU tests of the BATCHED per-symbol QuantizedLaplace / QuantizedCauchy calls (constriction_amd.batched.*_family and their
named forms): `encode_reverse(symbols, QuantizedLaplace(lo, hi), means, scales)` / `decode(QuantizedCauchy(lo, hi), locs, scales)`
(src/pybindings/stream/model.rs:736-900) for many coders at once, with the CDF evaluated inside the coder kernels.

Every expected word and symbol comes from the CPU oracle: one tabulated model per symbol from the oracle's own restatement of
the family (oracle.leaky_family_cdf: LeakyQuantizer<f64, i32, u32, P> over the `probability` crate's CDFs), fed to one oracle
coder per stream.  The u32 tables serve the (16, 32, 12) preset too: free_weight is the same and every product stays below 2^12.
No GPU result is the reference for another."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ["laplace", "cauchy"]


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


def fam_id(O, family):
    return O.FAMILY_LAPLACE if family == "laplace" else O.FAMILY_CAUCHY


def draw(rng, family, loc, scale):
    return rng.laplace(loc, scale) if family == "laplace" else loc + scale * rng.standard_cauchy(loc.shape)


def workload(family, n_streams, n_per, lo, hi, seed):
    """location uniform in 0.6 [lo, hi], scale log-uniform in [0.3, 40], symbols drawn from the model and clipped, the two ends
    of the support in front of every stream"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo * 0.6, hi * 0.6, (n_streams, n_per))
    b = np.exp(rng.uniform(np.log(0.3), np.log(40.0), (n_streams, n_per)))
    sym = np.clip(np.rint(draw(rng, family, a, b)), lo, hi).astype(np.int32)
    sym[:, :2] = np.array([lo, hi])[: min(2, n_per)]
    return sym, a, b


def models_of(O, family, lo, hi, a, b, P):
    return [O.TableModel(O.leaky_family_cdf(fam_id(O, family), lo, hi, x, y, P), lo, P) for x, y in zip(a, b)]


def oracle_words(O, coder, cfg, sym, models):
    W, S, P = cfg
    if coder == "ans":
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return c.get_compressed()


_expected = {}          # (family, coder, cfg, shape) -> (sym, a, b, [words of every stream]); both layouts share it


def expected(O, family, coder, cfg, n_streams, n_per):
    key = (family, coder, cfg, n_streams, n_per)
    if key not in _expected:
        P = cfg[2]
        lo, hi = (-100, 100) if P == 24 else (-60, 60)
        mkey = (family, P, n_streams, n_per)
        if mkey not in _expected:
            sym, a, b = workload(family, n_streams, n_per, lo, hi, n_streams * 13 + n_per + P)
            _expected[mkey] = (sym, a, b, [models_of(O, family, lo, hi, a[s], b[s], P) for s in range(n_streams)])
        sym, a, b, models = _expected[mkey]
        _expected[key] = (lo, hi, sym, a, b, [oracle_words(O, coder, cfg, sym[s], models[s]) for s in range(n_streams)])
    return _expected[key]


@pytest.mark.parametrize("layout", ["stream_major", "symbol_major"])
@pytest.mark.parametrize("n_streams,n_per", [(1, 300), (65, 40), (1000, 21)])
@pytest.mark.parametrize("cfg", [(32, 64, 24), (32, 64, 12), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_batch_parity(B, O, family, coder, cfg, n_streams, n_per, layout, knob):
    lo, hi, sym, a, b, want = expected(O, family, coder, cfg, n_streams, n_per)
    t = (lambda m: m.T) if layout == "symbol_major" else (lambda m: m)
    enc_fn = getattr(B, f"{coder}_encode_{family}")
    dec_fn = getattr(B, f"{coder}_decode_{family}")
    d_sym, d_a, d_b = dev(t(sym)), dev(t(a)), dev(t(b))
    # from 64 streams on: both encoders (CST_FUSED_MIN_STREAMS moves the fused kernel's threshold of 16 384 streams)
    for min_streams in (("1", "1000000000") if n_streams >= 64 else (None,)):
        if min_streams is not None:
            knob(CST_FUSED_MIN_STREAMS=min_streams)
        enc = enc_fn(d_sym, lo, hi, d_a, d_b, cfg, layout)
        torch.cuda.synchronize()
        if min_streams is not None:
            assert B.last_kernel() == f"{coder}_encode_{family}_" + ("fused_kernel" if min_streams == "1" else "two_pass")
        words, n_words, status = enc.to_numpy()
        assert (status == 0).all()
        for s in range(n_streams):
            assert words[s, : n_words[s]].tolist() == want[s].tolist(), f"stream {s} (CST_FUSED_MIN_STREAMS={min_streams})"
    dec, dstatus = dec_fn(enc, lo, hi, d_a, d_b, layout)
    torch.cuda.synchronize()
    if n_streams >= 64:
        assert B.last_kernel() == f"{coder}_decode_{family}_lane_kernel"
    assert (dstatus.cpu().numpy() == 0).all()
    assert np.array_equal(t(dec.cpu().numpy()), sym)
    if coder == "ans":
        packed, offsets = B.compact(enc)
        dec2, st2 = dec_fn((packed, enc.n_words), lo, hi, d_a, d_b, layout, offsets=offsets, config=cfg)
        torch.cuda.synchronize()
        assert (st2.cpu().numpy() == 0).all()
        assert np.array_equal(t(dec2.cpu().numpy()), sym)


@pytest.mark.parametrize("n_streams", [130, 3])          # a lane per stream / cdf rows or a wave per stream
@pytest.mark.parametrize("cfg", [(32, 64, 24), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("family", FAMILIES)
def test_family_decode_of_random_words_extreme_models(B, O, family, cfg, n_streams):
    """Decoding RANDOM words draws every quantile, the far tails included, and the models here are the hard ones for a search
    that starts from an inverse-CDF guess in f32: needle-thin and enormous scales, locations far outside the support (all the
    mass in the leak), supports of two symbols and supports where the leak outweighs the distribution.  The oracle builds a
    valid table for every such row, so every stream must decode -- to the oracle's symbols."""
    W, S, P = cfg
    rng = np.random.default_rng(P + len(family))
    n_per = 70
    for lo, hi in ((-100, 100), (0, 1), (-5, 2000 if P == 24 else 900), (-127, 127)):
        a = rng.uniform(lo - 50.0, hi + 50.0, (n_streams, n_per))
        b = np.exp(rng.uniform(np.log(1e-7), np.log(1e6), (n_streams, n_per)))
        a[:, 0] = lo - 1e9; a[:, 1] = hi + 1e9; b[:, 2] = 1e-300; b[:, 3] = 1e300
        stride = 160
        words = rng.integers(1, 1 << W, (n_streams, stride), dtype=np.uint64).astype(np.uint32)
        enc = B.EncodedBatch(dev(words.view(np.int32)), dev(np.full(n_streams, stride, np.int32)), dev(np.zeros(n_streams, np.int32)), cfg)
        dec, st = B.ans_decode_family(family, enc, lo, hi, dev(a), dev(b))
        torch.cuda.synchronize()
        dec = dec.cpu().numpy()
        assert (st.cpu().numpy() == 0).all(), (lo, hi)
        for s in range(0, n_streams, 3 if n_streams > 3 else 1):
            comp = words[s] if W == 32 else words[s].astype(np.uint16)
            want = O.AnsCoder(comp, W=W, S=S).decode(models_of(O, family, lo, hi, a[s], b[s], P), P=P)
            assert dec[s].tolist() == want.tolist(), f"stream {s} support [{lo}, {hi}]"


@pytest.mark.parametrize("layout", ["stream_major", "symbol_major"])
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_few_long_streams_in_pieces(B, O, family, coder, layout):
    """Fewer streams than lanes and a support below 256 symbols: the decoder tabulates cdf rows piece by piece and parks the coders
    between pieces.  40 streams x 2000 symbols = two pieces of 1600 symbols; one stream has a zero scale in the second piece
    (that stream fails there, with everything before it delivered; all other streams are unaffected)."""
    lo, hi, cfg = -100, 100, (32, 64, 24)
    n_streams, n_per = 40, 2000
    sym, a, b = workload(family, n_streams, n_per, lo, hi, 99)
    t = (lambda m: m.T) if layout == "symbol_major" else (lambda m: m)
    enc = getattr(B, f"{coder}_encode_family")(family, dev(t(sym)), lo, hi, dev(t(a)), dev(t(b)), cfg, layout)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == 0).all()
    for s in (0, 5, 17, 26, 39):
        assert enc.stream(s).tolist() == oracle_words(O, coder, cfg, sym[s], models_of(O, family, lo, hi, a[s], b[s], 24)).tolist(), f"stream {s}"
    dec_fn = getattr(B, f"{coder}_decode_family")
    dec, st = dec_fn(family, enc, lo, hi, dev(t(a)), dev(t(b)), layout)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"decode_{family}_by_rows"
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(t(dec.cpu().numpy()), sym)
    b_bad = b.copy()
    b_bad[5, 1700] = 0.0
    dec, st = dec_fn(family, enc, lo, hi, dev(t(a)), dev(t(b_bad)), layout)
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert st[5] == 1 and (np.delete(st, 5) == 0).all()
    got = t(dec.cpu().numpy())
    assert np.array_equal(np.delete(got, 5, axis=0), np.delete(sym, 5, axis=0))
    assert np.array_equal(got[5, :1700], sym[5, :1700])


@pytest.mark.parametrize("family", FAMILIES)
def test_family_batch_errors_and_edges(B, O, family, knob):
    lo, hi, cfg = -30, 30, (32, 64, 24)
    sym, a, b = workload(family, 70, 25, lo, hi, 5)
    good = sym.copy()
    sym[9, 3] = hi + 1                                  # impossible symbol -> that stream only
    b[11, 7] = 0.0                                      # invalid model -> that stream only (the reference panics)
    for enc_fn in (B.ans_encode_family, B.range_encode_family):
        enc = enc_fn(family, dev(sym), lo, hi, dev(a), dev(b), cfg)
        torch.cuda.synchronize()
        st = enc.status.cpu().numpy()
        assert st[9] == 1 and st[11] == 1 and (np.delete(st, [9, 11]) == 0).all()
        with pytest.raises(ValueError):
            enc_fn(family, dev(sym), lo, hi, dev(a[:, :5]), dev(b), cfg)
    with pytest.raises(ValueError):
        B.ans_decode_family(family, enc, lo, hi, dev(a), dev(b[:, :5]))
    with pytest.raises(ValueError):
        B.ans_encode_family("binomial", dev(sym), lo, hi, dev(a), dev(b), cfg)
    # a zero scale fails its own stream in the lane decoder too
    b_ok = np.where(b > 0.0, b, 1.0)
    enc = B.range_encode_family(family, dev(good), lo, hi, dev(a), dev(b_ok), cfg)
    dec, st = B.range_decode_family(family, enc, lo, hi, dev(a), dev(b))
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert st[11] == 1 and (np.delete(st, 11) == 0).all()
    assert np.array_equal(np.delete(dec.cpu().numpy(), 11, axis=0), np.delete(good, 11, axis=0))
    # supports wider than 65536 symbols work in both directions (P = 24)
    lo2, hi2 = -40000, 40000
    rng = np.random.default_rng(11)
    a2 = rng.uniform(lo2 * 0.6, hi2 * 0.6, (3, 50))
    b2 = np.exp(rng.uniform(np.log(0.3), np.log(40.0), (3, 50))) * 300
    sym2 = np.clip(np.rint(draw(rng, family, a2, b2)), lo2, hi2).astype(np.int32)
    enc2 = B.ans_encode_family(family, dev(sym2), lo2, hi2, dev(a2), dev(b2), cfg)
    dec2, st2 = B.ans_decode_family(family, enc2, lo2, hi2, dev(a2), dev(b2))
    torch.cuda.synchronize()
    assert (enc2.status.cpu().numpy() == 0).all() and (st2.cpu().numpy() == 0).all()
    assert np.array_equal(dec2.cpu().numpy(), sym2)
    assert enc2.stream(1).tolist() == oracle_words(O, "ans", cfg, sym2[1], models_of(O, family, lo2, hi2, a2[1], b2[1], 24)).tolist()
    # a partial wave in both geometries of the lane decoder
    sym3, a3, b3 = workload(family, 65, 40, -100, 100, 77)
    for coder in ("ans", "range"):
        enc3 = getattr(B, f"{coder}_encode_family")(family, dev(sym3), -100, 100, dev(a3), dev(b3), cfg)
        for geo in ("small", "big"):
            knob(CST_LANE_GEO=geo)
            dec3, st3 = getattr(B, f"{coder}_decode_family")(family, enc3, -100, 100, dev(a3), dev(b3))
            torch.cuda.synchronize()
            assert B.last_kernel() == f"{coder}_decode_{family}_lane_kernel" + ("<small>" if geo == "small" else "")
            assert (st3.cpu().numpy() == 0).all() and np.array_equal(dec3.cpu().numpy(), sym3)


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_drop_in(B, O, family, coder):
    """stream.stack.AnsCoder / stream.queue.Range{Encoder,Decoder} with a QuantizedLaplace / QuantizedCauchy family and per-symbol
    parameters take the new calls: the oracle's words, a round trip, and no table rows on the way."""
    from constriction_amd import stream  # noqa: F401
    import constriction_amd
    mod, stack, queue = constriction_amd.stream.model, constriction_amd.stream.stack, constriction_amd.stream.queue
    lo, hi, n = -100, 100, 3000
    sym, a, b = workload(family, 1, n, lo, hi, 31)
    sym, a, b = sym[0], a[0], b[0]
    model = (mod.QuantizedLaplace if family == "laplace" else mod.QuantizedCauchy)(lo, hi)
    if coder == "ans":
        enc = stack.AnsCoder()
        enc.encode_reverse(sym, model, a, b)
        assert B.last_kernel() == f"ans_encode_{family}_two_pass"
        words = enc.get_compressed()
        dec = stack.AnsCoder(words)
    else:
        enc = queue.RangeEncoder()
        enc.encode(sym, model, a, b)
        assert B.last_kernel() == f"range_encode_{family}_two_pass"
        words = enc.get_compressed()
        dec = queue.RangeDecoder(words)
    assert words.tolist() == oracle_words(O, coder, (32, 64, 24), sym, models_of(O, family, lo, hi, a, b, 24)).tolist()
    got = dec.decode(model, a, b)
    assert B.last_kernel() == f"decode_{family}_by_rows"       # (the family's own rows in pieces, not cst_*_decode_rows_batch)
    assert np.array_equal(got, sym)
    with pytest.raises(ValueError):
        stack.AnsCoder().encode_reverse(sym[:5], model, a[:5], np.zeros(5))
