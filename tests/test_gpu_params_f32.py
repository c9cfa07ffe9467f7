"""GPU tests of float32 per-symbol parameters read by the kernels themselves: a PAIR of float32 `means` / `stds`
(`a` / `b`) tensors goes to the _f32 entry points unconverted, and every word, count, status and jump-table entry must be the one the
float64 call gives on the widened tensors -- which is what the reference computes for a float32 caller (src/pybindings/mod.rs:187-214).

Parameters are drawn as float64, rounded to float32 and handed over as float32 tensors.  The rectangular test takes its expected words
from the CPU oracle on the WIDENED values, built as tests/test_gpu_per_symbol_batch.py and tests/test_gpu_family_batch.py build theirs
(one oracle coder per stream; computed once per (family, coder, configuration, shape) and shared by every route); everywhere the
float64 `batched` call on `x.double()` must agree bit for bit.  The shapes are the smallest that cross every boundary of the float
paths: the wave-decoder / by-rows routes (fewer than 64 streams), partial waves, rows shorter than, equal to and one past the 16- and
32-symbol request sizes (a 128-byte line is 32 floats), whole-line and general parameter requests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ["gaussian", "laplace", "cauchy"]
CONFIGS = [(32, 64, 24), (32, 64, 12), (16, 32, 12)]
SHAPES = [(1, 300), (3, 33), (33, 31), (64, 32), (64, 64), (65, 48), (130, 17)]
cfg_id = lambda c: "W%dS%dP%d" % c


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


def support(P):
    return (-100, 100) if P == 24 else (-60, 60)


def draw(rng, family, loc, scale):
    if family == "gaussian":
        return loc + scale * rng.standard_normal(loc.shape)
    return rng.laplace(loc, scale) if family == "laplace" else loc + scale * rng.standard_cauchy(loc.shape)


def workload(family, shape, lo, hi, seed):
    """tests/test_gpu_family_batch.py::workload with the parameters rounded to float32: (symbols, a32, b32)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo * 0.6, hi * 0.6, shape).astype(np.float32)
    b = np.exp(rng.uniform(np.log(0.3), np.log(40.0), shape)).astype(np.float32)
    sym = np.clip(np.rint(draw(rng, family, a.astype(np.float64), b.astype(np.float64))), lo, hi).astype(np.int32)
    if len(shape) == 2 and shape[1] >= 2:
        sym[:, :2] = np.array([lo, hi])
    return sym, a, b


def oracle_words(O, family, coder, cfg, lo, hi, sym, a, b):
    """get_compressed() of one oracle coder for one stream; a / b are float64 (the widened values)"""
    W, S, P = cfg
    if family == "gaussian":
        bits = 32 if W == 32 else 16
        if coder == "ans":
            c = O.AnsCoder(W=W, S=S)
            c.encode_gaussian_reverse(sym, lo, hi, a, b, P, bits)
        else:
            c = O.RangeEncoder(W=W, S=S)
            c.encode(sym, [O.GaussianModel(lo, hi, m, d, P, bits) for m, d in zip(a, b)], P)
        return c.get_compressed()
    fam = O.FAMILY_LAPLACE if family == "laplace" else O.FAMILY_CAUCHY
    models = [O.TableModel(O.leaky_family_cdf(fam, lo, hi, x, y, P), lo, P) for x, y in zip(a, b)]
    c = O.AnsCoder(W=W, S=S) if coder == "ans" else O.RangeEncoder(W=W, S=S)
    (c.encode_reverse if coder == "ans" else c.encode)(sym, models, P)
    return c.get_compressed()


_DATA = {}          # (family, P, shape) -> (sym, a32, b32)
_WANT = {}          # (family, coder, cfg, shape) -> [words of every stream]; never modified


def expected(O, family, coder, cfg, shape):
    lo, hi = support(cfg[2])
    dkey = (family, cfg[2], shape)
    if dkey not in _DATA:
        _DATA[dkey] = workload(family, shape, lo, hi, shape[0] * 13 + shape[1] + cfg[2])
    sym, a, b = _DATA[dkey]
    key = (family, coder, cfg, shape)
    if key not in _WANT:
        _WANT[key] = [oracle_words(O, family, coder, cfg, lo, hi, sym[s], a[s].astype(np.float64), b[s].astype(np.float64)) for s in range(shape[0])]
    return sym, a, b, _WANT[key]


def rect_calls(B, family, coder):
    """(encode, decode) with the Gaussian calls' jump points switched off (the family calls have none)"""
    enc, dec = getattr(B, f"{coder}_encode_{family}"), getattr(B, f"{coder}_decode_{family}")
    if family == "gaussian":
        return (lambda *a, **k: enc(*a, jump_points=0, **k)), dec
    return enc, dec


def route_names(family, coder, n_streams, n_per, n_symbols, fused, small):
    """the kernel names of a rectangular encode and decode: (f32 encode, f32 decode, f64 encode, f64 decode).  None: the f64 call has
    never recorded that route (cst_range_encode_gaussian_batch; the Gaussian's wave decoder), so cst_last_kernel_name() is stale there."""
    enc = f"{coder}_encode_{family}_" + ("fused_kernel" if fused else "two_pass")
    if n_streams >= 64:
        dec, tags = f"{coder}_decode_{family}_lane_kernel", (["small"] if small else [])
    elif n_symbols < 256 and n_per >= 32:
        dec, tags = f"decode_{family}_by_rows", []
    else:
        dec, tags = f"{coder}_decode_{family}_wave_kernel", []
    tagged = lambda name, t: name + ("<" + ", ".join(t) + ">" if t else "")
    enc64 = None if (family == "gaussian" and coder == "range") else enc
    dec64 = None if (family == "gaussian" and "wave" in dec) else tagged(dec, tags)
    return enc + "<f32>", tagged(dec, tags + ["f32"]), enc64, dec64


@pytest.mark.parametrize("geo", ["big", "small"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_pass"])
@pytest.mark.parametrize("layout", ["stream_major", "symbol_major"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_rectangular_parity(B, O, knob, family, coder, cfg, layout, fused, geo):
    knob(CST_FUSED_MIN_STREAMS="1" if fused else "1000000000", CST_LANE_GEO=geo)
    lo, hi = support(cfg[2])
    encode, decode = rect_calls(B, family, coder)
    t = (lambda m: m.T) if layout == "symbol_major" else (lambda m: m)
    for shape in SHAPES:
        what = f"{shape}"
        sym, a, b, want = expected(O, family, coder, cfg, shape)
        n_streams, n_per = shape
        d_sym, a32, b32 = dev(t(sym)), dev(t(a)), dev(t(b))
        assert a32.dtype == torch.float32 and b32.dtype == torch.float32
        e32, d32, e64, d64 = route_names(family, coder, n_streams, n_per, hi - lo + 1, fused, geo == "small")
        enc = encode(d_sym, lo, hi, a32, b32, cfg, layout)
        assert B.last_kernel() == e32, what
        words, n_words, status = enc.to_numpy()
        assert (status == 0).all(), what
        for s in range(n_streams):
            assert words[s, : n_words[s]].tolist() == want[s].tolist(), f"{what} stream {s}"
        # ... and the float64 call on the widened tensors: the same words, counts and statuses, under its own kernel name
        enc64 = encode(d_sym, lo, hi, a32.double(), b32.double(), cfg, layout)
        if e64 is not None:
            assert B.last_kernel() == e64 and "f32" not in B.last_kernel(), what
        words64, n_words64, status64 = enc64.to_numpy()
        assert np.array_equal(n_words, n_words64) and np.array_equal(status, status64), what
        for s in range(n_streams):
            assert np.array_equal(words[s, : n_words[s]], words64[s, : n_words[s]]), f"{what} stream {s}"
        dec, dstatus = decode(enc, lo, hi, a32, b32, layout)
        assert B.last_kernel() == d32, what
        assert (dstatus.cpu().numpy() == 0).all() and np.array_equal(t(dec.cpu().numpy()), sym), what
        dec64, dstatus64 = decode(enc, lo, hi, a32.double(), b32.double(), layout)
        if d64 is not None:
            assert B.last_kernel() == d64 and "f32" not in B.last_kernel(), what
        assert torch.equal(dec, dec64) and torch.equal(dstatus, dstatus64), what
        if coder == "ans":
            packed, offsets = B.compact(enc)
            dec2, st2 = decode((packed, enc.n_words), lo, hi, a32, b32, layout, offsets=offsets, config=cfg)
            assert B.last_kernel() == d32, what
            assert (st2.cpu().numpy() == 0).all() and np.array_equal(t(dec2.cpu().numpy()), sym), what


def assert_same_batch(enc, ref, what=""):
    words, n_words, status = enc.to_numpy()
    words_r, n_words_r, status_r = ref.to_numpy()
    assert np.array_equal(n_words, n_words_r) and np.array_equal(status, status_r), what
    for s in range(len(n_words)):
        assert np.array_equal(words[s, : n_words[s]], words_r[s, : n_words[s]]), f"{what} stream {s}"


@pytest.mark.parametrize("n_streams", [64, 65])
@pytest.mark.parametrize("points", [2, 4])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_jump_points(B, coder, points, n_streams):
    """jump_points= of the Gaussian calls: the tables and words of the float64 call, and the decode through the points"""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    sym, a, b = workload("gaussian", (n_streams, 64), lo, hi, 7 * n_streams + points)
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    encode, decode = getattr(B, f"{coder}_encode_gaussian"), getattr(B, f"{coder}_decode_gaussian")
    enc = encode(d_sym, lo, hi, a32, b32, cfg, jump_points=points)
    assert B.last_kernel() == f"{coder}_encode_gaussian_fused_kernel<ckpt, f32>"
    ref = encode(d_sym, lo, hi, a32.double(), b32.double(), cfg, jump_points=points)
    assert B.last_kernel() == f"{coder}_encode_gaussian_fused_kernel<ckpt>"
    assert (enc.status.cpu().numpy() == 0).all()
    assert_same_batch(enc, ref)
    assert enc.jump is not None and enc.jump.interval == 64 // points == ref.jump.interval
    for field in (("pos", "state") if coder == "ans" else ("pos", "lower", "range")):
        assert torch.equal(getattr(enc.jump, field), getattr(ref.jump, field)), field
    dec, status = decode(enc, lo, hi, a32, b32)
    assert "f32" in B.last_kernel() and "lane_kernel" in B.last_kernel()
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    dec64, status64 = decode(enc, lo, hi, a32.double(), b32.double())
    assert "f32" not in B.last_kernel()
    assert torch.equal(dec, dec64) and torch.equal(status, status64)


@pytest.mark.parametrize("n_streams", [64, 65])
def test_ans_gaussian_checkpointed(B, n_streams):
    cfg, interval = (32, 64, 24), 16
    lo, hi = support(24)
    sym, a, b = workload("gaussian", (n_streams, 64), lo, hi, 3 * n_streams)
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    enc, ck = B.ans_encode_gaussian_checkpointed(d_sym, lo, hi, a32, b32, interval, cfg)
    assert B.last_kernel() == "ans_encode_gaussian_fused_kernel<ckpt, f32>"
    ref, ck_ref = B.ans_encode_gaussian_checkpointed(d_sym, lo, hi, a32.double(), b32.double(), interval, cfg)
    assert B.last_kernel() == "ans_encode_gaussian_fused_kernel<ckpt>"
    assert (enc.status.cpu().numpy() == 0).all()
    assert_same_batch(enc, ref)
    assert torch.equal(ck.pos, ck_ref.pos) and torch.equal(ck.state, ck_ref.state)
    dec, status = B.ans_decode_gaussian_checkpointed(enc, ck, lo, hi, a32, b32)
    assert B.last_kernel() == "ans_decode_gaussian_lane_kernel<f32>"
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    dec64, status64 = B.ans_decode_gaussian_checkpointed(enc, ck, lo, hi, a32.double(), b32.double())
    assert B.last_kernel() == "ans_decode_gaussian_lane_kernel"
    assert torch.equal(dec, dec64) and torch.equal(status, status64)


# ---- ragged ----
EDGE_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 600]
_RAGGED = {}


def ragged_batch(B, family):
    """the edge lengths plus 70 streams of 1 .. 40 symbols: (lengths, flat symbols, offsets, a32, b32), built once per family"""
    if family not in _RAGGED:
        rng = np.random.default_rng(len(family))
        lengths = EDGE_LENGTHS + rng.integers(1, 41, 70).tolist()
        lo, hi = support(24)
        sym, a, b = workload(family, (sum(lengths),), lo, hi, 90 + len(family))
        flat, offsets = B.ragged([sym[o: o + n] for o, n in zip(np.cumsum([0] + lengths[:-1]), lengths)])
        _RAGGED[family] = (lengths, flat, offsets, dev(a), dev(b))
    return _RAGGED[family]


def ragged_streams(enc):
    words = enc.words.cpu().numpy().view(np.uint32)
    off, n = enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    return [words[off[s]: off[s] + n[s]].tolist() for s in range(len(n))], n.tolist(), enc.status.cpu().numpy().tolist()


def jump_fields(coder):
    return ("chunk_offsets", "pos", "state") if coder == "ans" else ("chunk_offsets", "pos", "lower", "range")


@pytest.mark.parametrize("jump_every", [0, 16, 256])
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_ragged(B, family, coder, jump_every):
    cfg = (32, 64, 24)
    lo, hi = support(24)
    lengths, flat, offsets, a32, b32 = ragged_batch(B, family)
    encode, decode = getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged")
    tag = lambda name, f32: name + ("<" + ", ".join((["jump"] if jump_every else []) + (["f32"] if f32 else [])) + ">" if jump_every or f32 else "")
    enc = encode(flat, offsets, lo, hi, a32, b32, cfg, jump_every=jump_every)
    assert B.last_kernel() == tag(f"{coder}_encode_{family}_ragged_kernel", True)
    ref = encode(flat, offsets, lo, hi, a32.double(), b32.double(), cfg, jump_every=jump_every)
    assert B.last_kernel() == tag(f"{coder}_encode_{family}_ragged_kernel", False)
    got, want = ragged_streams(enc), ragged_streams(ref)
    assert all(s == 0 for s in got[2]) and got == want
    if jump_every:
        n_chunks = sum((n + jump_every - 1) // jump_every for n in lengths)
        for field in jump_fields(coder):
            x, y = getattr(enc.jump, field), getattr(ref.jump, field)
            if field != "chunk_offsets":
                x, y = x[:n_chunks], y[:n_chunks]              # (entries behind the last chunk stay unused)
            assert torch.equal(x, y), field
    else:
        assert enc.jump is None
    dec, status = decode(enc, offsets, lo, hi, a32, b32)
    assert B.last_kernel() == tag(f"{coder}_decode_{family}_ragged_kernel", True)
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
    dec64, status64 = decode(enc, offsets, lo, hi, a32.double(), b32.double())
    assert B.last_kernel() == tag(f"{coder}_decode_{family}_ragged_kernel", False)
    assert torch.equal(dec, dec64) and torch.equal(status, status64)


@pytest.mark.parametrize("jump_every", [0, 16])
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_select(B, family, coder, jump_every):
    """queries equal slices of the full decode (which is the input): a whole stream, a range, a range that crosses a jump point, an empty
    stream, and one query beyond its stream -- refused with a non-zero status, and nothing of its slice written"""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    lengths, flat, offsets, a32, b32 = ragged_batch(B, family)
    enc = getattr(B, f"{coder}_encode_{family}_ragged")(flat, offsets, lo, hi, a32, b32, cfg, jump_every=jump_every)
    select = getattr(B, f"{coder}_decode_{family}_ragged_select")
    assert lengths[11] == 600 and lengths[10] == 257 and lengths[9] == 256 and lengths[0] == 0
    queries = [(11, 0, 600), (10, 5, 20), (11, 10, 20), (0, 0, 0), (9, 250, 20)]
    streams, first, count = (torch.tensor(x, dtype=torch.int64, device="cuda") for x in zip(*queries))
    out = torch.full((sum(q[2] for q in queries),), -7, dtype=torch.int32, device="cuda")
    sym, out_offsets, status = select(enc, offsets, lo, hi, a32, b32, streams, first, count, out=out)
    assert B.last_kernel() == f"{coder}_decode_{family}_ragged_kernel<select, f32>"
    out64 = torch.full_like(out, -7)
    sym64, out_offsets64, status64 = select(enc, offsets, lo, hi, a32.double(), b32.double(), streams, first, count, out=out64)
    assert B.last_kernel() == f"{coder}_decode_{family}_ragged_kernel<select>"
    assert torch.equal(sym, sym64) and torch.equal(out_offsets, out_offsets64) and torch.equal(status, status64)
    status, oo, sym, off = status.cpu().tolist(), out_offsets.cpu().tolist(), sym.cpu().numpy(), offsets.cpu().numpy()
    flat_h = flat.cpu().numpy()
    assert status[:4] == [0, 0, 0, 0] and status[4] != 0
    for q, (s, f, c) in enumerate(queries[:4]):
        assert oo[q + 1] - oo[q] == c
        assert np.array_equal(sym[oo[q]: oo[q + 1]], flat_h[off[s] + f: off[s] + f + c]), q
    assert (sym[oo[4]: oo[5]] == -7).all() and oo[5] - oo[4] == 20


@pytest.mark.parametrize("geo", ["big", "small"])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_parameter_tensors_that_start_between_16_byte_boundaries(B, knob, coder, geo):
    """the lane decoder's whole-line requests read 16 bytes at a time and need rows that start on 16 bytes: a float32 tensor whose
    storage starts 4 bytes further (a view into a larger buffer) takes the other requests, to the same symbols"""
    knob(CST_LANE_GEO=geo)
    cfg = (32, 64, 24)
    lo, hi = support(24)
    sym, a, b = workload("gaussian", (64, 64), lo, hi, 77)
    d_sym = dev(sym)
    shifted = lambda x: torch.cat([torch.zeros(1, dtype=torch.float32, device="cuda"), dev(x).reshape(-1)])[1:].view(64, 64)
    a32, b32 = shifted(a), shifted(b)
    assert a32.is_contiguous() and a32.data_ptr() % 16 == 4 and b32.data_ptr() % 16 == 4
    encode, decode = rect_calls(B, "gaussian", coder)
    enc = encode(d_sym, lo, hi, a32, b32, cfg)
    assert_same_batch(enc, encode(d_sym, lo, hi, dev(a), dev(b), cfg))
    dec, status = decode(enc, lo, hi, a32, b32)
    assert B.last_kernel().endswith("f32>")
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


# ---- exact widening ----
def edge_batch(shape=(70, 24)):
    """float32 parameters with the values at the edges of the format in the first columns of every stream, and three streams with an
    invalid scale"""
    lo, hi = support(24)
    sym, a, b = workload("gaussian", shape, lo, hi, 4)
    f = np.float32
    a[:, 2:10] = np.array([1e-40, -1e-40, 0.0, -0.0, 1.17549435e-38, -1.17549435e-38, 3e38, -3e38], dtype=f)
    b[:, 10:13] = np.array([1e-40, 1.17549435e-38, 3e38], dtype=f)
    a[:, 13] = f(1e-40); b[:, 13] = f(1e-40)            # a needle at a subnormal mean
    sym[:, 13] = 0
    assert a[0, 2] != 0 and a[0, 2] < np.finfo(f).tiny and b[0, 10] != 0 and b[0, 10] < np.finfo(f).tiny      # subnormal, not flushed here
    b[5, 7], b[6, 8], b[7, 9] = f("nan"), f("inf"), f(0.0)
    return lo, hi, sym, a, b


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_pass"])
@pytest.mark.parametrize("n_streams", [70, 33], ids=["lane", "wave"])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_exact_widening_at_the_edges(B, knob, coder, n_streams, fused):
    """every float32 bit pattern widens to the f64 of the same value inside the kernels: subnormals, signed zeros, the smallest normal
    and the largest magnitudes give the statuses and words of the float64 call on x.double(), stream for stream; NaN, +inf and 0.0 scales
    cost their own stream and nobody else's"""
    knob(CST_FUSED_MIN_STREAMS="1" if fused else "1000000000")
    cfg = (32, 64, 24)
    lo, hi, sym, a, b = edge_batch()
    sym, a, b = sym[:n_streams], a[:n_streams], b[:n_streams]
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    a64, b64 = a32.double(), b32.double()
    assert torch.equal(a64.cpu(), torch.from_numpy(a.astype(np.float64))) and a64[0, 2].item() == float(np.float32(1e-40)) != 0.0
    encode, decode = rect_calls(B, "gaussian", coder)
    enc = encode(d_sym, lo, hi, a32, b32, cfg)
    assert "f32" in B.last_kernel() and ("fused" in B.last_kernel()) == fused
    ref = encode(d_sym, lo, hi, a64, b64, cfg)
    assert_same_batch(enc, ref)
    status = enc.status.cpu().numpy()
    assert (status[[5, 6, 7]] != 0).all() and (np.delete(status, [5, 6, 7]) == 0).all()
    dec, dstatus = decode(ref, lo, hi, a32, b32)
    assert B.last_kernel().endswith("lane_kernel<f32>" if n_streams >= 64 else "wave_kernel<f32>")
    dec64, dstatus64 = decode(ref, lo, hi, a64, b64)
    assert torch.equal(dstatus, dstatus64)
    dstatus = dstatus.cpu().numpy()
    assert (dstatus[[5, 6, 7]] != 0).all() and (np.delete(dstatus, [5, 6, 7]) == 0).all()
    good = np.delete(np.arange(n_streams), [5, 6, 7])
    assert np.array_equal(dec.cpu().numpy()[good], sym[good]) and torch.equal(dec[good], dec64[good])


@pytest.mark.parametrize("geo", ["big", "small"])
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_exact_widening_through_whole_line_requests(B, knob, coder, geo):
    """rows of 24 never fill a 32-float line, so the batch above reaches the lane decoders through their single-tile requests only: the
    same values in 64 x 32 go through the vector loads of a whole-line request and land part by part, in both geometries"""
    knob(CST_LANE_GEO=geo)
    cfg = (32, 64, 24)
    lo, hi, sym, a, b = edge_batch((64, 32))
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    encode, decode = rect_calls(B, "gaussian", coder)
    ref = encode(d_sym, lo, hi, a32.double(), b32.double(), cfg)
    dec, dstatus = decode(ref, lo, hi, a32, b32)
    assert B.last_kernel() == f"{coder}_decode_gaussian_lane_kernel<" + ("small, " if geo == "small" else "") + "f32>"
    dec64, dstatus64 = decode(ref, lo, hi, a32.double(), b32.double())
    assert torch.equal(dstatus, dstatus64)
    dstatus = dstatus.cpu().numpy()
    assert (dstatus[[5, 6, 7]] != 0).all() and (np.delete(dstatus, [5, 6, 7]) == 0).all()
    good = np.delete(np.arange(64), [5, 6, 7])
    assert np.array_equal(dec.cpu().numpy()[good], sym[good]) and torch.equal(dec[good], dec64[good])


# ---- no widened copy ----
def peak_of(fn):
    """peak of the caching allocator's live bytes during fn(), above the level before it"""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    result = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, result


def test_no_widened_copy(B):
    """A float32 call allocates less than ONE widened array (8 n bytes) more than the float64 call on tensors widened beforehand: the
    conversion in front of the float64 entry points allocated two (16 n)."""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    n_streams, n_per = 64, 4096
    n = n_streams * n_per
    sym, a, b = workload("gaussian", (n_streams, n_per), lo, hi, 12)
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    a64, b64 = a32.double(), b32.double()
    new_batch = lambda: B.EncodedBatch(torch.empty((n_streams, B.max_words(n_per, cfg)), dtype=torch.int32, device="cuda"),
                                       torch.empty(n_streams, dtype=torch.int32, device="cuda"),
                                       torch.empty(n_streams, dtype=torch.int32, device="cuda"), cfg)
    out64, out32 = new_batch(), new_batch()
    p64, _ = peak_of(lambda: B.ans_encode_gaussian(d_sym, lo, hi, a64, b64, cfg, out=out64, jump_points=0))
    p32, _ = peak_of(lambda: B.ans_encode_gaussian(d_sym, lo, hi, a32, b32, cfg, out=out32, jump_points=0))
    print(f"rectangular encode: peak {p64} (f64) {p32} (f32), one widened array {8 * n}")
    assert "f32" in B.last_kernel()
    assert p32 - p64 < 8 * n
    assert_same_batch(out32, out64)
    dec64, dec32 = torch.empty_like(d_sym), torch.empty_like(d_sym)
    p64, _ = peak_of(lambda: B.ans_decode_gaussian(out64, lo, hi, a64, b64, out=dec64))
    p32, _ = peak_of(lambda: B.ans_decode_gaussian(out64, lo, hi, a32, b32, out=dec32))
    print(f"rectangular decode: peak {p64} (f64) {p32} (f32)")
    assert p32 - p64 < 8 * n
    assert torch.equal(dec32, d_sym) and torch.equal(dec64, d_sym)
    # ragged: the same elements as 64 streams of 4096
    flat, offsets = d_sym.reshape(-1), torch.arange(0, n + 1, n_per, dtype=torch.int64, device="cuda")
    fa32, fb32, fa64, fb64 = a32.reshape(-1), b32.reshape(-1), a64.reshape(-1), b64.reshape(-1)
    p64, r64 = peak_of(lambda: B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, fa64, fb64, cfg))
    p32, r32 = peak_of(lambda: B.ans_encode_gaussian_ragged(flat, offsets, lo, hi, fa32, fb32, cfg))
    print(f"ragged encode: peak {p64} (f64) {p32} (f32)")
    assert p32 - p64 < 8 * n
    assert ragged_streams(r32) == ragged_streams(r64)
    dec64, dec32 = torch.empty_like(flat), torch.empty_like(flat)
    p64, _ = peak_of(lambda: B.ans_decode_gaussian_ragged(r64, offsets, lo, hi, fa64, fb64, out=dec64))
    p32, _ = peak_of(lambda: B.ans_decode_gaussian_ragged(r64, offsets, lo, hi, fa32, fb32, out=dec32))
    print(f"ragged decode: peak {p64} (f64) {p32} (f32)")
    assert p32 - p64 < 8 * n
    assert torch.equal(dec32, flat) and torch.equal(dec64, flat)


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_mixed_dtypes_are_widened(B, coder):
    """(float32 mean, float64 std) and the reverse: widened, the float64 call's words under its kernel names"""
    cfg = (32, 64, 24)
    lo, hi = support(24)
    sym, a, b = workload("laplace", (70, 40), lo, hi, 31)
    d_sym, a32, b32 = dev(sym), dev(a), dev(b)
    encode, decode = getattr(B, f"{coder}_encode_laplace"), getattr(B, f"{coder}_decode_laplace")
    ref = encode(d_sym, lo, hi, a32.double(), b32.double(), cfg)
    for pa, pb in ((a32, b32.double()), (a32.double(), b32)):
        enc = encode(d_sym, lo, hi, pa, pb, cfg)
        assert "f32" not in B.last_kernel()
        assert_same_batch(enc, ref)
        dec, status = decode(enc, lo, hi, pa, pb)
        assert "f32" not in B.last_kernel()
        assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    flat, offsets = d_sym.reshape(-1), torch.arange(0, sym.size + 1, 40, dtype=torch.int64, device="cuda")
    rag = getattr(B, f"{coder}_encode_laplace_ragged")(flat, offsets, lo, hi, a32.reshape(-1), b32.double().reshape(-1), cfg)
    assert "f32" not in B.last_kernel()
    got = ragged_streams(rag)
    words, n_words, _ = ref.to_numpy()
    assert got[0] == [words[s, : n_words[s]].view(np.uint32).tolist() for s in range(70)]
