"""GPU tests of every per-symbol kernel (Gaussian, Laplace, Cauchy; ANS and range; rectangular, ragged, jump points, select) on the
ZOO of tests/per_symbol_extremes.py: needle-thin, enormous, subnormal and overflowing scales, locations far outside the support and
at +-DBL_MAX, a location exactly on a bin edge, supports of two symbols and supports that fill the precision, symbols of the smallest
and the largest probability -- and the boundary between valid and invalid parameters.

The encoders compute (left, prob) through lcp / lcp_quick, the decoders search with left / left3: two functions that must agree on
every cumulative.  So the two directions are tested apart: the encoders against the CPU oracle's WORDS, the decoders on slabs built on
the host from the oracle's words.  No GPU result is the reference for another.  tests/test_per_symbol_extremes_cpu.py checks the zoo
and the oracle's side of it without a GPU."""
import numpy as np
import pytest

import per_symbol_extremes as Z
import test_gpu_persymbol_ragged_jump as J
import test_gpu_ragged_per_symbol_forms as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

cfg_id = F.cfg_id
shape_id = lambda s: "%dx%d" % s
LAYOUTS = ["stream_major", "symbol_major"]
SHAPES = [(130, 70), (96, 80), (3, 70)]       # a partial third wave; whole waves and whole 16-symbol tiles (PAIR); fewer streams than lanes
RAGGED_LENGTHS = (0, 1, 15, 16, 17, 70, 300) * 10          # 70 streams: a wave boundary at 64 / 65
OK, IMPOSSIBLE = 0, 1


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from constriction_amd import batched
    return batched


dev = F.dev


def u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)


def rect_calls(B, family, coder):
    """(encode, decode) of a rectangular form; the Gaussian's encoders without the jump points they would choose themselves"""
    enc, dec = getattr(B, f"{coder}_encode_{family}"), getattr(B, f"{coder}_decode_{family}")
    if family == "gaussian":
        return (lambda *args: enc(*args, jump_points=0)), dec
    return enc, dec


def slab_words(B, coder, n_per, cfg):
    return (B.max_words if coder == "ans" else B.range_max_words)(n_per, cfg)


def host_batch(B, cfg, words, stride):
    """an EncodedBatch built on the host from the oracle's words, one slab of `stride` words per stream"""
    slabs = np.zeros((len(words), stride), np.uint32)
    for s, w in enumerate(words):
        assert len(w) <= stride
        slabs[s, : len(w)] = w
    n_words = np.array([len(w) for w in words], np.int32)
    return B.EncodedBatch(dev(slabs.view(np.int32)), dev(n_words), dev(np.zeros(len(words), np.int32)), tuple(cfg))


def host_ragged(B, cfg, coder, words, lengths=None, tables=None, every=0):
    """a RaggedBatch built on the host from the oracle's words (16-byte slabs), with the oracle's jump table if `tables`"""
    slabs = np.array([max(4, (len(w) + 3) // 4 * 4) for w in words], np.int64)
    off = np.concatenate([[0], np.cumsum(slabs)]).astype(np.int64)
    flat = np.zeros(int(off[-1]), np.uint32)
    for s, w in enumerate(words):
        flat[off[s]: off[s] + len(w)] = w
    jump = None
    if tables is not None:
        chunks = [-(-int(n) // every) for n in lengths]
        assert [len(t) for t in tables] == chunks
        rows = [row for t in tables for row in t]
        chunk_off = dev(np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64))
        pos = dev(np.array([r[0] for r in rows], np.uint32).view(np.int32))
        if coder == "ans":
            jump = B.RaggedJump(every, chunk_off, pos, dev(u64(r[1] for r in rows)))
        else:
            jump = B.RangeRaggedJump(every, chunk_off, pos, dev(u64(r[1] for r in rows)), dev(u64(r[2] for r in rows)))
    return B.RaggedBatch(dev(flat.view(np.int32)), dev(off), dev(np.array([len(w) for w in words], np.int32)),
                         dev(np.zeros(len(words), np.int32)), tuple(cfg), None, jump, coder)


def assert_rect_words(enc, want, what=""):
    words, n_words, status = enc.to_numpy()
    assert (status == OK).all(), f"{what}: statuses {status[status != 0][:5].tolist()} in streams {np.flatnonzero(status)[:5].tolist()}"
    for s, w in enumerate(want):
        assert n_words[s] == len(w) and words[s, : n_words[s]].tolist() == w.tolist(), f"{what}: stream {s}"


# ---------------------------------------------------------------------------------------------- a. rectangular encoders

@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_rectangular_encoders_write_the_oracles_words(B, family, coder, cfg, shape, knob):
    """the two-pass entry kernel and the fused kernel (from 64 streams on both, by CST_FUSED_MIN_STREAMS; (96, 80) stream-major at
    W = 32 is the Gaussian's whole-tile PAIR form), both layouts, four supports: status 0, counts and words of EVERY stream"""
    n_streams, n_per = shape
    encode, _ = rect_calls(B, family, coder)
    for lo, hi in Z.supports(cfg[2]):
        sym, a, b, want = Z.rect_expected(family, lo, hi, cfg, n_streams, n_per)
        for layout in LAYOUTS:
            t = (lambda m: m.T) if layout == "symbol_major" else (lambda m: m)
            d_sym, d_a, d_b = dev(t(sym)), dev(t(a)), dev(t(b))
            for min_streams in (("1", "1000000000") if n_streams >= 64 else (None,)):
                if min_streams is not None:
                    knob(CST_FUSED_MIN_STREAMS=min_streams)
                enc = encode(d_sym, lo, hi, d_a, d_b, cfg, layout)
                torch.cuda.synchronize()
                if min_streams is not None and (family, coder) != ("gaussian", "range"):     # (that call does not record its route)
                    assert B.last_kernel() == f"{coder}_encode_{family}_" + ("fused_kernel" if min_streams == "1" else "two_pass")
                assert_rect_words(enc, want[coder], f"[{lo}, {hi}] {layout} CST_FUSED_MIN_STREAMS={min_streams}")


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_rectangular_jump_points(B, coder, cfg):
    """(96, 64) with two jump points per stream (the fused kernel's <ckpt> form; the Gaussian's calls have them): the words are
    unchanged, every jump point is what the oracle coder reports at that position, and the oracle's words decode chunk-wise through
    the oracle's table"""
    W, S, P = cfg
    n_streams, n_per, k = 96, 64, 2
    every = n_per // k
    for lo, hi in Z.supports(P):
        sym, a, b, want = Z.rect_expected("gaussian", lo, hi, cfg, n_streams, n_per, every)
        want = want[coder]
        d_a, d_b = dev(a), dev(b)
        enc = getattr(B, f"{coder}_encode_gaussian")(dev(sym), lo, hi, d_a, d_b, cfg, jump_points=k)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_encode_gaussian_fused_kernel<ckpt>"
        assert_rect_words(enc, [w for w, _ in want], f"[{lo}, {hi}]")
        jump = enc.jump
        assert jump is not None and jump.interval == every and jump.pos.shape == (n_streams, k)
        arrays = [jump.pos.cpu().numpy().view(np.uint32)] + [x.cpu().numpy().view(np.uint64) for x in
                                                             ([jump.state] if coder == "ans" else [jump.lower, jump.range])]
        for s, (_, table) in enumerate(want):
            assert [tuple(int(x[s, j]) for x in arrays) for j in range(k)] == table, f"[{lo}, {hi}] stream {s}"
        # the decoder on the oracle's words and the oracle's table
        host = host_batch(B, cfg, [w for w, _ in want], slab_words(B, coder, n_per, cfg))
        cols = [u64(row[c] for _, table in want for row in table).reshape(n_streams, k) for c in range(len(arrays))]       # (Python ints: exact)
        pos, rest = dev(cols[0].astype(np.int32)), [dev(c) for c in cols[1:]]
        host.jump = B.Checkpoints(every, pos, *rest) if coder == "ans" else B.RangeCheckpoints(every, pos, *rest)
        for batch in (host, enc):
            dec, status = getattr(B, f"{coder}_decode_gaussian")(batch, lo, hi, d_a, d_b)
            torch.cuda.synchronize()
            assert B.last_kernel() == f"{coder}_decode_gaussian_lane_kernel"          # (192 chunks, a lane each)
            assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), sym), (lo, hi)


# ---------------------------------------------------------------------------------------------- b. rectangular decoders

@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_rectangular_decoders_read_the_oracles_words(B, family, coder, cfg, shape, knob):
    """slabs built on the host from the oracle's words: the lane decoder in both geometries (130 streams), in the one it chooses
    (96), the by-rows route or the wave-per-stream kernel (3 streams); both layouts: status 0 and the input symbols"""
    n_streams, n_per = shape
    _, decode = rect_calls(B, family, coder)
    for lo, hi in Z.supports(cfg[2]):
        sym, a, b, want = Z.rect_expected(family, lo, hi, cfg, n_streams, n_per)
        enc = host_batch(B, cfg, want[coder], slab_words(B, coder, n_per, cfg))
        for layout in LAYOUTS:
            t = (lambda m: m.T) if layout == "symbol_major" else (lambda m: m)
            d_a, d_b = dev(t(a)), dev(t(b))
            for geo in (("small", "big") if n_streams == 130 else (None,)):
                if geo is not None:
                    knob(CST_LANE_GEO=geo)
                dec, status = decode(enc, lo, hi, d_a, d_b, layout)
                torch.cuda.synchronize()
                if n_streams >= 64:
                    assert B.last_kernel() == f"{coder}_decode_{family}_lane_kernel" + ("<small>" if geo == "small" else "")
                elif hi - lo + 1 < 256:
                    assert B.last_kernel() == f"decode_{family}_by_rows"
                elif family != "gaussian":                                               # (the Gaussian's wave kernel records nothing)
                    assert B.last_kernel() == f"{coder}_decode_{family}_wave_kernel"
                what = f"[{lo}, {hi}] {layout} CST_LANE_GEO={geo}"
                status = status.cpu().numpy()
                assert (status == OK).all(), f"{what}: statuses {status[status != 0][:5].tolist()} in streams {np.flatnonzero(status)[:5].tolist()}"
                got = t(dec.cpu().numpy())
                for s in range(n_streams):
                    assert got[s].tolist() == sym[s].tolist(), f"{what}: stream {s}"


# ---------------------------------------------------------------------------------------------- c. ragged forms

def ragged_calls(B, family, coder):
    return (getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged"),
            getattr(B, f"{coder}_decode_{family}_ragged_select"), f"{coder}_encode_{family}_ragged_kernel", f"{coder}_decode_{family}_ragged_kernel")


@pytest.mark.parametrize("every", [0, 16])
@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_ragged_forms(B, family, coder, cfg, every):
    """70 streams of 0 .. 300 symbols, without jump points and with one in front of every tile (16 symbols: the smallest interval the
    encoders take), scheduled as they come and sorted: every container is its oracle coder's words, the jump table is the oracle's
    positions, and the oracle's containers (with the oracle's table) decode to the input"""
    lengths = RAGGED_LENGTHS
    encode, decode, _, enc_name, dec_name = ragged_calls(B, family, coder)
    for lo, hi in Z.supports(cfg[2]):
        syms, locs, scales, want = Z.ragged_expected(family, lo, hi, cfg, lengths, every)
        want = want[coder]
        words = [w for w, _ in want] if every else want
        flat, offsets, a, b = F.flatten(B, syms, locs, scales)
        host = host_ragged(B, cfg, coder, words, lengths, [t for _, t in want] if every else None, every)
        for order in ("auto", "sorted"):
            what = f"[{lo}, {hi}] order={order}: "
            enc = encode(flat, offsets, lo, hi, a, b, cfg, order=order, jump_every=every)
            torch.cuda.synchronize()
            assert B.last_kernel() == enc_name + ("<jump>" if every else "")
            assert (enc.status.cpu().numpy() == OK).all(), what + str(enc.status.cpu().tolist())
            got, n_words = F.batch_streams(enc)
            F.assert_streams_equal(got, n_words, words, what)
            if every:
                J.assert_tables_equal(B, enc, lengths, every, want)
            # "auto" takes the chunks of a jump table side by side; a schedule handed in runs whole streams
            dec, status = decode(host, offsets, lo, hi, a, b, order=order)
            torch.cuda.synchronize()
            assert B.last_kernel() == dec_name + ("<jump>" if every and order == "auto" else "")
            assert (status.cpu().numpy() == OK).all(), what + str(status.cpu().tolist())
            assert torch.equal(dec, flat), what + "decoded symbols"


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_ragged_select(B, family, coder, cfg):
    """one select call on the oracle's containers and the oracle's jump table: three whole streams and an inner range of a fourth"""
    lengths, every = RAGGED_LENGTHS, 16
    _, _, select, _, dec_name = ragged_calls(B, family, coder)
    for lo, hi in Z.supports(cfg[2])[:2]:
        syms, locs, scales, want = Z.ragged_expected(family, lo, hi, cfg, lengths, every)
        want = want[coder]
        flat, offsets, a, b = F.flatten(B, syms, locs, scales)
        host = host_ragged(B, cfg, coder, [w for w, _ in want], lengths, [t for _, t in want], every)
        queries = [(6, 0, 300), (68, 0, 70), (1, 0, 1), (13, 37, 150)]
        streams = torch.tensor([s for s, _, _ in queries], dtype=torch.int64, device="cuda")
        got, out_offsets, status = select(host, offsets, lo, hi, a, b, streams, [f for _, f, _ in queries], [c for _, _, c in queries])
        torch.cuda.synchronize()
        assert B.last_kernel() == dec_name + "<select>"
        assert status.cpu().tolist() == [OK] * len(queries)
        assert out_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([c for _, _, c in queries])]).tolist()
        assert got.cpu().tolist() == np.concatenate([syms[s][f: f + c] for s, f, c in queries]).tolist(), (lo, hi)


# ---------------------------------------------------------------------------------------------- d. the validity boundary

INF, NAN = float("inf"), float("nan")
VALID = [("b", Z.DENORM_MIN), ("b", Z.DBL_MIN), ("b", 1.3e308), ("b", Z.DBL_MAX), ("a", Z.DBL_MAX), ("a", -Z.DBL_MAX)]
INVALID = [("b", INF), ("b", -INF), ("b", NAN), ("b", 0.0), ("b", -0.0), ("b", -Z.DENORM_MIN), ("a", INF), ("a", -INF), ("a", NAN)]


def boundary_batch(family, lengths, lo, hi, cfg, seed):
    """A tame workload (tests/test_gpu_ragged_per_symbol_forms.py::workload) with every VALID value in a stream of its own and, in
    a second copy of the parameters, every INVALID value in three more streams of its own each: at the first, a middle and the last
    position.  Returns (syms, (locs, scales) valid only, (locs, scales) with the invalid ones, {stream: bad position}, oracle words of
    the valid-only parameters per coder)."""
    syms, locs, scales = F.workload(family, lengths, lo, hi, seed, thin_every=0)
    free = [s for s, n in enumerate(lengths) if n > 0]
    assert len(free) >= len(VALID) + 3 * len(INVALID)
    place = lambda n, k: (0, n // 2, n - 1)[k % 3]
    for k, (which, v) in enumerate(VALID):
        s = free.pop(0)
        (locs if which == "a" else scales)[s][place(lengths[s], k)] = v
    bad_locs, bad_scales, bad = [x.copy() for x in locs], [x.copy() for x in scales], {}
    for which, v in INVALID:
        for k in range(3):
            s = free.pop(0)
            bad[s] = place(lengths[s], k)
            (bad_locs if which == "a" else bad_scales)[s][bad[s]] = v
    W, S, P = cfg
    want = {"ans": [], "range": []}
    for sym, x, y in zip(syms, locs, scales):
        models = Z.models_of(family, lo, hi, x, y, P, W)
        for coder in want:
            want[coder].append(Z.oracle_words(coder, cfg, family, lo, hi, sym, x, y, models))
    return syms, (locs, scales), (bad_locs, bad_scales), bad, want


_BOUNDARY = {}


def boundary(family, lengths, cfg):
    key = (family, tuple(lengths), cfg)
    if key not in _BOUNDARY:
        lo, hi = F.support(cfg[2])
        _BOUNDARY[key] = (lo, hi) + boundary_batch(family, list(lengths), lo, hi, cfg, 50 + len(lengths) + cfg[2])
    return _BOUNDARY[key]


def check_statuses(status, bad, what):
    assert status.tolist() == [IMPOSSIBLE if s in bad else OK for s in range(len(status))], what


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", ["gaussian", "laplace"])
def test_validity_boundary_rectangular(B, family, coder, cfg, knob):
    """(70, 25).  Valid side: 5e-324, the smallest normal number, 1.3e308 and DBL_MAX as scales, +-DBL_MAX as locations -- status 0,
    the oracle's words, the input symbols.  Invalid side: +-inf, NaN, 0.0, -0.0 and -5e-324 as scales, +-inf and NaN as locations --
    exactly those streams report IMPOSSIBLE_SYMBOL, the encoders give them no words, the decoders deliver what lies in front of the
    bad position, and every other stream is the oracle's."""
    n_streams, n_per = 70, 25
    lo, hi, syms, ok, bad_params, bad, want = boundary(family, [n_per] * n_streams, cfg)
    sym = np.stack(syms)
    encode, decode = rect_calls(B, family, coder)
    host = host_batch(B, cfg, want[coder], slab_words(B, coder, n_per, cfg))
    for (locs, scales), flagged in ((ok, {}), (bad_params, bad)):
        d_a, d_b = dev(np.stack(locs)), dev(np.stack(scales))
        for min_streams in ("1", "1000000000"):
            knob(CST_FUSED_MIN_STREAMS=min_streams)
            enc = encode(dev(sym), lo, hi, d_a, d_b, cfg, "stream_major")
            torch.cuda.synchronize()
            words, n_words, status = enc.to_numpy()
            what = f"CST_FUSED_MIN_STREAMS={min_streams}, {len(flagged)} invalid streams"
            check_statuses(status, flagged, what)
            for s, w in enumerate(want[coder]):
                if s in flagged:
                    assert n_words[s] == 0, f"{what}: stream {s}"
                else:
                    assert n_words[s] == len(w) and words[s, : n_words[s]].tolist() == w.tolist(), f"{what}: stream {s}"
        dec, status = decode(host, lo, hi, d_a, d_b, "stream_major")
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_decode_{family}_lane_kernel"
        check_statuses(status.cpu().numpy(), flagged, f"decoder, {len(flagged)} invalid streams")
        got = dec.cpu().numpy()
        for s in range(n_streams):
            upto = flagged.get(s, n_per)
            assert got[s, :upto].tolist() == sym[s, :upto].tolist(), f"decoder, {len(flagged)} invalid streams: stream {s}"


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", ["gaussian", "laplace"])
def test_validity_boundary_ragged(B, family, coder, cfg):
    """the same for the ragged calls: (5, 64, 0, 300, 17) nine times over, so that every value has a stream of its own"""
    lengths = (5, 64, 0, 300, 17) * 9
    lo, hi, syms, ok, bad_params, bad, want = boundary(family, lengths, cfg)
    encode, decode, _, _, _ = ragged_calls(B, family, coder)
    host = host_ragged(B, cfg, coder, want[coder])
    for (locs, scales), flagged in ((ok, {}), (bad_params, bad)):
        flat, offsets, a, b = F.flatten(B, syms, locs, scales)
        enc = encode(flat, offsets, lo, hi, a, b, cfg)
        torch.cuda.synchronize()
        check_statuses(enc.status.cpu().numpy(), flagged, f"encoder, {len(flagged)} invalid streams")
        got, n_words = F.batch_streams(enc)
        for s, w in enumerate(want[coder]):
            if s in flagged:
                assert n_words[s] == 0, f"stream {s}"
            else:
                assert n_words[s] == len(w) and got[s].tolist() == w.tolist(), f"{len(flagged)} invalid streams: stream {s}"
        dec, status = decode(host, offsets, lo, hi, a, b)
        torch.cuda.synchronize()
        check_statuses(status.cpu().numpy(), flagged, f"decoder, {len(flagged)} invalid streams")
        dec, off = dec.cpu().numpy(), offsets.cpu().numpy()
        for s, sym in enumerate(syms):
            upto = flagged.get(s, len(sym))
            assert dec[off[s]: off[s] + upto].tolist() == sym[:upto].tolist(), f"decoder, {len(flagged)} invalid streams: stream {s}"


# ---------------------------------------------------------------------------------------------- e. a support that fills the precision

FULL = {}


def full_support_batch(family, hi, cfg, n_streams, n_per):
    key = (family, hi, cfg, n_streams, n_per)
    if key not in FULL:
        lo = -2048
        sym, a, b = Z.uniform_batch(lo, hi, n_streams, n_per, 4096 + hi + n_per)
        want = {"ans": [], "range": []}
        for s in range(n_streams):
            models = Z.models_of(family, lo, hi, a[s], b[s], cfg[2], cfg[0])
            for coder in want:
                want[coder].append(Z.oracle_words(coder, cfg, family, lo, hi, sym[s], a[s], b[s], models))
        FULL[key] = (sym, a, b, want)
    return FULL[key]


@pytest.mark.parametrize("hi", [2047, 2046], ids=["n=2^P", "n=2^P-1"])
@pytest.mark.parametrize("cfg", [(16, 32, 12), (32, 64, 12)], ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", ["gaussian", "laplace"])
def test_a_support_that_fills_the_precision(B, family, coder, cfg, hi, knob):
    """n = 2^P symbols: free weight 0, every probability 1, every symbol costs exactly P bits -- a model edge and the most words a
    slab of max_words / range_max_words has to hold; n = 2^P - 1 next to it.  (65, 100) through both rectangular encoders and the
    lane decoder, the same streams cut to ragged lengths through the ragged calls; uniform symbols."""
    W, S, P = cfg
    lo, n_streams, n_per = -2048, 65, 100
    sym, a, b, want = full_support_batch(family, hi, cfg, n_streams, n_per)
    encode, decode = rect_calls(B, family, coder)
    d_sym, d_a, d_b = dev(sym), dev(a), dev(b)
    for min_streams in ("1", "1000000000"):
        knob(CST_FUSED_MIN_STREAMS=min_streams)
        enc = encode(d_sym, lo, hi, d_a, d_b, cfg, "stream_major")
        torch.cuda.synchronize()
        assert enc.stride == slab_words(B, coder, n_per, cfg)
        assert_rect_words(enc, want[coder], f"CST_FUSED_MIN_STREAMS={min_streams}")
        assert int(enc.n_words.max().item()) >= n_per * P // W
    host = host_batch(B, cfg, want[coder], slab_words(B, coder, n_per, cfg))
    dec, status = decode(host, lo, hi, d_a, d_b, "stream_major")
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_decode_{family}_lane_kernel"
    assert (status.cpu().numpy() == OK).all() and np.array_equal(dec.cpu().numpy(), sym)
    # a short ragged batch: prefixes of the first streams (a prefix of a range coder's stream is not a prefix of its words: own oracle runs)
    lengths = [0, 1, 16, 17, 100, 33]
    syms, locs, scales = [sym[s, :n] for s, n in enumerate(lengths)], [a[s, :n] for s, n in enumerate(lengths)], [b[s, :n] for s, n in enumerate(lengths)]
    words = [Z.oracle_words(coder, cfg, family, lo, hi, x, y, z) for x, y, z in zip(syms, locs, scales)]
    r_encode, r_decode, _, _, _ = ragged_calls(B, family, coder)
    flat, offsets, ra, rb = F.flatten(B, syms, locs, scales)
    enc = r_encode(flat, offsets, lo, hi, ra, rb, cfg)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == OK).all()
    got, n_words = F.batch_streams(enc)
    F.assert_streams_equal(got, n_words, words)
    assert n_words[4] >= 100 * P // W
    dec, status = r_decode(host_ragged(B, cfg, coder, words), offsets, lo, hi, ra, rb)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == OK).all() and torch.equal(dec, flat)


@pytest.mark.parametrize("cfg", [(16, 32, 12), (32, 64, 12)], ids=cfg_id)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("family", ["gaussian", "laplace"])
def test_one_symbol_more_than_quantiles_is_refused(B, family, coder, cfg):
    """n = 2^P + 1 (LeakyQuantizer::new asserts n <= 2^P): CST_ERR_MODEL from the encode and the decode calls, rectangular and ragged"""
    lo, hi = -2048, 2048
    sym, a, b = Z.uniform_batch(lo, hi, 65, 20, 1)
    encode, decode = rect_calls(B, family, coder)
    r_encode, r_decode, select, _, _ = ragged_calls(B, family, coder)
    refused = lambda: pytest.raises(ValueError, match="model cannot be built")
    with refused():
        encode(dev(sym), lo, hi, dev(a), dev(b), cfg, "stream_major")
    ok = encode(dev(sym), lo, hi - 1, dev(a), dev(b), cfg, "stream_major")       # (sym may hold 2048: that stream fails, the call does not)
    with refused():
        decode(ok, lo, hi, dev(a), dev(b), "stream_major")
    flat, offsets, ra, rb = F.flatten(B, list(sym[:5]), list(a[:5]), list(b[:5]))
    with refused():
        r_encode(flat, offsets, lo, hi, ra, rb, cfg)
    r_ok = r_encode(flat, offsets, lo, hi - 1, ra, rb, cfg)
    with refused():
        r_decode(r_ok, offsets, lo, hi, ra, rb)
    with refused():
        select(r_ok, offsets, lo, hi, ra, rb, torch.tensor([0, 1], dtype=torch.int64, device="cuda"))
