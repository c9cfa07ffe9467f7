"""GPU tests of jump points for ragged per-symbol batches: `jump_every` of batched.{ans,range}_encode_{gaussian,laplace,cauchy}_ragged,
the chunk route of the matching decoders, and the C entry points cst_{ans,range}_{encode,decode}_{gaussian,family}_ragged_jump.

The reference is the CPU oracle alone: one coder per stream for the words, and the same coder coded chunk by chunk for the jump table
(tests/persymbol_jump_oracle.py, checked on its own in tests/test_persymbol_ragged_jump_cpu.py).  No GPU result is the reference for
another, except where a test says that two GPU calls must agree.  Workload and oracle helpers are those of
tests/test_gpu_ragged_per_symbol_forms.py; a batch and its oracle results are built once per (family, precision, interval) and shared."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_ragged_per_symbol_forms as F
from persymbol_jump_oracle import ans_table, range_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CONFIGS = [(32, 64, 24), (32, 64, 12), (16, 32, 12)]
FORMS = [(coder, family) for coder in ("ans", "range") for family in ("gaussian", "laplace", "cauchy")]
# all six forms at every = 48 (three tiles, no power of two); the two Gaussian forms also at one tile and at sixteen
PARITY = [(form, 48) for form in FORMS] + [((coder, "gaussian"), every) for coder in ("ans", "range") for every in (16, 256)]
form_id = F.form_id
cfg_id = F.cfg_id
OK, IMPOSSIBLE, INVALID = 0, 1, 3


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


def calls(B, form):
    coder, family = form
    return (getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged"),
            f"{coder}_encode_{family}_ragged_kernel", f"{coder}_decode_{family}_ragged_kernel")


def parity_lengths(every, seed):
    rng = np.random.default_rng(seed)
    lengths = ([0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 0]
               + [every - 1, every, every + 1, 2 * every - 1, 2 * every, 2 * every + 1, 5 * every + 7]
               + rng.integers(0, 121, 200).tolist() + rng.integers(300, 1201, 6).tolist())
    return [int(x) for x in rng.permutation(lengths)]


def oracle_batch(O, coder, cfg, syms, models, every):
    """per stream: (words, table) of one oracle coder, coded chunk by chunk"""
    table_of = ans_table if coder == "ans" else range_table
    return [table_of(O, cfg, sym, m, every) for sym, m in zip(syms, models)]


_BATCHES = {}       # (family, P, every) -> (lengths, syms, locs, scales, models): built once, never modified
_WANT = {}          # (form, cfg, every) -> [(words, table)] of that batch


def parity_batch(O, form, cfg, every):
    coder, family = form
    P = cfg[2]
    if (family, P, every) not in _BATCHES:
        lo, hi = F.support(P)
        lengths = parity_lengths(every, 500 + P + every)
        syms, locs, scales = F.workload(family, lengths, lo, hi, 91 + P + every)
        _BATCHES[(family, P, every)] = (lengths, syms, locs, scales, F.batch_models(O, family, P, locs, scales))
    lengths, syms, locs, scales, models = _BATCHES[(family, P, every)]
    if (form, cfg, every) not in _WANT:
        _WANT[(form, cfg, every)] = oracle_batch(O, coder, cfg, syms, models, every)
    return lengths, syms, locs, scales, models, _WANT[(form, cfg, every)]


def device_tables(enc):
    """the batch's jump table, per stream, as the oracle helpers give it: [(pos, state)] or [(pos, lower, range)]"""
    jump = enc.jump
    off = jump.chunk_offsets.cpu().numpy()
    pos = jump.pos.cpu().numpy().view(np.uint32)
    arrays = [jump.state] if enc.coder == "ans" else [jump.lower, jump.range]
    cols = [pos] + [a.cpu().numpy().view(np.uint64) for a in arrays]
    return [[tuple(int(c[k]) for c in cols) for k in range(off[s], off[s + 1])] for s in range(len(off) - 1)]


def assert_tables_equal(B, enc, lengths, every, want, skip=()):
    jump = enc.jump
    assert isinstance(jump, B.RaggedJump if enc.coder == "ans" else B.RangeRaggedJump) and jump.interval == every
    chunks = [-(-n // every) for n in lengths]
    assert jump.chunk_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(chunks)]).tolist()
    assert jump.pos.numel() >= sum(chunks)
    got = device_tables(enc)
    for s, (g, (_, w)) in enumerate(zip(got, want)):
        if s not in skip:
            assert g == w, f"stream {s} ({lengths[s]} symbols): the table differs from the oracle's"


def encode_and_compare(B, form, cfg, syms, locs, scales, lengths, every, want, order=None):
    """the jump encoder against the oracle (words, counts, statuses, table); returns the batch and the flat inputs"""
    lo, hi = F.support(cfg[2])
    encode, _, enc_name, _ = calls(B, form)
    flat, offsets, a, b = F.flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg, order=order, jump_every=every)
    torch.cuda.synchronize()
    assert B.last_kernel() == enc_name + "<jump>"
    assert enc.coder == form[0] and (enc.status.cpu().numpy() == 0).all(), enc.status.cpu().tolist()
    got, n_words = F.batch_streams(enc)
    F.assert_streams_equal(got, n_words, [w for w, _ in want])
    assert_tables_equal(B, enc, lengths, every, want)
    return enc, flat, offsets, a, b


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("form,every", PARITY, ids=lambda v: form_id(v) if isinstance(v, tuple) else f"every{v}")
def test_parity(B, O, form, every, cfg):
    """about 230 streams of 0 .. 1200 symbols around every tile and chunk boundary, every fifth non-empty one needle-thin"""
    lo, hi = F.support(cfg[2])
    encode, decode, enc_name, dec_name = calls(B, form)
    lengths, syms, locs, scales, models, want = parity_batch(O, form, cfg, every)
    n = len(lengths)
    assert n == 226 and sum(-(-x // every) for x in lengths) > (256 if every == 48 else 0)
    enc, flat, offsets, a, b = encode_and_compare(B, form, cfg, syms, locs, scales, lengths, every, want)
    # the plain call: the same words, counts, statuses and slabs, no table, today's kernel
    plain = encode(flat, offsets, lo, hi, a, b, cfg, order=None, jump_every=0)
    torch.cuda.synchronize()
    assert B.last_kernel() == enc_name and plain.jump is None
    assert torch.equal(plain.word_offsets, enc.word_offsets) and torch.equal(plain.n_words, enc.n_words) and torch.equal(plain.status, enc.status)
    got, n_words = F.batch_streams(enc)
    got_plain, n_plain = F.batch_streams(plain)
    F.assert_streams_equal(got, n_words, got_plain)
    # the chunk route ...
    dec, status = decode(enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert B.last_kernel() == dec_name + "<jump>"
    assert (status.cpu().numpy() == 0).all(), status.cpu().tolist()
    assert torch.equal(dec, flat)
    # ... and a schedule handed in: whole streams
    dec, status = decode(enc, offsets, lo, hi, a, b, order=torch.arange(n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert B.last_kernel() == dec_name
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
    if form[0] == "ans":
        # the oracle's seek on the DEVICE's words from the DEVICE's jump points: first, middle and last chunk of the longest stream
        W, S, P = cfg
        s = int(np.argmax(lengths))
        table = device_tables(enc)[s]
        for j in (0, len(table) // 2, len(table) - 1):
            c = O.AnsCoder(got[s], W=W, S=S)
            c.seek(*table[j])
            assert c.decode(models[s][j * every: (j + 1) * every], P=P).tolist() == syms[s][j * every: (j + 1) * every].tolist()


@pytest.mark.parametrize("n_streams", [1, 31, 32, 33, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "laplace")], ids=form_id)
def test_shapes_of_the_launch(B, O, form, n_streams):
    """stream counts around the encoder's 32 and the decoder's 64 lanes per wave and the workgroups; one-tile chunks"""
    cfg, every = (32, 64, 24), 16
    lo, hi = F.support(24)
    lengths = [(every - 1, every, every + 1, 3 * every, 0)[s % 5] for s in range(n_streams)]
    syms, locs, scales = F.workload(form[1], lengths, lo, hi, 7000 + n_streams)
    models = F.batch_models(O, form[1], 24, locs, scales)
    want = oracle_batch(O, form[0], cfg, syms, models, every)
    enc, flat, offsets, a, b = encode_and_compare(B, form, cfg, syms, locs, scales, lengths, every, want)
    dec, status = calls(B, form)[1](enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert B.last_kernel() == calls(B, form)[3] + "<jump>"
    assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)


@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "cauchy")], ids=form_id)
def test_schedule_does_not_change_results(B, O, form):
    cfg, every = (32, 64, 24), 48
    lengths, syms, locs, scales, models, want = parity_batch(O, form, cfg, every)
    rng = np.random.default_rng(3)
    for order in (None, "sorted", F.dev(rng.permutation(len(lengths)).astype(np.int32))):
        enc, flat, offsets, a, b = encode_and_compare(B, form, cfg, syms, locs, scales, lengths, every, want, order=order)
        assert (enc.order is None) == (order is None)


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_flagged_streams(B, O, form):
    """std <= 0 in a middle chunk of stream 2, a symbol outside the support in the last chunk of stream 5: those two report
    IMPOSSIBLE_SYMBOL and no words; every other stream's words and table are the oracle's and decode to their input.  Nothing is
    asserted about what the flagged streams decode to."""
    cfg, every = (32, 64, 24), 48
    lo, hi = F.support(24)
    encode, decode, _, _ = calls(B, form)
    lengths = [100, 0, 200, 47, 48, 150, 49, 500]
    syms, locs, scales = F.workload(form[1], lengths, lo, hi, 4321, thin_every=0)
    models = F.batch_models(O, form[1], 24, locs, scales)
    want = oracle_batch(O, form[0], cfg, syms, models, every)
    scales[2][100] = 0.0                                        # chunk 2 of 5
    syms[5][149] = hi + 1                                       # chunk 3 of 4, its last
    flagged = (2, 5)
    flat, offsets, a, b = F.flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert enc.status.cpu().tolist() == [IMPOSSIBLE if s in flagged else OK for s in range(len(lengths))]
    got, n_words = F.batch_streams(enc)
    for s, (w, _) in enumerate(want):
        if s in flagged:
            assert n_words[s] == 0
        else:
            assert n_words[s] == len(w) and got[s].tolist() == w.tolist(), s
    assert_tables_equal(B, enc, lengths, every, want, skip=flagged)
    dec, status = decode(enc, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    st, off = status.cpu().tolist(), offsets.cpu().numpy()
    for s in range(len(lengths)):
        if s not in flagged:
            assert st[s] == OK and torch.equal(dec[off[s]: off[s + 1]], flat[off[s]: off[s + 1]]), s


def copy_of(B, enc):
    """the batch with a copy of its table"""
    jump = enc.jump
    fields = {k: getattr(jump, k).clone() if torch.is_tensor(getattr(jump, k)) else getattr(jump, k) for k in jump.__dataclass_fields__}
    table = type(jump)(**fields)
    return B.RaggedBatch(enc.words, enc.word_offsets, enc.n_words, enc.status, enc.config, enc.order, table, enc.coder)


@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "gaussian"), ("ans", "cauchy"), ("range", "laplace")], ids=form_id)
def test_tables_are_checked(B, form):
    """tables that do not describe their batch: the stream concerned reports INVALID_DATA, all others still decode (the decoder
    clamps or rejects every index derived from the table before it is an address: persymbol_jump_chunks_kernel)"""
    cfg, every = (32, 64, 24), 48
    lo, hi = F.support(24)
    encode, decode, _, dec_name = calls(B, form)
    lengths = [100, 0, 200, 47, 48, 150, 49, 500, 96]
    syms, locs, scales = F.workload(form[1], lengths, lo, hi, 99, thin_every=0)
    flat, offsets, a, b = F.flatten(B, syms, locs, scales)
    enc = encode(flat, offsets, lo, hi, a, b, cfg, jump_every=every)
    torch.cuda.synchronize()
    assert (enc.status.cpu().numpy() == 0).all()
    off = offsets.cpu().numpy()
    chunk_off = enc.jump.chunk_offsets.cpu().numpy()

    def others_decode(dec, status, bad):
        st = status.cpu().tolist()
        assert [st[s] for s in bad] == [INVALID] * len(bad), st
        for s in range(len(lengths)):
            if s not in bad:
                assert st[s] == OK and torch.equal(dec[off[s]: off[s + 1]], flat[off[s]: off[s + 1]]), s

    # (1) a jump point one word beyond its stream's words: chunk 1 of stream 5
    bad = copy_of(B, enc)
    bad.jump.pos[chunk_off[5] + 1] = int(enc.n_words[5].item()) + 1
    dec, status = decode(bad, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    assert B.last_kernel() == dec_name + "<jump>"
    others_decode(dec, status, (5,))
    # (2) one chunk too many for stream 2: its successors keep their chunk counts, so only stream 2 is not described -- and the last
    #     stream's chunks reach one entry further, which the table arrays hold (an upper bound sizes them)
    bad = copy_of(B, enc)
    assert bad.jump.pos.numel() > chunk_off[-1] + 1
    shifted = chunk_off.copy()
    shifted[3:] += 1
    bad.jump.chunk_offsets = F.dev(shifted)
    for name in ("pos", "state", "lower", "range"):
        if hasattr(bad.jump, name):      # the entries of streams 3 .. move one up with their offsets
            t = getattr(bad.jump, name)
            t[chunk_off[3] + 1: chunk_off[-1] + 1] = getattr(enc.jump, name)[chunk_off[3]: chunk_off[-1]]
    dec, status = decode(bad, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    others_decode(dec, status, (2,))
    # (3) n_chunks_total as an upper bound: the arrays are longer than the table (sized without a read-back), and longer still
    assert enc.jump.pos.numel() > chunk_off[-1]
    big = copy_of(B, enc)
    for name in ("pos", "state", "lower", "range"):
        if hasattr(big.jump, name):
            t = getattr(big.jump, name)
            setattr(big.jump, name, torch.cat([t, torch.full((100,), -1, dtype=t.dtype, device=t.device)]))
    dec, status = decode(big, offsets, lo, hi, a, b)
    torch.cuda.synchronize()
    others_decode(dec, status, ())


@pytest.mark.parametrize("form", [("ans", "gaussian"), ("range", "cauchy")], ids=form_id)
def test_c_abi_with_slabs(B, O, form):
    """the C entry points with d_word_offsets = NULL: stream s owns words[s * stride_words .. + stride_words)"""
    from constriction_amd import _native as N
    coder, family = form
    cfg, every = (32, 64, 24), 32
    lo, hi = F.support(24)
    lengths = [0, 1, 31, 32, 33, 64, 65, 200, 96, 17]
    syms, locs, scales = F.workload(family, lengths, lo, hi, 555)
    models = F.batch_models(O, family, 24, locs, scales)
    want = oracle_batch(O, coder, cfg, syms, models, every)
    flat, offsets, a, b = F.flatten(B, syms, locs, scales)
    n, stride = len(lengths), 208
    chunks = [-(-x // every) for x in lengths]
    chunk_off = F.dev(np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64))
    n_chunks = sum(chunks) + 3                                   # an upper bound
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
    words, n_words, status = torch.full((n * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), z(n, torch.int32), z(n, torch.int32)
    table = [z(n_chunks, torch.int32)] + [z(n_chunks, torch.int64) for _ in range(1 if coder == "ans" else 2)]
    p = lambda t: C.c_void_p(t.data_ptr())
    fam = () if family == "gaussian" else (B.FAMILIES[family],)
    kind = "gaussian" if family == "gaussian" else "family"
    L = N.lib()
    name = f"cst_{coder}_encode_{kind}_ragged_jump"
    N.check(getattr(L, name)(N.CoderConfig(*cfg), *fam, lo, hi, p(flat), p(a), p(b), p(offsets), n, None, p(words), None, stride, p(n_words),
                             every, p(chunk_off), *(p(t) for t in table), p(status), None), name)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_encode_{family}_ragged_kernel<jump>"
    assert status.cpu().tolist() == [0] * n
    w, nw = words.cpu().numpy().view(np.uint32), n_words.cpu().numpy()
    cols = [table[0].cpu().numpy().view(np.uint32)] + [t.cpu().numpy().view(np.uint64) for t in table[1:]]
    k = 0
    for s, (ww, wt) in enumerate(want):
        assert nw[s] == len(ww) and w[s * stride: s * stride + nw[s]].tolist() == ww.tolist(), s
        assert (w[s * stride + nw[s]: (s + 1) * stride] == 0x5A5A5A5A).all(), s
        assert [tuple(int(c[k + j]) for c in cols) for j in range(chunks[s])] == wt, s
        k += chunks[s]
    out = z(flat.numel(), torch.int32)
    scratch = torch.empty(L.cst_persymbol_ragged_jump_scratch_bytes(n_chunks), dtype=torch.uint8, device="cuda")
    name = f"cst_{coder}_decode_{kind}_ragged_jump"
    for capacity in (words.numel(), 0):
        out.zero_()
        status.fill_(-1)
        N.check(getattr(L, name)(N.CoderConfig(*cfg), *fam, lo, hi, p(words), None, stride, capacity, p(n_words), p(a), p(b), p(out), p(offsets), n,
                                 every, p(chunk_off), n_chunks, *(p(t) for t in table), p(scratch), p(status), None), name)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_decode_{family}_ragged_kernel<jump>"
        assert status.cpu().tolist() == [0] * n and torch.equal(out, flat)


def test_auto(B):
    """"auto" notes a table every RAGGED_JUMP_EVERY symbols for streams that average more than that, none for short streams; 0 is the
    plain kernel"""
    lo, hi = F.support(24)
    assert B.RAGGED_JUMP_EVERY == 256
    for form in (("ans", "gaussian"), ("range", "laplace")):
        encode, decode, enc_name, dec_name = calls(B, form)
        for lengths, noted in (([300, 200, 400, 257], True), ([100] * 12, False)):
            syms, locs, scales = F.workload(form[1], lengths, lo, hi, 12, thin_every=0)
            flat, offsets, a, b = F.flatten(B, syms, locs, scales)
            enc = encode(flat, offsets, lo, hi, a, b, jump_every="auto")
            torch.cuda.synchronize()
            assert B.last_kernel() == enc_name + ("<jump>" if noted else "")
            assert (enc.jump is not None) == noted and (not noted or enc.jump.interval == 256)
            dec, status = decode(enc, offsets, lo, hi, a, b)
            torch.cuda.synchronize()
            assert B.last_kernel() == dec_name + ("<jump>" if noted else "")
            assert (status.cpu().numpy() == 0).all() and torch.equal(dec, flat)
            enc = encode(flat, offsets, lo, hi, a, b, jump_every=0)
            torch.cuda.synchronize()
            assert B.last_kernel() == enc_name and enc.jump is None
            assert encode(flat, offsets, lo, hi, a, b).jump is None
