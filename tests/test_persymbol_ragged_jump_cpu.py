"""CPU-only: jump points for ragged per-symbol batches (cst_{ans,range}_{encode,decode}_{gaussian,family}_ragged_jump and
cst_persymbol_ragged_jump_scratch_bytes) exist at every layer, the calls judge their arguments before they touch the device -- so the
argument checks run here, without a GPU -- and the oracle recipe that the GPU tests take their expected jump tables from is itself
checked: coding a stream chunk by chunk gives the words of coding it in one go, and seek + decode returns the chunk."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
SCRATCH = "cst_persymbol_ragged_jump_scratch_bytes"
CALLS = [f"cst_{coder}_{way}_{fam}_ragged_jump" for fam in ("gaussian", "family") for coder in ("ans", "range") for way in ("encode", "decode")]


def table_args(name):
    return ["d_jump_state"] if "_ans_" in name else ["d_jump_lower", "d_jump_range"]


def expected_args(name):
    """the arguments of the plain call (the decoder's without d_order), then the interval and the table, in the order of
    cst_{ans,range}_{encode,decode}_ragged_jump"""
    fam = ["family"] if "_family_" in name else []
    a, b = ("d_a", "d_b") if fam else ("d_means", "d_stds")
    if "_encode_" in name:
        return (["cfg"] + fam + ["min_symbol", "max_symbol", "d_symbols", a, b, "d_sym_offsets", "n_streams", "d_order", "d_words", "d_word_offsets",
                                 "stride_words", "d_n_words", "jump_interval", "d_chunk_offsets", "d_jump_pos"] + table_args(name)
                + ["d_status", "stream"])
    return (["cfg"] + fam + ["min_symbol", "max_symbol", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", a, b, "d_symbols",
                             "d_sym_offsets", "n_streams", "jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos"] + table_args(name)
            + ["d_scratch", "d_status", "stream"])


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def _declared(text, name):
    m = re.search(r"(?:cst_status|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name}: not declared"
    return [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_nine_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert _declared(text, SCRATCH) == ["n_chunks_total"]
    assert hasattr(lib, SCRATCH) and SCRATCH in _native.SIGNATURES
    for name in CALLS:
        assert _declared(text, name) == expected_args(name), name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(expected_args(name)), name
        # the plain call's arguments lead (the decoder's without d_order)
        plain = _declared(text, name[: -len("_jump")])
        k = expected_args(name).index("jump_interval")
        assert expected_args(name)[:k] == ([x for x in plain if x != "d_order"] if "_decode_" in name else plain)[:k]
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5
    assert "No jump points for any of these" not in HEADER.read_text()
    # per chunk: what the decoder keeps of it is no less than the table entry itself
    assert lib.cst_persymbol_ragged_jump_scratch_bytes(0) > 0
    assert lib.cst_persymbol_ragged_jump_scratch_bytes(1000) >= lib.cst_persymbol_ragged_jump_scratch_bytes(0) + 20 * 1000


POINTERS = ("symbols", "a", "b", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "chunk_offsets", "jump_pos", "jump_a",
            "jump_b", "scratch")


def _call(lib, name, cfg=(32, 64, 24), family=1, lo=-100, hi=100, null=(), stride=0, n_streams=1, interval=64, n_chunks=8):
    """one call with HOST buffers behind every pointer (non-NULL dummies that a refused call never touches): a call that passed its
    argument checks with n_streams > 0 would go on to the device, so only calls that must fail them -- or hold no stream -- are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in POINTERS}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    c = N.CoderConfig(*cfg)
    fam = (family,) if "_family_" in name else ()
    table = (p["jump_pos"], p["jump_a"]) if "_ans_" in name else (p["jump_pos"], p["jump_a"], p["jump_b"])
    if "_encode_" in name:
        return getattr(lib, name)(c, *fam, lo, hi, p["symbols"], p["a"], p["b"], p["sym_offsets"], n_streams, p["order"], p["words"],
                                  p["word_offsets"], stride, p["n_words"], interval, p["chunk_offsets"], *table, p["status"], None)
    return getattr(lib, name)(c, *fam, lo, hi, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["a"], p["b"], p["symbols"],
                              p["sym_offsets"], n_streams, interval, p["chunk_offsets"], n_chunks, *table, p["scratch"], p["status"], None)


def required(name):
    """what may not be NULL: the plain call's pointers, d_chunk_offsets, the table arrays and the decoder's scratch"""
    r = ["symbols", "a", "b", "sym_offsets", "words", "n_words", "status", "chunk_offsets", "jump_pos", "jump_a"]
    if "_range_" in name:
        r.append("jump_b")
    if "_decode_" in name:
        r.append("scratch")
    return r


@pytest.mark.parametrize("name", CALLS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad = N.CST_ERR_INVALID_ARGUMENT
    for n_streams in (0, 1):
        # what the plain call refuses
        for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
            assert _call(lib, name, cfg=cfg, n_streams=n_streams) == bad, cfg
        assert _call(lib, name, lo=5, hi=5, n_streams=n_streams) == bad and _call(lib, name, lo=5, hi=4, n_streams=n_streams) == bad
        assert _call(lib, name, null=("word_offsets",), stride=0, n_streams=n_streams) == bad
        # ... and what the jump points add
        for interval in (0, 8, 24, 100, 1 << 31, (1 << 31) + 16):
            assert _call(lib, name, interval=interval, n_streams=n_streams) == bad, (interval, n_streams)
        for pointer in required(name):
            assert _call(lib, name, null=(pointer,), n_streams=n_streams) == bad, pointer
        if "_decode_" in name:
            assert _call(lib, name, n_chunks=1 << 32, n_streams=n_streams) == bad
        if "_family_" in name:
            for family in (0, 3, 99, -1):
                assert _call(lib, name, family=family, n_streams=n_streams) == bad, family
    if "_encode_" in name:
        assert _call(lib, name, n_streams=1 << 32) == bad        # (an order with more streams than its entries can name)
    assert _call(lib, name, null=POINTERS) == bad


@pytest.mark.parametrize("name", CALLS)
def test_no_streams_is_ok_and_launches_nothing(lib, name):
    from constriction_amd import _native as N
    for cfg in ((32, 64, 24), (32, 64, 12), (16, 32, 12)):
        for family in (1, 2):
            assert _call(lib, name, cfg=cfg, family=family, n_streams=0) == N.CST_OK
    assert _call(lib, name, n_streams=0, interval=(1 << 31) - 16, n_chunks=(1 << 32) - 1) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("order", "word_offsets"), stride=7) == N.CST_OK


ENCODERS = ["ans_encode_gaussian_ragged", "range_encode_gaussian_ragged", "ans_encode_laplace_ragged", "range_encode_laplace_ragged",
            "ans_encode_cauchy_ragged", "range_encode_cauchy_ragged", "ans_encode_family_ragged", "range_encode_family_ragged"]


@pytest.mark.parametrize("fn", ENCODERS)
def test_the_eight_encoders_take_jump_every(fn):
    """a keyword-only option with the default 0 -- the plain call -- on all eight (the named Laplace / Cauchy forms hand their
    keywords on to the family call)"""
    pytest.importorskip("torch")
    from constriction_amd import batched
    f = getattr(batched, fn.replace("laplace", "family").replace("cauchy", "family"))
    assert f.__kwdefaults__ == {"jump_every": 0}
    assert callable(getattr(batched, fn))


@pytest.mark.parametrize("jump_every", [-16, 8, 24, "often"])
@pytest.mark.parametrize("fn", ENCODERS)
def test_jump_every_is_judged_first(fn, jump_every):
    """CPU tensors: anything else the function did with them would fail differently"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    sym, off, par = torch.zeros(8, dtype=torch.int32), torch.tensor([0, 3, 8]), torch.ones(8, dtype=torch.float64)
    fam = ("laplace",) if "family" in fn else ()
    with pytest.raises(ValueError, match="jump_every"):
        getattr(batched, fn)(*fam, sym, off, -100, 100, par, par, jump_every=jump_every)


def test_a_table_of_the_other_coder_is_refused():
    """judged right after the coder itself, before any tensor is looked at (CPU tensors: anything else would fail differently)"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    par, off = torch.ones(8, dtype=torch.float64), torch.tensor([0, 3, 8])
    of_range = batched.RangeRaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    of_ans = batched.RaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64))
    for coder, table, decode in (("ans", of_range, batched.ans_decode_gaussian_ragged), ("range", of_ans, batched.range_decode_laplace_ragged),
                                 ("range", of_ans, batched.range_decode_gaussian_ragged), ("ans", of_range, batched.ans_decode_cauchy_ragged)):
        enc = batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None, table, coder)
        with pytest.raises(ValueError, match="another coder"):
            decode(enc, off, -100, 100, par, par)


# ---- the oracle recipe of tests/test_gpu_persymbol_ragged_jump.py ----

def _models(O, lo, hi, n, P, rng):
    return [O.GaussianModel(lo, hi, float(m), float(s), P) for m, s in zip(rng.uniform(-30, 30, n), np.exp(rng.uniform(-1, 3, n)))]


@pytest.mark.parametrize("cfg", [(32, 64, 24), (16, 32, 12)], ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("every", [16, 48])
def test_chunkwise_oracle_equals_one_shot(cfg, every):
    """AnsCoder: encode_reverse per chunk, last chunk first, pos() after each; RangeEncoder: pos() before each encode(chunk), first
    chunk first.  The words are those of one call over the whole stream; AnsCoder(words).seek(pos, state) + decode returns the chunk;
    chunk 0 is the final (bulk, state) -- n_words - S / W words where the state fills S / W words -- and (0, 0, all ones of the state width)."""
    from oracle import oracle as O
    from persymbol_jump_oracle import ans_table, range_table
    W, S, P = cfg
    lo, hi = (-100, 100) if P == 24 else (-60, 60)
    rng = np.random.default_rng(every + P)
    for n in (1, 49, 96, 700):
        models = _models(O, lo, hi, n, P, rng)
        sym = rng.integers(lo, hi + 1, n).astype(np.int32)
        one = O.AnsCoder(W=W, S=S)
        one.encode_reverse(sym, models, P)
        words, table = ans_table(O, cfg, sym, models, every)
        assert words.tolist() == one.get_compressed().tolist()
        assert len(table) == -(-n // every)
        assert table[0] == one.pos()
        if one.pos()[1] >> (S - W):           # (a state below 2^(S - W) -- a stream of a symbol or two -- leaves fewer than S / W words)
            assert table[0][0] == len(words) - S // W
        for j, (pos, state) in enumerate(table):
            c = O.AnsCoder(words, W=W, S=S)
            c.seek(pos, state)
            assert c.decode(models[j * every: (j + 1) * every], P=P).tolist() == sym[j * every: (j + 1) * every].tolist()
        rone = O.RangeEncoder(W=W, S=S)
        rone.encode(sym, models, P)
        rwords, rtable = range_table(O, cfg, sym, models, every)
        assert rwords.tolist() == rone.get_compressed().tolist()
        assert len(rtable) == -(-n // every) and rtable[0] == (0, 0, (1 << S) - 1)
        assert all(rtable[j][0] <= rtable[j + 1][0] <= len(rwords) for j in range(len(rtable) - 1))
