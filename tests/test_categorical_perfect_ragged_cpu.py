"""CPU-only: the ragged per-symbol Categorical(perfect=True) calls (cst_{ans,range}_{encode,decode}_categorical_perfect_ragged and their
*_jump forms) exist at every layer -- exported, declared, bound in _native.SIGNATURES, present in the Rust ffi, wrapped in
constriction_amd.batched -- and judge their arguments before they touch the device, so the refusals run here, without a GPU (the
harness of tests/test_categorical_ragged_cpu.py: host buffers behind every pointer, and only calls that must be refused, or that hold
no stream, are made).  Last: the condition the GPU file rests on -- the library's host quantiser gives every row of that file's batches
code 0 and the words of oracle.categorical_perfect_cdf."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import categorical_perfect_ragged_rows as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
FFI = ROOT / "bindings" / "rust" / "src" / "ffi.rs"
PLAIN = [f"cst_{coder}_{way}_categorical_perfect_ragged" for coder in ("ans", "range") for way in ("encode", "decode")]
JUMP = [name + "_jump" for name in PLAIN]
CALLS = PLAIN + JUMP
MAX_K = 1024


def table_args(name):
    return ["d_jump_state"] if "_ans_" in name else ["d_jump_lower", "d_jump_range"]


def expected_args(name):
    """the lists of cst_*_categorical_ragged[_jump]; the two plain decoders take max_len directly after n_total"""
    jump = name.endswith("_jump")
    if "_encode_" in name:
        args = ["cfg", "d_symbols", "d_probs", "prob_bytes", "n_symbols", "n_total", "d_sym_offsets", "n_streams", "d_order", "d_words",
                "d_word_offsets", "stride_words", "d_n_words"]
        if jump:
            args += ["jump_interval", "d_chunk_offsets", "d_jump_pos"] + table_args(name)
        return args + ["d_status", "stream"]
    args = ["cfg", "d_words", "d_word_offsets", "stride_words", "words_capacity", "d_n_words", "d_probs", "prob_bytes", "n_symbols", "n_total"]
    tail = ["d_symbols", "d_sym_offsets", "n_streams"]
    if jump:
        return args + tail + ["jump_interval", "d_chunk_offsets", "n_chunks_total", "d_jump_pos"] + table_args(name) + ["d_scratch", "d_status", "stream"]
    return args + ["max_len"] + tail + ["d_order", "d_status", "stream"]


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def _declared(text, name):
    m = re.search(r"cst_status\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name}: not declared"
    return [re.search(r"(\w+)\s*$", arg.strip()).group(1) for arg in m.group(1).split(",")]


def test_the_eight_entry_points_exist_at_every_layer(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = FFI.read_text()
    for name in CALLS:
        assert _declared(text, name) == expected_args(name), name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _native.SIGNATURES[name]
        assert res == ctypes.c_int32 and len(args) == len(expected_args(name)), name
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} is not in the Rust ffi"
        # argument for argument the fast ragged call's, but for max_len
        fast = _declared(text, name.replace("_perfect", ""))
        assert [a for a in expected_args(name) if a != "max_len"] == fast, name
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5
    assert re.search(r"#define\s+CST_CATEGORICAL_PERFECT_MAX_K\s+%d\b" % MAX_K, HEADER.read_text()) and _native.CATEGORICAL_PERFECT_MAX_K == MAX_K
    assert "CST_PERFECT_RAGGED_BUDGET" in HEADER.read_text()


POINTERS = ("symbols", "probs", "sym_offsets", "order", "words", "word_offsets", "n_words", "status", "chunk_offsets", "jump_pos", "jump_a", "jump_b",
            "scratch")


def _call(lib, name, cfg=(32, 64, 24), null=(), prob_bytes=4, k=5, n_total=8, max_len=8, stride=0, n_streams=1, interval=64, n_chunks=8):
    from constriction_amd import _native as N
    buf = {key: np.zeros(64, dtype=np.float64) for key in POINTERS}
    p = {key: (None if key in null else ctypes.c_void_p(v.ctypes.data)) for key, v in buf.items()}
    c = N.CoderConfig(*cfg)
    table = (p["jump_pos"], p["jump_a"]) if "_ans_" in name else (p["jump_pos"], p["jump_a"], p["jump_b"])
    jump = name.endswith("_jump")
    if "_encode_" in name:
        tail = (interval, p["chunk_offsets"], *table) if jump else ()
        return getattr(lib, name)(c, p["symbols"], p["probs"], prob_bytes, k, n_total, p["sym_offsets"], n_streams, p["order"], p["words"],
                                  p["word_offsets"], stride, p["n_words"], *tail, p["status"], None)
    head = (c, p["words"], p["word_offsets"], stride, 64, p["n_words"], p["probs"], prob_bytes, k, n_total)
    if jump:
        return getattr(lib, name)(*head, p["symbols"], p["sym_offsets"], n_streams, interval, p["chunk_offsets"], n_chunks, *table, p["scratch"],
                                  p["status"], None)
    return getattr(lib, name)(*head, max_len, p["symbols"], p["sym_offsets"], n_streams, p["order"], p["status"], None)


def required(name):
    r = ["symbols", "probs", "sym_offsets", "words", "n_words", "status"]
    if name.endswith("_jump"):
        r += ["chunk_offsets", "jump_pos", "jump_a"] + (["jump_b"] if "_range_" in name else []) + (["scratch"] if "_decode_" in name else [])
    return r


@pytest.mark.parametrize("name", CALLS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad, model = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    for n_streams in (0, 1):
        for cfg in ((32, 64, 25), (32, 64, 0), (16, 32, 17), (32, 32, 12), (16, 64, 12), (64, 64, 24)):
            assert _call(lib, name, cfg=cfg, n_streams=n_streams) == bad, cfg
        for pointer in required(name):
            assert _call(lib, name, null=(pointer,), n_streams=n_streams) == bad, pointer
        assert _call(lib, name, null=("word_offsets",), stride=0, n_streams=n_streams) == bad
        for prob_bytes in (0, 2, 3, 5, 16, -4):
            assert _call(lib, name, prob_bytes=prob_bytes, n_streams=n_streams) == bad, prob_bytes
        # the perfect limits: K < 2, more entries than the quantiser has slots, more than there are units of weight (K > 2^P)
        for cfg, k in (((32, 64, 24), 1), ((32, 64, 24), 0), ((32, 64, 24), -3), ((32, 64, 24), MAX_K + 1), ((32, 64, 24), (1 << 24) - 2),
                       ((16, 32, 12), MAX_K + 1), ((32, 64, 3), 9), ((16, 32, 1), 3), ((32, 64, 9), 513)):
            assert _call(lib, name, cfg=cfg, k=k, n_streams=n_streams) == model, (cfg, k)
        # ... an invalid argument is reported before a model that cannot be built
        assert _call(lib, name, k=1, prob_bytes=3, n_streams=n_streams) == bad
        assert _call(lib, name, k=1, null=("probs",), n_streams=n_streams) == bad
        if name.endswith("_jump"):
            for interval in (0, 8, 24, 100, 1 << 31, (1 << 31) + 16):
                assert _call(lib, name, interval=interval, n_streams=n_streams) == bad, (interval, n_streams)
            if "_decode_" in name:
                assert _call(lib, name, n_chunks=1 << 32, n_streams=n_streams) == bad
    for n_streams in (1 << 31, 1 << 32, 1 << 62):                       # more streams than a launch has blocks
        assert _call(lib, name, n_streams=n_streams) == bad, n_streams
    if "_encode_" in name:
        for n_total in (1 << 31, 1 << 40):                               # more rows than the quantiser has workgroups
            assert _call(lib, name, n_total=n_total) == bad, n_total
            assert _call(lib, name, n_total=n_total, n_streams=0) == bad, n_total
    assert _call(lib, name, null=POINTERS) == bad


@pytest.mark.parametrize("name", CALLS)
def test_no_streams_is_ok_and_launches_nothing(lib, name):
    from constriction_amd import _native as N
    # K at its limits: 2, the slots, 2^P where that is smaller
    for cfg, k in (((32, 64, 24), 2), ((32, 64, 24), MAX_K), ((32, 64, 12), 257), ((16, 32, 12), MAX_K), ((16, 32, 16), 65), ((32, 64, 3), 8),
                   ((16, 32, 1), 2)):
        for prob_bytes in (4, 8):
            assert _call(lib, name, cfg=cfg, k=k, prob_bytes=prob_bytes, n_streams=0) == N.CST_OK, (cfg, k)
    assert _call(lib, name, n_streams=0, n_total=0, max_len=0, interval=(1 << 31) - 16, n_chunks=(1 << 32) - 1) == N.CST_OK
    assert _call(lib, name, n_streams=0, n_total=(1 << 31) - 1, max_len=1 << 40) == N.CST_OK
    assert _call(lib, name, n_streams=0, null=("order", "word_offsets"), stride=7) == N.CST_OK


NAMES = ["ans_encode_categorical_perfect_ragged", "ans_decode_categorical_perfect_ragged", "range_encode_categorical_perfect_ragged",
         "range_decode_categorical_perfect_ragged"]


def test_batched_exposes_the_four_names():
    pytest.importorskip("torch")
    import inspect
    from constriction_amd import batched
    for fn in NAMES:
        f, fast = getattr(batched, fn), getattr(batched, fn.replace("_perfect", ""))
        assert f is not fast
        assert str(inspect.signature(f)) == str(inspect.signature(fast)), fn
        params = list(inspect.signature(f).parameters)
        if "_encode_" in fn:
            assert params == ["symbols", "sym_offsets", "probabilities", "config", "order", "jump_every"], fn
            assert f.__kwdefaults__ == {"jump_every": 0} and inspect.signature(f).parameters["config"].default == (32, 64, 24)
        else:
            assert params == ["encoded", "sym_offsets", "probabilities", "out", "order"], fn
        assert inspect.signature(f).parameters["order"].default == "auto"


@pytest.mark.parametrize("jump_every", [-16, 8, 24, "often", 1 << 31])
@pytest.mark.parametrize("fn", [n for n in NAMES if "_encode_" in n])
def test_jump_every_is_judged_first(fn, jump_every):
    """CPU tensors: anything else the function did with them would fail differently"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    sym, off, probs = torch.zeros(8, dtype=torch.int32), torch.tensor([0, 3, 8]), torch.ones(8, 5)
    with pytest.raises(ValueError, match="jump_every"):
        getattr(batched, fn)(sym, off, probs, jump_every=jump_every)


def test_decoders_refuse_the_other_coders_batch_and_table():
    """judged before any tensor is looked at (CPU tensors: anything else would fail differently)"""
    torch = pytest.importorskip("torch")
    from constriction_amd import batched
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    probs, off = torch.ones(8, 5), torch.tensor([0, 3, 8])
    of_range = batched.RangeRaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64), z(4, torch.int64))
    of_ans = batched.RaggedJump(16, z(3, torch.int64), z(4, torch.int32), z(4, torch.int64))
    batch = lambda coder, table: batched.RaggedBatch(z(8, torch.int32), z(3, torch.int64), z(2, torch.int32), z(2, torch.int32), (32, 64, 24), None,
                                                     table, coder)
    with pytest.raises(ValueError, match="coder"):
        batched.ans_decode_categorical_perfect_ragged(batch("range", None), off, probs)
    with pytest.raises(ValueError, match="coder"):
        batched.range_decode_categorical_perfect_ragged(batch("ans", None), off, probs)
    with pytest.raises(ValueError, match="another coder"):
        batched.ans_decode_categorical_perfect_ragged(batch("ans", of_range), off, probs)
    with pytest.raises(ValueError, match="another coder"):
        batched.range_decode_categorical_perfect_ragged(batch("range", of_ans), off, probs)


def _host_rows(lib, probs, P):
    probs = np.ascontiguousarray(probs)
    n, k = probs.shape
    rows, bad = np.zeros((n, k + 1), np.uint32), np.full(n, -1, np.int32)
    rc = lib.cst_categorical_perfect_cdf_host(P, ctypes.c_void_p(probs.ctypes.data), probs.itemsize, n, k, ctypes.c_void_p(rows.ctypes.data),
                                              ctypes.c_void_p(bad.ctypes.data), None)
    assert rc == 0
    return rows, bad


# every batch of the GPU file: (name, lengths, K, dtype, P)
GPU_BATCHES = ([("parity", R.PARITY_LENGTHS, k, dt, cfg[2]) for k, dt in R.MODELS for cfg in R.CONFIGS]
               + [("local", R.LOCAL_LENGTHS, 1024, "f32", 24), ("local", R.LOCAL_LENGTHS, 65, "f32", 24), ("bounds", [40, 30, 50], 5, "f64", 24)])


@pytest.mark.parametrize("case", GPU_BATCHES, ids=lambda c: "%s-K%d-%s-P%d" % (c[0], c[2], c[3], c[4]))
def test_the_gpu_files_rows_quantise(lib, case):
    """the condition of tests/test_gpu_categorical_perfect_ragged.py: the host form of the device quantiser gives every row code 0 and the
    words of the oracle"""
    from oracle import oracle as O
    name, lengths, k, dtype, P = case
    assert sum(R.PARITY_LENGTHS) == 2955 and len(R.PARITY_LENGTHS) == 70 and sum(R.LOCAL_LENGTHS) == 1190 and len(R.LOCAL_LENGTHS) == 9
    _, (sym, probs, off, models) = R.batch(O, name, lengths, k, dtype, P)
    rows, bad = _host_rows(lib, probs, P)
    assert (bad == 0).all(), np.flatnonzero(bad)[:5]
    flat = [m for stream in models for m in stream]
    assert len(flat) == len(rows) == sum(lengths)
    for i, m in enumerate(flat):
        assert rows[i].tolist() == m.cdf.tolist(), i
    assert sym.min() >= 0 and sym.max() < k and int(off[-1]) == len(sym)
