"""CPU-only: the per-symbol Categorical entry points (cst_{ans,range}_{encode,decode}_categorical_batch, cst_categorical_fast_cdf_rows
and the host form cst_categorical_fast_cdf_host) exist at every layer and judge their arguments before they touch the device; and
the row walk of csrc/cst_categorical.hpp -- the one implementation the kernels share with the host function -- equals the oracle's
restatement of fast_quantized_cdf word for word, through the host function, which needs no GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
CODER_CALLS = ["cst_ans_encode_categorical_batch", "cst_ans_decode_categorical_batch", "cst_range_encode_categorical_batch",
               "cst_range_decode_categorical_batch"]
ENTRY_POINTS = CODER_CALLS + ["cst_categorical_fast_cdf_rows", "cst_categorical_fast_cdf_host"]
KS = [2, 3, 5, 63, 64, 65, 257, 1031]


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_header_library_ctypes_and_rust_know_the_entry_points(lib):
    from constriction_amd import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    wrappers = re.sub(r"//[^\n]*", "", (ROOT / "bindings" / "rust" / "src" / "lib.rs").read_text())
    for name in ENTRY_POINTS:
        assert re.search(r"cst_status\s+%s\s*\(" % name, text), f"{name}: not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
        assert re.search(r"pub fn %s\s*\(" % name, ffi), f"{name}: not in the Rust extern block"
        assert f"ffi::{name}(" in wrappers, f"{name}: no Rust wrapper"
    for name in CODER_CALLS:
        assert re.search(r"%s\s*\(\s*cst_coder_config\s+cfg\s*,[^;]*\bprob_bytes\b[^;]*\bn_symbols\b" % name, text), name
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def _call(lib, name, null=(), prob_bytes=4, n_symbols=5, cfg=(32, 64, 24), flags=None):
    """one call with n_streams = 1, n_per_stream = 4 and HOST buffers behind every pointer: a call that passed its argument checks
    would go on to the device, so only calls that must fail them are made"""
    from constriction_amd import _native as N
    buf = {k: np.zeros(64, dtype=np.float64) for k in ("symbols", "probs", "words", "n_words", "state", "status", "n_words_out")}
    p = {k: (None if k in null else ctypes.c_void_p(v.ctypes.data)) for k, v in buf.items()}
    c = N.CoderConfig(*cfg)
    flags = N.FLAG_NONE if flags is None else flags
    if "encode" in name:
        return getattr(lib, name)(c, p["symbols"], p["probs"], prob_bytes, n_symbols, 1, 4, N.LAYOUT_STREAM_MAJOR, p["words"], 16, p["n_words"],
                                  p["state"], p["status"], flags, None)
    if name == "cst_ans_decode_categorical_batch":
        return lib.cst_ans_decode_categorical_batch(c, p["words"], None, 16, 16, p["n_words"], p["probs"], prob_bytes, n_symbols, p["symbols"], 1, 4,
                                                    N.LAYOUT_STREAM_MAJOR, p["state"], p["n_words_out"], p["status"], flags, None)
    return lib.cst_range_decode_categorical_batch(c, p["words"], None, 16, 16, p["n_words"], p["probs"], prob_bytes, n_symbols, p["symbols"], 1, 4,
                                                  N.LAYOUT_STREAM_MAJOR, p["state"], p["status"], flags, None)


@pytest.mark.parametrize("name", CODER_CALLS)
def test_invalid_arguments_are_refused_before_the_device(lib, name):
    from constriction_amd import _native as N
    bad, model = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    for nothing in ("symbols", "probs", "words", "n_words", "status"):
        assert _call(lib, name, null=(nothing,)) == bad, nothing
    for prob_bytes in (0, 2, 5, 16, -4):
        assert _call(lib, name, prob_bytes=prob_bytes) == bad, prob_bytes
    assert _call(lib, name, prob_bytes=8, null=("status",)) == bad
    assert _call(lib, name, null=("state",), flags=N.FLAG_RAW_STATE) == bad
    for k in (-1, 0, 1, (1 << 24) - 1, 1 << 24):
        assert _call(lib, name, n_symbols=k) == model, k
    for k in (4095, 4096, 70000):
        assert _call(lib, name, n_symbols=k, cfg=(32, 64, 12)) == model, k
        assert _call(lib, name, n_symbols=k, cfg=(16, 32, 12), prob_bytes=8) == model, k
    # the pointer and prob_bytes checks come first
    assert _call(lib, name, n_symbols=1, null=("probs",)) == bad
    assert _call(lib, name, n_symbols=1, prob_bytes=3) == bad


def test_tabulation_calls_check_their_arguments(lib):
    from constriction_amd import _native as N
    probs, rows = np.full(8, 0.125, np.float32), np.zeros(9, np.uint32)
    pp, pr = ctypes.c_void_p(probs.ctypes.data), ctypes.c_void_p(rows.ctypes.data)
    bad, model = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    assert lib.cst_categorical_fast_cdf_rows(24, None, 4, 1, 8, pr, None, None) == bad
    assert lib.cst_categorical_fast_cdf_rows(24, pp, 4, 1, 8, None, None, None) == bad
    assert lib.cst_categorical_fast_cdf_rows(24, pp, 3, 1, 8, pr, None, None) == bad
    assert lib.cst_categorical_fast_cdf_rows(24, pp, 4, 1, 1, pr, None, None) == model
    assert lib.cst_categorical_fast_cdf_rows(3, pp, 4, 1, 7, pr, None, None) == model
    assert lib.cst_categorical_fast_cdf_host(24, None, 4, 1, 8, pr, None) == bad
    assert lib.cst_categorical_fast_cdf_host(24, pp, 4, 1, 8, None, None) == bad
    assert lib.cst_categorical_fast_cdf_host(24, pp, 2, 1, 8, pr, None) == bad
    assert lib.cst_categorical_fast_cdf_host(24, pp, 4, 1, 1, pr, None) == model
    assert lib.cst_categorical_fast_cdf_host(3, pp, 4, 1, 7, pr, None) == model
    assert lib.cst_categorical_fast_cdf_host(24, pp, 4, 1, 8, pr, None) == N.CST_OK      # (bad flags are optional)
    assert rows.tolist() == [i * ((1 << 21) - 1) + i for i in range(8)] + [1 << 24]


def test_batched_exposes_the_five_names():
    pytest.importorskip("torch")
    from constriction_amd import batched
    for name in ("categorical_cdf_rows", "ans_encode_categorical", "range_encode_categorical", "ans_decode_categorical", "range_decode_categorical"):
        assert callable(getattr(batched, name)), name


# ---------------------------------------------------------------------------------------------------------------------
# the row walk against the oracle
# ---------------------------------------------------------------------------------------------------------------------

def host_rows(lib, probs, P):
    probs = np.ascontiguousarray(probs)
    n, k = probs.shape
    rows, bad = np.zeros((n, k + 1), np.uint32), np.full(n, -1, np.int32)
    rc = lib.cst_categorical_fast_cdf_host(P, ctypes.c_void_p(probs.ctypes.data), probs.itemsize, n, k, ctypes.c_void_p(rows.ctypes.data),
                                           ctypes.c_void_p(bad.ctypes.data))
    assert rc == 0
    return rows, bad


def row_sets(dtype, k, seed):
    """name -> rows [16, k]: Dirichlet(0.3); the same with exact zeros inside; a first entry of 1e-42 (an f32 denormal); unnormalised
    exp(logits) (sums far from 1, entries over forty orders of magnitude)"""
    rng = np.random.default_rng(seed)
    d = rng.dirichlet(np.full(k, 0.3), size=16)
    zeros = d.copy()
    if k > 2:
        zeros[:, 1:-1][rng.random((16, k - 2)) < 0.4] = 0.0
    else:
        zeros[::2, 0] = 0.0
    tiny = d.copy()
    tiny[:, 0] = 1e-42
    logits = np.exp(rng.normal(0.0, 12.0, (16, k)))
    return {name: np.ascontiguousarray(m.astype(dtype)) for name, m in (("dirichlet", d), ("zeros", zeros), ("tiny_first", tiny), ("exp_logits", logits))}


@pytest.mark.parametrize("P", [12, 24])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_walk_equals_the_oracle_word_for_word(lib, O, dtype, k, P):
    for name, probs in row_sets(dtype, k, 1000 * P + k).items():
        if name == "tiny_first" and dtype == np.float32:
            assert 0.0 < probs[0, 0] < np.finfo(np.float32).tiny        # (it is a denormal, and it is not flushed on the way here)
        rows, bad = host_rows(lib, probs, P)
        assert (bad == 0).all(), name
        for r in range(len(probs)):
            want = O.categorical_fast_cdf(probs[r], P)
            assert rows[r].tolist() == want.tolist(), (name, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bad_models_are_reported(lib, dtype):
    big = np.finfo(dtype).max
    probs = np.full((6, 7), 0.125, dtype)
    probs[1, 3] = np.nan
    probs[2, 6] = -0.25
    probs[3, :] = 0.0
    probs[4, :2] = big                  # the sum overflows
    probs[5, 0] = -0.0                  # (a negative zero is a zero)
    rows, bad = host_rows(lib, probs, 24)
    assert bad.tolist() == [0, 1, 1, 1, 1, 0]
    for r in (1, 2, 3, 4):
        assert rows[r].tolist() == [0xFFFFFFFF] + [1 << 24] * 7        # no quantile lies in a bad model's row
    tiny = np.full((1, 4), np.finfo(dtype).tiny / 8, dtype)             # a subnormal sum is not normal
    assert host_rows(lib, tiny, 24)[1].tolist() == [1]


def test_trailing_zero_in_f32_gives_an_empty_last_interval_as_in_the_reference(lib, O):
    """an f32 row whose last entry is exactly 0 can have cdf[K - 1] == 2^P: reproduced, not repaired"""
    rng = np.random.default_rng(7)
    P, hits = 24, 0
    for k in (5, 64, 257):
        probs = rng.dirichlet(np.full(k, 0.3), size=400).astype(np.float32)
        probs[:, -1] = 0.0                  # (the rest no longer sums to 1: norm * (free_weight / norm) then rounds up often enough)
        rows, bad = host_rows(lib, probs, P)
        assert (bad == 0).all()
        for r in range(400):
            want = O.categorical_fast_cdf(probs[r], P)
            assert rows[r].tolist() == want.tolist()
            hits += int(want[k - 1] == 1 << P)
            assert (rows[r, k - 1] == 1 << P) == (want[k - 1] == 1 << P)
    assert hits > 100          # (the oracle does have it, often)


def reassociated_table(probs, P):
    """the table from prefix sums taken in another order: pairwise within blocks of two, then across (what a parallel scan does)"""
    dt = probs.dtype.type
    k = len(probs)
    pairs = [dt(probs[i] + probs[i + 1]) if i + 1 < k else probs[i] for i in range(0, k, 2)]
    block = np.concatenate([[dt(0)], np.cumsum(np.array(pairs, dtype=probs.dtype), dtype=probs.dtype)])
    cum = np.empty(k + 1, dtype=probs.dtype)
    for i in range(k + 1):
        cum[i] = block[i // 2] if i % 2 == 0 else dt(block[i // 2] + probs[i - 1])
    scale = dt(dt((1 << P) - k) / cum[k])
    return (np.trunc((cum[:k] * scale).astype(probs.dtype).astype(np.float64)).astype(np.uint64) + np.arange(k, dtype=np.uint64)).astype(np.uint32)


def test_the_inputs_tell_a_reordered_sum_from_the_sequential_one(O):
    """For f32 rows with K >= 63 a table built from reassociated prefix sums differs from the oracle's in EVERY row: so the
    word-for-word tests above cannot be passed by a scan or a tree sum."""
    for k in (63, 64, 65, 257, 1031):
        probs = row_sets(np.float32, k, 24000 + k)["dirichlet"]
        for r in range(len(probs)):
            want = O.categorical_fast_cdf(probs[r], 24)
            assert reassociated_table(probs[r], 24).tolist() != want[:k].tolist(), (k, r)


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in coders' classification of a call with parameters (no device needed)
# ---------------------------------------------------------------------------------------------------------------------

def test_drop_in_classifies_fast_categorical_calls_as_matrices():
    pytest.importorskip("torch")
    from constriction_amd.stream import _single as S, model as M
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        mat = rng.dirichlet(np.ones(6), size=9).astype(dtype)
        for model in (M.Categorical(perfect=False), M.Categorical(lazy=True)):
            kind = S.model_args(model, (mat,), families=True)
            assert kind[0] == "categorical" and kind[1].dtype == dtype and np.array_equal(kind[1], mat)      # (f32 is not widened)
            assert S.model_args(model, (mat,))[0] == "rows"                  # the chain coder keeps the tabulated rows
        assert S.model_args(M.Categorical(perfect=True), (mat,), families=True)[0] == "rows"      # a sequential host search
    ps = rng.uniform(0.0, 1.0, 11)
    kind = S.model_args(M.Bernoulli(perfect=False), (ps,), families=True)
    assert kind[0] == "categorical" and kind[1].dtype == np.float64 and np.array_equal(kind[1], np.stack([1.0 - ps, ps], axis=1))
    assert S.model_args(M.Bernoulli(perfect=True), (ps,), families=True)[0] == "rows"
    # the rows the other coders get are the rows the matrix quantises to
    rows = S.model_args(M.Categorical(perfect=False), (mat,))[1]
    assert rows.shape == (9, 7) and (rows[:, 0] == 0).all() and (rows[:, -1] == 1 << 24).all()


def test_drop_in_keeps_the_reference_errors_for_invalid_matrices():
    pytest.importorskip("torch")
    from constriction_amd.stream import _single as S, model as M
    good = np.random.default_rng(6).dirichlet(np.ones(5), size=8)
    fast = M.Categorical(perfect=False)
    for dtype in (np.float32, np.float64):
        for spoil in (np.nan, -0.5, np.inf, np.finfo(dtype).max):
            bad = good.astype(dtype)
            bad[3, 2] = spoil
            bad[3, 3] = spoil
            with pytest.raises(ValueError, match="not normalizable"):
                S.model_args(fast, (bad,), families=True)
        zero = good.astype(dtype)
        zero[5, :] = 0.0
        with pytest.raises(ValueError, match="not normalizable"):
            S.model_args(M.Categorical(lazy=True), (zero,), families=True)
        with pytest.raises(ValueError, match="not normalizable"):
            S.model_args(fast, (good.astype(dtype)[:, :1],), families=True)          # K < 2
    with pytest.raises(TypeError):
        S.model_args(fast, (good.astype(np.float16),), families=True)
    with pytest.raises(ValueError):
        S.model_args(fast, (good[0],), families=True)                               # rank 1
    for p in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="`p` must be"):
            S.model_args(M.Bernoulli(perfect=False), (np.array([0.5, p]),), families=True)
