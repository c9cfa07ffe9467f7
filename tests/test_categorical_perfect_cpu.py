"""CPU-only: the Categorical(perfect=True) entry points (cst_{ans,range}_{encode,decode}_categorical_perfect_batch,
cst_categorical_perfect_cdf_rows and the host form cst_categorical_perfect_cdf_host) exist at every layer and judge their arguments
before they touch the device; the kernel's formulation of the search (positions and counted ranks instead of a sorted vector,
csrc/cst_categorical_perfect.hip) gives, through the host form, the words of the library's sorted-vector host function and of the
oracle and the move counts of a line-by-line Python restatement; and the rows of the GPU tests stay far below the move cap."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import categorical_perfect_rows as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
CODER_CALLS = ["cst_ans_encode_categorical_perfect_batch", "cst_ans_decode_categorical_perfect_batch",
               "cst_range_encode_categorical_perfect_batch", "cst_range_decode_categorical_perfect_batch"]
ENTRY_POINTS = CODER_CALLS + ["cst_categorical_perfect_cdf_rows", "cst_categorical_perfect_cdf_host"]


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
        # the argument list of the fast call of the same coder and direction
        fast = name.replace("_perfect", "")
        args = {n: re.sub(r"\s+", " ", re.search(r"%s\s*\(([^;]*)\)\s*;" % n, text).group(1)).strip() for n in (name, fast)}
        assert args[name] == args[fast], name
    assert re.search(r"#define\s+CST_CATEGORICAL_PERFECT_MAX_K\s+1024\b", HEADER.read_text()) and _native.CATEGORICAL_PERFECT_MAX_K == 1024
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
    if name.startswith("cst_ans"):
        return getattr(lib, name)(c, p["words"], None, 16, 16, p["n_words"], p["probs"], prob_bytes, n_symbols, p["symbols"], 1, 4,
                                  N.LAYOUT_STREAM_MAJOR, p["state"], p["n_words_out"], p["status"], flags, None)
    return getattr(lib, name)(c, p["words"], None, 16, 16, p["n_words"], p["probs"], prob_bytes, n_symbols, p["symbols"], 1, 4,
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
    for k in (-1, 0, 1, 1025, 4096, 1 << 24):
        assert _call(lib, name, n_symbols=k) == model, k
    for k in (257, 1024):                                               # more symbols than units of weight
        assert _call(lib, name, n_symbols=k, cfg=(32, 64, 8)) == model, k
        assert _call(lib, name, n_symbols=k, cfg=(16, 32, 8), prob_bytes=8) == model, k
    # the pointer and prob_bytes checks come first
    assert _call(lib, name, n_symbols=1, null=("probs",)) == bad
    assert _call(lib, name, n_symbols=1025, prob_bytes=3) == bad


def test_tabulation_calls_check_their_arguments(lib):
    from constriction_amd import _native as N
    probs, rows = np.full(8, 0.125, np.float32), np.zeros(9, np.uint32)
    pp, pr = ctypes.c_void_p(probs.ctypes.data), ctypes.c_void_p(rows.ctypes.data)
    bad, model = N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    dev_call, host_call = lib.cst_categorical_perfect_cdf_rows, lib.cst_categorical_perfect_cdf_host
    for call, tail in ((dev_call, (None, None, None)), (host_call, (None, None))):
        assert call(24, None, 4, 1, 8, pr, *tail) == bad
        assert call(24, pp, 4, 1, 8, None, *tail) == bad
        assert call(24, pp, 3, 1, 8, pr, *tail) == bad
        assert call(0, pp, 4, 1, 8, pr, *tail) == bad
        assert call(32, pp, 4, 1, 8, pr, *tail) == bad
        assert call(24, pp, 4, 1, 1, pr, *tail) == model
        assert call(24, pp, 4, 1, 1025, pr, *tail) == model
        assert call(2, pp, 4, 1, 5, pr, *tail) == model                 # 5 symbols, 4 units of weight
    assert host_call(24, pp, 4, 1, 8, pr, None, None) == N.CST_OK       # (codes and move counts are optional)
    assert rows.tolist() == [i << 21 for i in range(9)]
    assert host_call(3, pp, 4, 1, 8, pr, None, None) == N.CST_OK        # K == 2^P: every symbol gets its one unit
    assert rows.tolist() == list(range(9))


def test_batched_checks_its_arguments_without_a_device():
    torch = pytest.importorskip("torch")
    from constriction_amd import batched as B
    for name in ("categorical_cdf_rows", "ans_encode_categorical", "range_encode_categorical", "ans_decode_categorical", "range_decode_categorical"):
        import inspect
        assert "perfect" in inspect.signature(getattr(B, name)).parameters, name
        assert inspect.signature(getattr(B, name)).parameters["perfect"].default is False, name
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        B.categorical_cdf_rows(torch.zeros((3, 5), dtype=torch.float16), perfect=True)
    with pytest.raises(ValueError, match="at least one axis"):
        B.categorical_cdf_rows(torch.tensor(1.0), perfect=True)
    with pytest.raises(ValueError, match="2 <= K"):
        B.categorical_cdf_rows(torch.ones((3, 1)), perfect=True)
    with pytest.raises(ValueError, match="1024"):
        B.categorical_cdf_rows(torch.ones((3, 1025)), perfect=True)
    with pytest.raises(ValueError, match="2\\*\\*precision"):
        B.categorical_cdf_rows(torch.ones((3, 9)), precision=3, perfect=True)
    with pytest.raises(ValueError, match="return_moves"):
        B.categorical_cdf_rows(torch.ones((3, 9)), return_moves=True)
    with pytest.raises(ValueError, match="device memory"):
        B.categorical_cdf_rows(torch.ones((3, 1024)), perfect=True)     # (a valid shape gets as far as the device check)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's formulation, on the CPU
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_ranked_formulation_equals_the_sorted_vector_and_the_oracle(lib, O, case):
    """the rows the GPU test uses: the same words as cst_categorical_perfect_cdf and oracle.categorical_perfect_cdf, no row near
    the move cap (the maximum below a quarter of it)"""
    k, n, P, _ = case
    probs = R.case_rows(case)
    rows, codes, moves = R.host_perfect(lib, probs, P)
    assert (codes == 0).all()
    for r in range(n):
        rc, want = R.sorted_vector_perfect(lib, probs[r], P)
        assert rc == 0 and rows[r].tolist() == want.tolist(), r
        assert rows[r].tolist() == O.categorical_perfect_cdf(probs[r], P).tolist(), r
    print(f"{R.case_id(case)}: moves max {int(moves.max())} mean {moves.mean():.2f} (cap {R.move_cap(k)})")
    assert int(moves.max()) < R.move_cap(k) // 4


def test_f32_rows_hold_subnormals_and_ties():
    probs = R.make_rows(12, 64, np.float32, 3)
    tail = probs[5]
    assert ((tail > 0) & (tail < np.finfo(np.float32).tiny)).sum() >= 3                 # softmax_tail: subnormal entries
    assert len(set(probs[2].tolist())) == 1 and (probs[3] == 0).sum() == 32 and len(set(probs[4].tolist())) <= 3


@pytest.mark.parametrize("case", [c for c in R.ROW_CASES if c[0] <= 65], ids=R.case_id)
def test_move_counts_equal_the_reference_formulation_line_by_line(lib, case):
    """d_moves / h_moves count what the reference's loop does: a Python restatement of categorical.rs:56-177 with a sorted list of
    slots makes the same number of unit moves and builds the same row"""
    k, n, P, _ = case
    probs = R.case_rows(case)[:24]
    rows, codes, moves = R.host_perfect(lib, probs, P)
    for r in range(len(probs)):
        cdf, n_moves = R.python_perfect(lib, probs[r], P)
        assert cdf.tolist() == rows[r].tolist() and n_moves == int(moves[r]), r
    assert int(moves.max()) > 0 or k == 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bad_rows_are_flagged_where_the_host_function_refuses(lib, dtype):
    big = np.finfo(dtype).max
    probs = R.make_rows(8, 7, dtype, 11)
    probs[1, 3] = np.nan
    probs[2, 6] = -0.25
    probs[3, :] = 0.0
    probs[4, 2] = np.inf
    probs[5, 0] = -0.0                                                   # (a negative zero is a zero)
    if dtype == np.float64:
        probs[6, :2] = big                                               # the f64 sum overflows (an f32 row is widened: no overflow)
    rows, codes, moves = R.host_perfect(lib, probs, 24)
    refused = [int(R.sorted_vector_perfect(lib, probs[r], 24)[0] != 0) for r in range(8)]
    assert codes.tolist() == refused == [0, 1, 1, 1, 1, 0, int(dtype == np.float64), 0]
    for r in range(8):
        if refused[r]:
            assert rows[r].tolist() == [0xFFFFFFFF] + [1 << 24] * 7 and moves[r] == 0
        else:
            assert rows[r].tolist() == R.sorted_vector_perfect(lib, probs[r], 24)[1].tolist()
    tiny = np.full((1, 4), np.finfo(np.float64).tiny / 8, np.float64)    # a subnormal sum is not normal
    assert R.host_perfect(lib, tiny, 24)[1].tolist() == [1]


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in coders' classification of a call with parameters (no device needed)
# ---------------------------------------------------------------------------------------------------------------------

def test_drop_in_classifies_perfect_calls_for_the_device_quantiser():
    pytest.importorskip("torch")
    from constriction_amd.stream import _single as S, model as M
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        mat = rng.dirichlet(np.ones(6), size=9).astype(dtype)
        kind = S.model_args(M.Categorical(perfect=True), (mat,), families=True, device_perfect=True)
        assert kind[0] == "categorical_perfect" and kind[1].dtype == dtype and np.array_equal(kind[1], mat)     # (widened on the device)
        assert S.model_args(M.Categorical(perfect=True), (mat,))[0] == "rows"          # the chain coder keeps the host quantiser
        assert S.model_args(M.Categorical(perfect=True), (mat,), families=True)[0] == "rows"       # ... and so does who does not ask
        assert S.model_args(M.Categorical(perfect=True), (mat,), device_perfect=True)[0] == "rows"
    wide = rng.random((2, 1025))
    assert S.model_args(M.Categorical(perfect=True), (wide,), families=True, device_perfect=True)[0] == "rows"      # more symbols than the kernel has slots
    assert S.model_args(M.Categorical(perfect=True), (wide[:, :1024],), families=True, device_perfect=True)[0] == "categorical_perfect"
    ps = rng.uniform(0.0, 1.0, 11)
    ps[:2] = (0.0, 1.0)
    kind = S.model_args(M.Bernoulli(perfect=True), (ps,), families=True, device_perfect=True)
    assert kind[0] == "categorical_perfect" and kind[1].dtype == np.float64 and np.array_equal(kind[1], np.stack([1.0 - ps, ps], axis=1))
    assert S.model_args(M.Bernoulli(perfect=True), (ps,))[0] == "rows"
    assert S.model_args(M.Categorical(perfect=False), (mat,), families=True, device_perfect=True)[0] == "categorical"               # unchanged


def test_drop_in_keeps_the_reference_errors_for_invalid_perfect_matrices():
    pytest.importorskip("torch")
    from constriction_amd.stream import _single as S, model as M
    good = np.random.default_rng(6).dirichlet(np.ones(5), size=8)
    perfect = M.Categorical(perfect=True)
    for dtype in (np.float32, np.float64):
        for spoil in (np.nan, -0.5, np.inf):
            bad = good.astype(dtype)
            bad[3, 2] = spoil
            for device in (True, False):                                 # the device route and the host route refuse alike
                with pytest.raises(ValueError, match="not normalizable"):
                    S.model_args(perfect, (bad,), families=True, device_perfect=device)
        zero = good.astype(dtype)
        zero[5, :] = 0.0
        with pytest.raises(ValueError, match="not normalizable"):
            S.model_args(perfect, (zero,), families=True, device_perfect=True)
        with pytest.raises(ValueError, match="not normalizable"):
            S.model_args(perfect, (good.astype(dtype)[:, :1],), families=True, device_perfect=True)          # K < 2
    # an f32 row whose f32 sum would overflow is a valid model: the sum runs in f64
    huge = np.full((2, 4), np.finfo(np.float32).max, np.float32)
    assert S.model_args(perfect, (huge,), families=True, device_perfect=True)[0] == "categorical_perfect"
    assert S.model_args(perfect, (huge,))[0] == "rows"
    with pytest.raises(TypeError):
        S.model_args(perfect, (good.astype(np.float16),), families=True, device_perfect=True)
    for p in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="`p` must be"):
            S.model_args(M.Bernoulli(perfect=True), (np.array([0.5, p]),), families=True, device_perfect=True)
