"""CPU-only: fitting table models (csrc/cst_fit.hip, batched.count_symbols / fit_cdf_rows / Model.fit / Model.fit_per_stream /
Model.from_cdf_rows_per_stream / TableSet.fit) -- that the five entry points are named at every layer, what they refuse before the
device is touched, the counts -> cdf rows rule (cst_fit_cdf_rows_host) against the oracle's quantisers, and the ValueErrors of the
Python layer.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
NAMES = ["cst_count_symbols", "cst_count_symbols_per_stream", "cst_fit_cdf_rows", "cst_fit_cdf_rows_host",
         "cst_model_create_tables_per_stream"]


@pytest.fixture(scope="module")
def N():
    from constriction_amd import build, _native
    build.build_library()
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_the_names_are_everywhere(N):
    header = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    wrappers = (ROOT / "bindings" / "rust" / "src" / "lib.rs").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    lib = N.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert re.search(r"ffi::%s\s*\(" % name, wrappers), name
        assert name in design, name
    assert "4.33" in design
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def test_count_argument_errors_come_before_the_device(N):
    lib, bad = N.load_library(), N.CST_ERR_INVALID_ARGUMENT
    buf = C.create_string_buffer(64)        # dummy non-NULL pointers: nothing is dereferenced before the checks pass, and they never pass here
    p = C.addressof(buf)

    def shared(sym=p, n_total=8, lo=0, n=16, idx=None, ib=0, k=1, counts=p, outside=p):
        return lib.cst_count_symbols(sym, n_total, lo, n, idx, ib, k, counts, outside, None)

    assert shared(sym=None) == bad and shared(counts=None) == bad and shared(outside=None) == bad
    assert shared(k=2) == bad                               # more than one table needs indices
    for ib in (0, 2, 8, -1):
        assert shared(idx=p, ib=ib, k=4) == bad, ib
    for k in (0, 257, -1):
        assert shared(idx=p, ib=1, k=k) == bad, k
    for n in (1, 0, 65537, -5):
        assert shared(n=n) == bad, n
    assert shared(n_total=2**31) == bad and shared(n_total=2**40) == bad
    assert shared(lo=2**31 - 4, n=16) == bad                # the support leaves int32

    def per_stream(sym=p, off=None, n_streams=2, n_per=4, lo=0, n=16, counts=p, outside=p):
        return lib.cst_count_symbols_per_stream(sym, off, n_streams, n_per, lo, n, counts, outside, None)

    assert per_stream(sym=None) == bad and per_stream(counts=None) == bad and per_stream(outside=None) == bad
    assert per_stream(n_streams=0) == bad
    for n in (1, 0, 1025, 65537):
        assert per_stream(n=n) == bad, n
    assert per_stream(n_streams=2**16, n_per=2**15) == bad and per_stream(n_streams=1, n_per=2**31) == bad
    assert per_stream(n_streams=2**31, n_per=0) == bad
    assert per_stream(lo=2**31 - 4, n=16) == bad


def test_rows_and_model_argument_errors_come_before_the_device(N):
    lib, bad, model = N.load_library(), N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    for fn, tail in ((lib.cst_fit_cdf_rows, (None, None)), (lib.cst_fit_cdf_rows_host, (None,))):
        assert fn(12, 0, None, 1, 8, p, *tail) == bad and fn(12, 0, p, 1, 8, None, *tail) == bad
        for precision in (0, 32, -1):
            assert fn(precision, 0, p, 1, 8, p, *tail) == bad, precision
        assert fn(12, 0, p, 1, 1, p, *tail) == model                      # fewer than two symbols
        assert fn(12, 1, p, 1, 1025, p, *tail) == model                   # perfect: more than CST_CATEGORICAL_PERFECT_MAX_K symbols
        assert fn(3, 0, p, 1, 7, p, *tail) == model                       # the fast quantiser's n < 2^P - 1
        assert fn(3, 1, p, 1, 9, p, *tail) == model                       # the perfect quantiser's n <= 2^P
        assert fn(12, 0, p, 0, 8, p, *tail) == N.CST_OK                   # no rows: nothing to do
    out = C.c_void_p()

    def create(precision=12, lo=0, n=8, rows=p, k=2, o=C.byref(out)):
        return lib.cst_model_create_tables_per_stream(precision, lo, n, rows, k, None, o)

    assert create(rows=None) == bad and create(o=None) == bad and create(k=0) == bad
    for precision in (17, 24, 0, 25):
        assert create(precision=precision, n=2) == bad, precision
    assert create(n=1) == model and create(precision=2, n=5) == model
    assert create(lo=2**31 - 4) == bad
    assert not out.value


def host_rows(N, counts, P, perfect):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    rows = np.zeros((counts.shape[0], counts.shape[1] + 1), np.uint32)
    empty = np.full(counts.shape[0], -1, np.int32)
    rc = N.load_library().cst_fit_cdf_rows_host(P, int(perfect), counts.ctypes.data, counts.shape[0], counts.shape[1], rows.ctypes.data,
                                                empty.ctypes.data)
    return rc, rows, empty


def count_rows(n, seed):
    """random counts, counts with many zeros, one non-zero bin (each end and the middle), counts near 2^31"""
    rng = np.random.default_rng(seed)
    sparse = rng.integers(0, 1000, n) * (rng.random(n) < 0.1)
    sparse[rng.integers(0, n)] += 1
    rows = [rng.integers(0, 5000, n), rng.integers(1, 3, n), sparse, rng.integers(2**31 - 1000, 2**31, n),
            np.where(np.arange(n) == 0, 2**31 - 1, 0)]
    for hot in (0, n // 2, n - 1):
        one = np.zeros(n, np.int64)
        one[hot] = rng.integers(1, 10**6)
        rows.append(one)
    return np.stack(rows).astype(np.uint32)


def rows_valid(rows, P):
    r = rows.astype(np.int64)
    return bool((r[:, 0] == 0).all() and (r[:, -1] == 1 << P).all() and (np.diff(r, axis=1) > 0).all())


@pytest.mark.parametrize("P", [8, 12, 16, 24])
@pytest.mark.parametrize("n", [2, 255, 1024])
@pytest.mark.parametrize("perfect", [False, True], ids=["fast", "perfect"])
def test_host_rows_equal_the_oracle(N, O, n, P, perfect):
    counts = count_rows(n, 1000 * n + P)
    rc, rows, empty = host_rows(N, counts, P, perfect)
    if n > (1 << P) if perfect else n >= (1 << P) - 1:          # the quantiser itself refuses the shape, and so does the reference
        with pytest.raises(ValueError):
            (O.categorical_perfect_cdf if perfect else O.categorical_fast_cdf)(counts[0].astype(np.float64), P)
        assert rc == N.CST_ERR_MODEL
        return
    assert rc == N.CST_OK and not empty.any()
    quantise = O.categorical_perfect_cdf if perfect else O.categorical_fast_cdf
    for r in range(len(counts)):
        assert rows[r].tolist() == quantise(counts[r].astype(np.float64), P).tolist(), r
    assert rows_valid(rows, P)                                 # what cst_model_create_table asks of a row


@pytest.mark.parametrize("perfect", [False, True], ids=["fast", "perfect"])
def test_a_row_without_counts_is_the_row_of_ones(N, O, perfect):
    n, P = 37, 12
    counts = count_rows(n, 5)
    counts[[1, 4]] = 0
    ones = counts.copy()
    ones[[1, 4]] = 1
    rc, rows, empty = host_rows(N, counts, P, perfect)
    rc1, rows1, empty1 = host_rows(N, ones, P, perfect)
    assert rc == rc1 == N.CST_OK
    assert np.array_equal(rows, rows1)
    assert empty.tolist() == [int(r in (1, 4)) for r in range(len(counts))] and not empty1.any()
    assert rows_valid(rows, P)
    lib = N.load_library()                                     # the flags are optional
    again = np.zeros_like(rows)
    assert lib.cst_fit_cdf_rows_host(P, int(perfect), counts.ctypes.data, len(counts), n, again.ctypes.data, None) == N.CST_OK
    assert np.array_equal(again, rows)


def test_fitted_rows_make_models_and_table_sets(N):
    """every row the host form produces passes cst_model_create_table's and cst_table_set_create's validation: the calls get as far
    as asking for a device"""
    lib = N.load_library()
    counts = count_rows(64, 9)
    counts[2] = 0
    for perfect in (False, True):
        rc, rows, _ = host_rows(N, counts, 12, perfect)
        assert rc == N.CST_OK
        for r in range(len(rows)):
            out = C.c_void_p()
            rc = lib.cst_model_create_table(12, -3, 64, rows[r].ctypes.data, C.byref(out))
            assert rc in (N.CST_OK, N.CST_ERR_NO_DEVICE), (perfect, r, rc)
            if rc == N.CST_OK:
                lib.cst_model_destroy(out)
        out = C.c_void_p()
        rc = lib.cst_table_set_create(12, -3, 64, len(rows), rows.ctypes.data, C.byref(out))
        assert rc in (N.CST_OK, N.CST_ERR_NO_DEVICE), (perfect, rc)
        if rc == N.CST_OK:
            lib.cst_table_set_destroy(out)


def test_python_layer_value_errors_need_no_device(N):
    torch = pytest.importorskip("torch")
    from constriction_amd import batched as B
    sym = torch.zeros((3, 8), dtype=torch.int32)
    idx = torch.zeros((3, 8), dtype=torch.uint8)
    off = torch.tensor([0, 8, 24], dtype=torch.int64)
    bad_calls = [
        lambda: B.count_symbols(sym, 0, 15),                                               # symbols in host memory
        lambda: B.count_symbols(sym.to(torch.int64), 0, 15),
        lambda: B.count_symbols(np.zeros(8, np.int32), 0, 15),
        lambda: B.count_symbols(sym, 0, 0),                                                # one symbol
        lambda: B.count_symbols(sym, 5, 4),
        lambda: B.count_symbols(sym, 0, 65536),                                            # 65 537 symbols
        lambda: B.count_symbols(sym, 0, 1024, per_stream=True),                            # 1025 symbols per stream
        lambda: B.count_symbols(sym, 0, 2**31),
        lambda: B.count_symbols(sym, 0, 15, indices=idx),                                  # indices without n_tables
        lambda: B.count_symbols(sym, 0, 15, n_tables=4),
        lambda: B.count_symbols(sym, 0, 15, indices=idx, n_tables=0),
        lambda: B.count_symbols(sym, 0, 15, indices=idx, n_tables=257),
        lambda: B.count_symbols(sym, 0, 15, indices=idx[:, :7], n_tables=4),
        lambda: B.count_symbols(sym, 0, 15, indices=idx.to(torch.int8), n_tables=4),
        lambda: B.count_symbols(sym, 0, 15, indices=idx.to(torch.int64), n_tables=4),
        lambda: B.count_symbols(sym, 0, 15, indices=idx, n_tables=4),                      # everything in host memory
        lambda: B.count_symbols(sym, 0, 15, indices=idx, n_tables=4, per_stream=True),
        lambda: B.count_symbols(sym.reshape(-1), 0, 15, per_stream=True),                  # flat symbols without offsets
        lambda: B.count_symbols(sym, 0, 15, per_stream=True, sym_offsets=off),             # offsets with a matrix
        lambda: B.count_symbols(sym.reshape(-1), 0, 15, per_stream=True, sym_offsets=off.to(torch.int32)),
        lambda: B.count_symbols(sym.reshape(-1), 0, 15, per_stream=True, sym_offsets=off[:1]),
        lambda: B.count_symbols(sym.reshape(-1), 0, 15, sym_offsets=off),                  # offsets without per_stream
        lambda: B.count_symbols(sym.reshape(-1), 0, 15, per_stream=True, sym_offsets=off),  # host memory
        lambda: B.fit_cdf_rows(torch.zeros((2, 8), dtype=torch.int32), 12),                # host memory
        lambda: B.fit_cdf_rows(torch.zeros((2, 8), dtype=torch.int64), 12),
        lambda: B.fit_cdf_rows(torch.zeros(8, dtype=torch.int32), 12),
        lambda: B.fit_cdf_rows(torch.zeros((2, 1), dtype=torch.int32), 12),
        lambda: B.fit_cdf_rows(torch.zeros((2, 8), dtype=torch.int32), 0),
        lambda: B.fit_cdf_rows(torch.zeros((2, 8), dtype=torch.int32), 32),
        lambda: B.fit_cdf_rows(torch.zeros((2, 7), dtype=torch.int32), 3),                 # fast: n < 2^P - 1
        lambda: B.fit_cdf_rows(torch.zeros((2, 1025), dtype=torch.int32), 12, perfect=True),
        lambda: B.Model.fit(sym, 0, 15, 12),
        lambda: B.Model.fit(sym, 0, 15, 25),
        lambda: B.Model.fit_per_stream(sym, 0, 15, 12),
        lambda: B.Model.fit_per_stream(sym, 0, 15, 17),                                    # per-stream tables stop at 16 bits
        lambda: B.Model.fit_per_stream(sym, 0, 1024, 12),
        lambda: B.TableSet.fit(sym, idx, 4, 0, 15, 12),
        lambda: B.TableSet.fit(sym, idx, 4, 0, 15, 25),
        lambda: B.TableSet.fit(sym, None, 4, 0, 15, 12),
        lambda: B.TableSet.fit(sym, idx, 300, 0, 15, 12),
        lambda: B.Model.from_cdf_rows_per_stream(torch.zeros((2, 9), dtype=torch.int32), 0, 12),      # host memory
        lambda: B.Model.from_cdf_rows_per_stream(torch.zeros((2, 9), dtype=torch.int64), 0, 12),
        lambda: B.Model.from_cdf_rows_per_stream(torch.zeros(9, dtype=torch.int32), 0, 12),
        lambda: B.Model.from_cdf_rows_per_stream(np.zeros(9, np.uint32), 0, 12),
        lambda: B.Model.from_cdf_rows_per_stream(np.zeros((2, 9), np.float64), 0, 12),
        lambda: B.Model.from_cdf_rows_per_stream(np.zeros((2, 2), np.uint32), 0, 12),       # one symbol
        lambda: B.Model.from_cdf_rows_per_stream(np.zeros((0, 9), np.uint32), 0, 12),
        lambda: B.Model.from_cdf_rows_per_stream(np.zeros((2, 9), np.uint32), 0, 17),
        lambda: B.Model.from_cdf_rows_per_stream([[0, 1, 2]], 0, 12),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert k >= 0
