"""CPU-only: what indexed table coding (csrc/cst_indexed.hip, batched.TableSet / *_indexed) decides before any device call -- the
argument errors of cst_table_set_create and of the four cst_*_indexed_batch entry points, the ValueErrors of the Python layer --
and that the header, the ctypes binding and the Rust declarations all list the new names.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"
NAMES = ["cst_table_set_create", "cst_table_set_destroy", "cst_table_set_precision", "cst_table_set_min_symbol", "cst_table_set_n_symbols",
         "cst_table_set_n_tables", "cst_ans_encode_indexed_batch", "cst_ans_decode_indexed_batch", "cst_range_encode_indexed_batch",
         "cst_range_decode_indexed_batch"]


@pytest.fixture(scope="module")
def N():
    from constriction_amd import build, _native
    build.build_library()
    _native.load_library()
    return _native


def test_the_names_are_everywhere(N):
    header = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    lib = N.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"#define\s+CST_ABI_VERSION\s+5\b", HEADER.read_text()) and lib.cst_abi_version() == 5


def cdfs_of(k, n, p):
    """k valid rows: row r gives symbol r % n all the weight the others leave"""
    rows = np.zeros((k, n + 1), dtype=np.uint32)
    for r in range(k):
        prob = np.ones(n, dtype=np.int64)
        prob[r % n] = (1 << p) - (n - 1)
        rows[r, 1:] = np.cumsum(prob)
    return rows


def create(N, p, lo, n, k, rows):
    out = C.c_void_p()
    rc = N.load_library().cst_table_set_create(p, lo, n, k, None if rows is None else rows.ctypes.data, C.byref(out))
    assert not out.value or rc == N.CST_OK
    return rc, out


def test_table_set_argument_errors_come_before_the_device(N):
    lib = N.load_library()
    rows = cdfs_of(4, 5, 12)
    assert lib.cst_table_set_create(12, 0, 5, 4, rows.ctypes.data, None) == N.CST_ERR_INVALID_ARGUMENT
    assert create(N, 12, 0, 5, 4, None)[0] == N.CST_ERR_INVALID_ARGUMENT
    for k in (0, 257, -1):
        assert create(N, 12, 0, 5, k, cdfs_of(max(k, 1), 5, 12))[0] == N.CST_ERR_INVALID_ARGUMENT, k
    for p in (0, 25, -3):
        assert create(N, p, 0, 5, 4, rows)[0] == N.CST_ERR_INVALID_ARGUMENT, p
    assert create(N, 12, 2**31 - 3, 5, 4, rows)[0] == N.CST_ERR_INVALID_ARGUMENT      # the support leaves int32
    # the rules of cst_model_create_table, row by row
    assert create(N, 12, 0, 1, 4, cdfs_of(4, 2, 12))[0] == N.CST_ERR_MODEL              # fewer than two symbols
    assert create(N, 2, 0, 5, 1, cdfs_of(1, 5, 12))[0] == N.CST_ERR_MODEL               # more symbols than quantiles
    for r, (i, v) in enumerate([(0, 1), (5, 4095), (5, 4097), (3, None)]):               # cdf[0] != 0, cdf[n] != 2^P twice, a zero probability
        bad = rows.copy()
        bad[r, i] = bad[r, i - 1] if v is None else v
        assert create(N, 12, 0, 5, 4, bad)[0] == N.CST_ERR_MODEL, (r, i, v)
    # a set whose image does not fit beside the rings and tiles: 256 tables of 255 symbols are 128 KiB of 16-bit rows
    assert create(N, 16, -127, 255, 256, cdfs_of(256, 255, 16))[0] == N.CST_ERR_MODEL
    assert create(N, 24, -127, 255, 128, cdfs_of(128, 255, 24))[0] == N.CST_ERR_MODEL
    # what must fit is refused only for want of a device here (or built, where there is one)
    for p, n, k in ((16, 255, 64), (24, 255, 64), (16, 64, 256)):
        rc, h = create(N, p, 0, n, k, cdfs_of(k, n, p))
        assert rc in (N.CST_OK, N.CST_ERR_NO_DEVICE), (p, n, k, rc)
        if rc == N.CST_OK:
            assert (lib.cst_table_set_precision(h), lib.cst_table_set_n_symbols(h), lib.cst_table_set_n_tables(h)) == (p, n, k)
            assert lib.cst_table_set_destroy(h) == N.CST_OK
    # the getters and destroy on what is no table set
    junk = C.create_string_buffer(256)
    for getter in ("precision", "min_symbol", "n_symbols", "n_tables"):
        assert getattr(lib, "cst_table_set_" + getter)(None) == 0 and getattr(lib, "cst_table_set_" + getter)(junk) == 0
    assert lib.cst_table_set_destroy(None) == N.CST_OK and lib.cst_table_set_destroy(junk) == N.CST_ERR_INVALID_ARGUMENT


def coder_calls(N, tables, cfg, index_bytes=1, layout=0, flags=0, sym=1, idx=1, words=1, n_words=1, status=1):
    """the four entry points with dummy non-NULL pointers (nothing is dereferenced before the checks pass, and they never pass here)"""
    lib = N.load_library()
    buf = C.create_string_buffer(64)
    p = lambda on: C.addressof(buf) if on else None
    return [
        lib.cst_ans_encode_indexed_batch(tables, cfg, p(sym), p(idx), index_bytes, 1, 4, layout, p(words), 16, p(n_words), None, p(status), flags, None),
        lib.cst_range_encode_indexed_batch(tables, cfg, p(sym), p(idx), index_bytes, 1, 4, layout, p(words), 16, p(n_words), None, p(status), flags, None),
        lib.cst_ans_decode_indexed_batch(tables, cfg, p(words), None, 16, 16, p(n_words), p(idx), index_bytes, p(sym), 1, 4, layout, None, None,
                                         p(status), flags, None),
        lib.cst_range_decode_indexed_batch(tables, cfg, p(words), None, 16, 16, p(n_words), p(idx), index_bytes, p(sym), 1, 4, layout, None,
                                           p(status), flags, None),
    ]


def test_coder_argument_errors_come_before_the_device(N):
    bad = [N.CST_ERR_INVALID_ARGUMENT] * 4
    cfg = N.CoderConfig(32, 64, 12)
    not_a_set = C.create_string_buffer(256)             # a handle that is no live table set: refused, never followed
    for tables in (None, not_a_set):
        assert coder_calls(N, tables, cfg) == bad
    for kw in (dict(index_bytes=0), dict(index_bytes=2), dict(index_bytes=8), dict(layout=N.LAYOUT_SYMBOL_MAJOR), dict(layout=7),
               dict(flags=N.FLAG_RAW_STATE), dict(flags=N.FLAG_COLD_WORDS), dict(sym=0), dict(idx=0), dict(words=0), dict(n_words=0),
               dict(status=0)):
        assert coder_calls(N, not_a_set, cfg, **kw) == bad, kw
    for other in (N.CoderConfig(16, 32, 12), N.CoderConfig(32, 32, 12), N.CoderConfig(16, 64, 12)):
        assert coder_calls(N, not_a_set, other) == bad


def test_python_layer_value_errors_need_no_device(N):
    torch = pytest.importorskip("torch")
    from constriction_amd import batched as B
    rows = cdfs_of(4, 5, 12)
    for bad_rows, lo, p in ((rows[0], 0, 12), (rows[:, :2], 0, 12), (np.zeros((0, 6), np.uint32), 0, 12), (cdfs_of(257, 5, 12), 0, 12),
                            (rows, 0, 0), (rows, 0, 25)):
        with pytest.raises(ValueError):
            B.TableSet.from_cdfs(bad_rows, lo, p)
    broken = rows.copy()
    broken[2, 3] = broken[2, 2]
    with pytest.raises(ValueError):                     # CST_ERR_MODEL, decided before the device is asked for
        B.TableSet.from_cdfs(broken, 0, 12)
    with pytest.raises(ValueError):
        B.TableSet.quantized_gaussians(-4, 4, [0.0, 1.0], [1.0], 12)

    tables = B.TableSet(None, rows, 0, 12)              # no handle: the checks below come before it is used
    assert (tables.precision, tables.min_symbol, tables.n_symbols, tables.n_tables) == (12, 0, 5, 4)
    assert np.array_equal(tables.cdfs(), rows)
    sym = torch.zeros((3, 8), dtype=torch.int32)
    idx = torch.zeros((3, 8), dtype=torch.uint8)
    for enc in (B.ans_encode_indexed, B.range_encode_indexed):
        with pytest.raises(ValueError):                 # symbols in host memory
            enc(sym, idx, tables, (32, 64, 12))
    # the index checks, on tensors that claim no device: shape, dtype, device, configuration
    device = torch.device("cpu")
    for bad_idx in (torch.zeros((3, 7), dtype=torch.uint8), torch.zeros((8, 3), dtype=torch.uint8), torch.zeros(24, dtype=torch.uint8),
                    torch.zeros((3, 8), dtype=torch.int64), torch.zeros((3, 8), dtype=torch.int8), torch.zeros((3, 8), dtype=torch.float32),
                    np.zeros((3, 8), np.uint8), idx):
        with pytest.raises(ValueError):
            B._indexed_args((3, 8), device, bad_idx, tables, (32, 64, 12))
    for config in ((16, 32, 12), (32, 64, 16), (32, 32, 12)):
        with pytest.raises(ValueError):
            B._indexed_args((3, 8), device, idx, tables, config)
    with pytest.raises(ValueError):
        B._indexed_args((3, 8), device, idx, "not a table set", (32, 64, 12))
    words, n_words = torch.zeros((3, 16), dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    for dec in (B.ans_decode_indexed, B.range_decode_indexed):
        with pytest.raises(ValueError):                 # indices of another shape
            dec((words, n_words), torch.zeros((3, 7), dtype=torch.uint8), tables, 8)
        with pytest.raises(ValueError):                 # indices in host memory
            dec((words, n_words), idx, tables, 8)
        with pytest.raises(ValueError):
            dec(B.EncodedBatch(words, n_words, n_words, (32, 64, 24)), idx, tables, 8)
