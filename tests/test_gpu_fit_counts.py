"""GPU: the counting kernels of csrc/cst_fit.hip against np.bincount (exactly; counts.sum() + outside == n_total), the device
quantisation of counts against cst_fit_cdf_rows_host, and Model.fit / Model.fit_per_stream / TableSet.fit against the oracle's
quantisers over np.bincount."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from constriction_amd import batched
    return batched


@pytest.fixture(scope="module")
def N():
    from constriction_amd import _native
    return _native


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def want_counts(sym, lo, n, rows=None, n_rows=1):
    """np.bincount over symbol - lo + row * n of what lies inside; (counts [n_rows, n], outside)"""
    sym = np.asarray(sym, dtype=np.int64).reshape(-1)
    rows = np.zeros(len(sym), np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    inside = (sym >= lo) & (sym < lo + n) & (rows >= 0) & (rows < n_rows)
    counts = np.bincount((sym - lo + rows * n)[inside], minlength=n_rows * n).reshape(n_rows, n)
    return counts, int((~inside).sum())


def check(counts, outside, want, want_outside, n_total):
    got = counts.cpu().numpy().astype(np.int64)
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    assert int(outside.item()) == want_outside
    assert got.sum() + int(outside.item()) == n_total


def draw(rng, kind, n_total, lo, n):
    if kind == "uniform":
        return rng.integers(lo, lo + n, n_total, dtype=np.int64).astype(np.int32)
    if kind == "constant":                       # every symbol equal: all lanes of every wave on one address
        return np.full(n_total, lo + n // 3, np.int32)
    sym = rng.integers(lo, lo + n, n_total, dtype=np.int64)
    strays = np.array([lo - 1, lo + n, -2**31, 2**31 - 1], np.int64)
    where = rng.random(n_total) < 0.3
    sym[where] = strays[rng.integers(0, 4, int(where.sum()))]
    return sym.astype(np.int32)


@pytest.mark.parametrize("kind", ["uniform", "constant", "strays"])
@pytest.mark.parametrize("n", [2, 255, 1024, 20000])
@pytest.mark.parametrize("n_total", [1, 63, 64, 65, 1027, 100003])
def test_shared_counts(B, kind, n, n_total):
    lo = -(n // 2)
    sym = draw(np.random.default_rng(n * 131 + n_total), kind, n_total, lo, n)
    counts, outside = B.count_symbols(dev(sym), lo, lo + n - 1)
    assert B.last_kernel() == ("fit_count_kernel<lds>" if n <= 16384 else "fit_count_kernel<global>")
    check(counts, outside, *want_counts(sym, lo, n), n_total)


@pytest.mark.parametrize("n", [255, 20000])
def test_shared_counts_of_a_view_off_the_16_byte_boundary(B, n):
    """a view that starts 4 bytes behind a 16-byte boundary, and one 12 bytes behind: the kernel's 16-byte loads start at the next one"""
    rng = np.random.default_rng(n)
    sym = draw(rng, "strays", 100003, -7, n)
    whole = dev(sym)
    assert whole.data_ptr() % 16 == 0
    for first in (1, 3):
        view = whole[first:]
        assert view.data_ptr() % 16 == 4 * first and view.is_contiguous()
        counts, outside = B.count_symbols(view, -7, -7 + n - 1)
        check(counts, outside, *want_counts(sym[first:], -7, n), len(sym) - first)


def test_shared_counts_of_a_matrix_and_of_nothing(B):
    rng = np.random.default_rng(3)
    sym = rng.integers(-5, 9, (37, 53)).astype(np.int32)
    counts, outside = B.count_symbols(dev(sym), -3, 6)
    check(counts, outside, *want_counts(sym, -3, 10), sym.size)
    counts, outside = B.count_symbols(torch.zeros(0, dtype=torch.int32, device="cuda"), -3, 6)
    assert counts.shape == (1, 10) and not counts.any() and int(outside.item()) == 0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32], ids=["u8", "i32"])
@pytest.mark.parametrize("K", [1, 3, 64, 256])
@pytest.mark.parametrize("n,n_total", [(64, 1027), (255, 100003), (20000, 4099)])
def test_indexed_counts(B, K, dtype, n, n_total):
    """K * 64 bins fit into LDS for every K, K * 255 from K = 64 on only without replicas, K * 20000 never"""
    rng = np.random.default_rng(K * 7 + n)
    lo = 10
    sym = draw(rng, "strays", n_total, lo, n)
    idx = rng.integers(0, K, n_total)
    if dtype == torch.int32:                     # indices outside [0, K) count as outside
        stray = rng.random(n_total) < 0.1
        idx[stray] = rng.choice([-1, K, K + 1000, -2**31], int(stray.sum()))
        idx_t = dev(idx.astype(np.int32))
    else:
        idx_t = dev(idx.astype(np.uint8))
    for first in (0, 1):                         # and from a view 4 bytes (1 index byte) off the boundary
        counts, outside = B.count_symbols(dev(sym)[first:], lo, lo + n - 1, indices=idx_t[first:], n_tables=K)
        assert B.last_kernel() == ("fit_count_kernel<lds>" if K * n <= 16384 else "fit_count_kernel<global>")
        check(counts, outside, *want_counts(sym[first:], lo, n, idx[first:], K), n_total - first)


@pytest.mark.parametrize("uniform", [0, 1])
@pytest.mark.parametrize("replicas", [1, 2, 4, 8])
def test_the_measurement_switches_change_no_count(B, knob, replicas, uniform):
    """CST_FIT_REPLICAS / CST_FIT_WAVE_UNIFORM (scripts/bench_fit.py): one LDS copy or several, with and without the single add of a
    wave whose symbols share a bin -- on constant data, where that add is all there is, on stray-ridden data, and on both in one array"""
    knob(CST_FIT_REPLICAS=replicas, CST_FIT_WAVE_UNIFORM=uniform)
    rng = np.random.default_rng(replicas)
    n, lo = 101, -50
    constant = draw(rng, "constant", 100003, lo, n)
    strays = draw(rng, "strays", 100003, lo, n)
    outside = np.full(5000, lo + n, np.int32)                  # whole waves of one mind about a symbol that is in no bin
    for sym in (constant, strays, np.concatenate([constant[:4099], strays[:1000], outside, constant])):
        counts, n_outside = B.count_symbols(dev(sym), lo, lo + n - 1)
        check(counts, n_outside, *want_counts(sym, lo, n), len(sym))
        idx = rng.integers(0, 3, len(sym)).astype(np.uint8)
        counts, n_outside = B.count_symbols(dev(sym), lo, lo + n - 1, indices=dev(idx), n_tables=3)
        check(counts, n_outside, *want_counts(sym, lo, n, idx, 3), len(sym))


def test_indexed_counts_constant_data(B):
    sym = np.full((33, 1000), 4, np.int32)
    idx = np.full((33, 1000), 2, np.uint8)
    counts, outside = B.count_symbols(dev(sym), 0, 7, indices=dev(idx), n_tables=5)
    check(counts, outside, *want_counts(sym, 0, 8, idx, 5), sym.size)


@pytest.mark.parametrize("n", [2, 255, 1024])
@pytest.mark.parametrize("n_streams,n_per", [(1, 1), (3, 64), (65, 127), (257, 33), (2, 70001)])
def test_per_stream_counts(B, n, n_streams, n_per):
    rng = np.random.default_rng(n_streams * 11 + n_per + n)
    lo = -1
    sym = draw(rng, "strays", n_streams * n_per, lo, n).reshape(n_streams, n_per)
    sym[0] = lo + n - 1                          # one stream of one symbol: a whole row in one bin
    counts, outside = B.count_symbols(dev(sym), lo, lo + n - 1, per_stream=True)
    assert B.last_kernel() == "fit_count_ps_kernel"
    rows = np.repeat(np.arange(n_streams), n_per)
    check(counts, outside, *want_counts(sym, lo, n, rows, n_streams), sym.size)
    view = dev(np.concatenate([[0], sym.reshape(-1)]).astype(np.int32))[1:].reshape(n_streams, n_per)      # rows that start unaligned
    counts, outside = B.count_symbols(view, lo, lo + n - 1, per_stream=True)
    check(counts, outside, *want_counts(sym, lo, n, rows, n_streams), sym.size)


@pytest.mark.parametrize("n", [2, 255, 1024])
def test_per_stream_counts_ragged(B, n):
    """empty streams (first, last, two in a row), streams of one symbol, lengths that are no multiple of 4, one stream of 70 001
    symbols among short ones -- it spreads over 18 units of 4096 symbols and shares the first and the last with its neighbours"""
    rng = np.random.default_rng(n)
    lengths = np.array([0, 1, 5, 0, 0, 3, 70001, 1, 2, 4095, 4096, 4097, 7, 0, 33, 1, 0], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    total = int(offsets[-1])
    lo = 100
    sym = draw(rng, "strays", total, lo, n)
    rows = np.repeat(np.arange(len(lengths)), lengths)
    want, want_outside = want_counts(sym, lo, n, rows, len(lengths))
    counts, outside = B.count_symbols(dev(sym), lo, lo + n - 1, per_stream=True, sym_offsets=dev(offsets))
    check(counts, outside, want, want_outside, total)
    # the streams somewhere inside a longer buffer: offsets that do not begin at 0
    padded = np.concatenate([np.full(5, lo, np.int32), sym, np.full(9, lo, np.int32)])
    counts, outside = B.count_symbols(dev(padded), lo, lo + n - 1, per_stream=True, sym_offsets=dev(offsets + 5))
    check(counts, outside, want, want_outside, total)
    # nothing but empty streams
    counts, outside = B.count_symbols(dev(sym), lo, lo + n - 1, per_stream=True, sym_offsets=dev(np.zeros(4, np.int64)))
    assert counts.shape == (3, n) and not counts.any() and int(outside.item()) == 0


def test_ragged_offsets_beyond_the_symbols_are_refused(B):
    sym = torch.zeros(10, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        B.count_symbols(sym, 0, 3, per_stream=True, sym_offsets=dev(np.array([0, 4, 11], np.int64)))


def host_rows(N, counts, P, perfect):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    rows = np.zeros((counts.shape[0], counts.shape[1] + 1), np.uint32)
    empty = np.zeros(counts.shape[0], np.int32)
    assert N.load_library().cst_fit_cdf_rows_host(P, int(perfect), counts.ctypes.data, counts.shape[0], counts.shape[1], rows.ctypes.data,
                                                  empty.ctypes.data) == N.CST_OK
    return rows, empty


@pytest.mark.parametrize("perfect", [False, True], ids=["fast", "perfect"])
@pytest.mark.parametrize("n,P", [(2, 8), (37, 12), (255, 16), (1024, 24)])
def test_device_rows_equal_the_host_rows(B, N, n, P, perfect):
    rng = np.random.default_rng(n + P)
    counts = rng.integers(0, 3000, (70, n)) * (rng.random((70, n)) < 0.6)
    counts[0, 0] += 1
    counts[[5, 69]] = 0                                        # rows without a count
    counts[7] = rng.integers(2**31 - 100, 2**31, n)
    counts[9] = 0
    counts[9, n - 1] = 12345
    want, want_empty = host_rows(N, counts, P, perfect)
    rows, empty = B.fit_cdf_rows(dev(counts.astype(np.uint32).view(np.int32)), P, perfect, return_empty=True)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (70, n + 1)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), want)
    assert empty.cpu().numpy().tolist() == want_empty.tolist() and want_empty.sum() >= 2
    assert torch.equal(B.fit_cdf_rows(dev(counts.astype(np.uint32).view(np.int32)), P, perfect), rows)


def oracle_rows(O, counts, P, perfect):
    quantise = O.categorical_perfect_cdf if perfect else O.categorical_fast_cdf
    return np.stack([quantise((c if c.any() else np.ones_like(c)).astype(np.float64), P) for c in counts])


@pytest.mark.parametrize("perfect", [False, True], ids=["fast", "perfect"])
def test_fitted_models_equal_the_oracle(B, O, perfect):
    rng = np.random.default_rng(17)
    lo, hi, n = -20, 42, 63
    n_streams, n_per, K = 70, 257, 9
    sym = np.clip(np.round(rng.normal(3, 6, (n_streams, n_per))), lo, hi).astype(np.int32)
    sym[3] = 7                                                 # a stream that knows one symbol
    idx = rng.integers(0, K - 1, (n_streams, n_per)).astype(np.uint8)      # class K - 1 is named by nobody
    rows = np.repeat(np.arange(n_streams), n_per)

    shared = B.Model.fit(dev(sym), lo, hi, 16, perfect)
    assert shared.cdf().tolist() == oracle_rows(O, want_counts(sym, lo, n)[0], 16, perfect)[0].tolist()
    assert (shared.min_symbol, shared.n_symbols, shared.n_tables, shared.precision) == (lo, n, 1, 16)

    per = B.Model.fit_per_stream(dev(sym), lo, hi, 12, perfect)
    want = oracle_rows(O, want_counts(sym, lo, n, rows, n_streams)[0], 12, perfect)
    assert (per.n_tables, per.n_symbols, per.min_symbol) == (n_streams, n, lo)
    assert np.array_equal(per.cdfs_device().cpu().numpy().view(np.uint32), want)
    assert per.cdf(3).tolist() == want[3].tolist()

    lengths = rng.integers(0, 40, n_streams)
    lengths[[0, 11]] = 0
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flat = sym.reshape(-1)[: offsets[-1]]
    ragged = B.Model.fit_per_stream(dev(flat), lo, hi, 12, perfect, sym_offsets=dev(offsets))
    want = oracle_rows(O, want_counts(flat, lo, n, np.repeat(np.arange(n_streams), lengths), n_streams)[0], 12, perfect)
    assert np.array_equal(ragged.cdfs_device().cpu().numpy().view(np.uint32), want)

    tables = B.TableSet.fit(dev(sym), dev(idx), K, lo, hi, 14, perfect)
    want = oracle_rows(O, want_counts(sym, lo, n, idx, K)[0], 14, perfect)
    assert np.array_equal(tables.cdfs(), want) and tables.n_tables == K
    assert tables.cdfs()[K - 1].tolist() == oracle_rows(O, np.ones((1, n), np.int64), 14, perfect)[0].tolist()


def test_fit_refuses_data_outside_the_support(B):
    sym = np.zeros((4, 50), np.int32)
    sym[2, 7], sym[3, 49] = 9, -1
    idx = np.zeros((4, 50), np.int32)
    for call in (lambda: B.Model.fit(dev(sym), 0, 8, 12), lambda: B.Model.fit_per_stream(dev(sym), 0, 8, 12),
                 lambda: B.TableSet.fit(dev(sym), dev(idx), 3, 0, 8, 12)):
        with pytest.raises(ValueError, match="2 symbols"):
            call()
    idx[1, 1] = 3                                              # an index that names no table
    with pytest.raises(ValueError, match="1 symbols"):
        B.TableSet.fit(dev(np.zeros((4, 50), np.int32)), dev(idx), 3, 0, 8, 12)
    B.Model.fit(dev(sym), -1, 9, 12)                           # and inside it, no complaint
