"""GPU: per-stream table models built from device cdf rows (Model.from_cdf_rows_per_stream, cst_model_create_tables_per_stream) through
the kernels that had only ever seen Gaussian rows -- the compact-row pair of cst_ans_pt.hip, the full-row pair, the checkpointing
encoder and the sub-lane decoder, int8 matrices -- against the CPU oracle bit for bit, and the fitted models end to end."""
import os

import numpy as np
import pytest

from kernel_names import with_jump

pytestmark = pytest.mark.gpu
ALT = any(os.environ.get(k) for k in ("CST_NO_N8", "CST_PT_SUB_WAVES", "CST_AUTO_JUMP"))
torch = pytest.importorskip("torch")

SHAPES = [(64, 96), (130, 100), (257, 4096 + 3)]


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


def cdfs_of(prob):
    """probabilities [S, n] (integers >= 1 that sum to 2^P) -> cdf rows [S, n + 1]"""
    rows = np.zeros((prob.shape[0], prob.shape[1] + 1), np.uint32)
    rows[:, 1:] = np.cumsum(prob, axis=1)
    return rows


def rest_on(n_streams, n, P, where):
    """every probability 1, what is left on symbol where[s]"""
    prob = np.ones((n_streams, n), np.int64)
    prob[np.arange(n_streams), where] = (1 << P) - (n - 1)
    return prob


# case -> (n_symbols, P, the kernels the rows must take: "pt" compact rows, "ps" full rows)
CASES = {
    "skewed_fitted": (40, 12, "pt"),        # rows fitted to geometric data: a few large bins, a long unit run behind them
    "bimodal": (255, 12, "pt"),             # two peaks, unit runs in front, BETWEEN and behind them
    "one_interior": (255, 12, "pt"),        # all the mass on one symbol inside the support
    "one_first": (255, 12, "pt"),
    "one_last": (255, 12, "pt"),
    "uniform": (255, 12, "ps"),             # no unit run anywhere: 256 rows of 255 entries do not fit beside the rings and tiles
    "alternating": (255, 12, "ps"),         # 1, large, 1, large, ...: no run reaches length 2, nothing is trimmed or merged
    "alternating_small": (40, 12, "pt"),    # ... and at a size where the image fits
    "n2": (2, 12, "pt"),
    "n256": (256, 12, "pt"),
    "n257": (257, 12, "ps"),                # beyond the compact image's 8-bit symbol index
    "n_2_to_P": (256, 8, "pt"),             # n = 2^P: every probability is 1, one run is the whole row
}


def case_rows(O, case, n_streams, rng):
    n, P, _ = CASES[case]
    total = 1 << P
    s = np.arange(n_streams)
    if case == "skewed_fitted":
        data = np.minimum(rng.geometric(rng.uniform(0.2, 0.7, (n_streams, 1)), (n_streams, 3000)) - 1, n - 1)
        return np.stack([O.categorical_fast_cdf(np.bincount(d, minlength=n).astype(np.float64), P) for d in data])
    if case in ("bimodal", "n256"):
        prob = np.ones((n_streams, n), np.int64)
        a, b = rng.integers(60, 100, n_streams), rng.integers(120, 160, n_streams)
        left = total - n
        share = rng.integers(1, left, n_streams)
        prob[s, a] += share
        prob[s, b] += left - share
        return cdfs_of(prob)
    if case == "one_interior":
        return cdfs_of(rest_on(n_streams, n, P, rng.integers(1, n - 1, n_streams)))
    if case == "one_first":
        return cdfs_of(rest_on(n_streams, n, P, np.zeros(n_streams, np.int64)))
    if case == "one_last":
        return cdfs_of(rest_on(n_streams, n, P, np.full(n_streams, n - 1)))
    if case == "uniform":
        prob = np.full((n_streams, n), total // n, np.int64)
        prob[s, rng.integers(0, n, n_streams)] += total - n * (total // n)
        assert (prob >= 2).all()
        return cdfs_of(prob)
    if case in ("alternating", "alternating_small"):
        prob = np.ones((n_streams, n), np.int64)
        large = np.arange(1, n, 2)
        prob[:, large] = (total - (n - len(large))) // len(large)
        prob[s, large[rng.integers(0, len(large), n_streams)]] += total - prob.sum(axis=1)
        return cdfs_of(prob)
    if case == "n2":
        first = rng.integers(1, total, n_streams)
        first[:3] = [1, total - 1, total // 2]
        return cdfs_of(np.stack([first, total - first], axis=1))
    if case == "n257":
        return cdfs_of(rest_on(n_streams, n, P, rng.integers(0, n, n_streams)))
    assert case == "n_2_to_P"
    return cdfs_of(np.ones((n_streams, n), np.int64))


def batch(O, case, n_streams, n_per):
    """(lo, P, cdfs, symbols): symbols drawn from the rows, the first and last two symbols of the support forced in"""
    n, P, _ = CASES[case]
    lo = -127 if n <= 255 else -128
    rng = np.random.default_rng(n_streams * 7 + n_per + n)
    cdfs = case_rows(O, case, n_streams, rng)
    assert cdfs.shape == (n_streams, n + 1) and (cdfs[:, -1] == 1 << P).all() and (np.diff(cdfs.astype(np.int64), axis=1) > 0).all()
    sym = O.synth_symbols(0xF17, 0, n_streams, n_per, lo, cdfs, P, per_stream_tables=True)
    hi = lo + n - 1
    sym[:, :4] = np.array([lo, hi, lo + 1, hi - 1])[: sym[:, :4].shape[1]]
    return lo, P, cdfs, sym


def assert_words(enc, want_words, want_n, want_status):
    words, n_words, status = enc.to_numpy()
    assert (status == 0).all() and (want_status == 0).all()
    assert n_words.tolist() == want_n.tolist()
    for s in range(len(want_n)):
        assert words[s, : n_words[s]].tolist() == want_words[s, : want_n[s]].tolist(), f"stream {s}"


@pytest.mark.parametrize("n_streams,n_per", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_rows_no_gaussian_makes(B, O, case, n_streams, n_per):
    lo, P, cdfs, sym = batch(O, case, n_streams, n_per)
    cfg = (32, 64, P)
    model = B.Model.from_cdf_rows_per_stream(dev(cdfs.view(np.int32)), lo, P)
    assert (model.n_tables, model.n_symbols, model.min_symbol, model.precision) == (n_streams, cdfs.shape[1] - 1, lo, P)
    assert np.array_equal(model.cdfs_device().cpu().numpy().view(np.uint32), cdfs)
    want = O.ans_encode_batch(sym, lo, cdfs, P, 32, 64)
    enc = B.ans_encode(dev(sym), model, cfg, jump_points=0)
    path = CASES[case][2]
    assert ALT or B.last_kernel() == ("ans_encode_pt_kernel" if path == "pt" else "ans_encode_per_stream_kernel"), B.last_kernel()
    assert_words(enc, *want)
    dec, dstatus = B.ans_decode(enc, model, n_per)
    assert ALT or B.last_kernel() == ("ans_decode_pt_kernel" if path == "pt" else "ans_decode_per_stream_kernel"), B.last_kernel()
    assert (dstatus.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)
    back, bstatus = O.ans_decode_batch(want[0], want[1], n_per, lo, cdfs, P, 32, 64)      # (the oracle's own round trip)
    assert (bstatus == 0).all() and np.array_equal(back, sym)


@pytest.mark.parametrize("case", ["bimodal", "alternating_small", "uniform", "n_2_to_P"])
def test_the_other_forms(B, O, case):
    """jump points (the checkpointing encoder, the sub-lane decoder), an int8 symbol matrix, the symbol-major layout and packed words,
    once each at (130, 100)"""
    n_streams, n_per = 130, 100
    lo, P, cdfs, sym = batch(O, case, n_streams, n_per)
    cfg = (32, 64, P)
    model = B.Model.from_cdf_rows_per_stream(cdfs, lo, P)                   # (a numpy array this time)
    want = O.ans_encode_batch(sym, lo, cdfs, P, 32, 64)
    compact_rows = CASES[case][2] == "pt"

    if compact_rows:        # (jump points for tables per stream are noted by the compact-row encoder alone: cst_ans_encode_batch_ckpt)
        enc = B.ans_encode(dev(sym), model, cfg, jump_points=2)
        assert enc.jump is not None
        assert ALT or B.last_kernel() == with_jump("ans_encode_pt_kernel", enc), B.last_kernel()
        assert_words(enc, *want)
        pos, state = O.ans_jump_table(sym, lo, cdfs, P, n_per // 2)
        assert np.array_equal(enc.jump.pos.cpu().numpy().view(np.uint32), pos)
        assert np.array_equal(enc.jump.state.cpu().numpy().view(np.uint64), state)
        dec, st = B.ans_decode(enc, model, n_per)
        assert ALT or B.last_kernel() == "ans_decode_pt_sub_kernel", B.last_kernel()
        assert int(st.abs().sum()) == 0 and np.array_equal(dec.cpu().numpy(), sym)

    if lo >= -128 and lo + cdfs.shape[1] - 2 <= 127:
        narrow = dev(sym.astype(np.int8))
        enc8 = B.ans_encode(narrow, model, cfg)
        assert_words(enc8, *want)
        dec8, st = B.ans_decode(enc8, model, n_per, dtype=torch.int8)
        assert dec8.dtype == torch.int8 and int(st.abs().sum()) == 0 and torch.equal(dec8, narrow)

    encT = B.ans_encode(dev(sym.T), model, cfg, "symbol_major")
    assert_words(encT, *want)
    decT, st = B.ans_decode(encT, model, n_per, "symbol_major")
    assert int(st.abs().sum()) == 0 and np.array_equal(decT.cpu().numpy().T, sym)

    plain = B.ans_encode(dev(sym), model, cfg, jump_points=0)
    packed, offsets = B.compact(plain)
    decP, st = B.ans_decode((packed, plain.n_words), model, n_per, offsets=offsets, config=cfg)
    assert int(st.abs().sum()) == 0 and np.array_equal(decP.cpu().numpy(), sym)


@pytest.mark.parametrize("cfg", [(32, 64, 12), (16, 32, 12), (32, 64, 16)], ids=lambda c: "W%dS%dP%d" % c)
def test_gaussian_rows_give_the_gaussian_models_words(B, cfg):
    """a model rebuilt from a Gaussian per-stream model's rows is that model: the same words, bit for bit, from the same kernels"""
    n_streams, n_per, P = 130, 100, cfg[2]
    rng = np.random.default_rng(P)
    mu, sigma = rng.uniform(-10, 10, n_streams), np.exp(rng.uniform(np.log(0.5), np.log(16), n_streams))
    g = B.Model.quantized_gaussian_per_stream(-127, 127, dev(mu), dev(sigma), P)
    m = B.Model.from_cdf_rows_per_stream(g.cdfs_device(), -127, P)
    assert torch.equal(m.cdfs_device(), g.cdfs_device())
    sym = torch.clamp(torch.round(torch.randn((n_streams, n_per), device="cuda", dtype=torch.float64) * dev(sigma)[:, None] + dev(mu)[:, None]),
                      -127, 127).to(torch.int32)
    eg = B.ans_encode(sym, g, cfg, jump_points=0)
    kernel = B.last_kernel()
    em = B.ans_encode(sym, m, cfg, jump_points=0)
    assert B.last_kernel() == kernel
    assert int(eg.status.abs().sum()) == 0 and torch.equal(em.status, eg.status) and torch.equal(em.n_words, eg.n_words)
    wg, ng, _ = eg.to_numpy()
    wm, _, _ = em.to_numpy()
    for s in range(n_streams):
        assert np.array_equal(wm[s, : ng[s]], wg[s, : ng[s]]), f"stream {s}"
    dg, _ = B.ans_decode(eg, m, n_per)                     # each decodes the other's words
    dm, _ = B.ans_decode(em, g, n_per)
    assert torch.equal(dg, sym) and torch.equal(dm, sym)


def test_fit_per_stream_end_to_end(B):
    """the encoder fits and codes; the decoder has the rows alone"""
    rng = np.random.default_rng(5)
    n_streams, n_per, lo, hi, P = 130, 100, -127, 127, 12
    mu, sigma = rng.uniform(-60, 60, (n_streams, 1)), np.exp(rng.uniform(np.log(0.3), np.log(30), (n_streams, 1)))
    sym_np = np.clip(np.round(rng.normal(mu, sigma, (n_streams, n_per))), lo, hi).astype(np.int32)
    sym_np[7] = 5                                           # a stream of one symbol
    sym = dev(sym_np)
    model = B.Model.fit_per_stream(sym, lo, hi, P)
    enc = B.ans_encode(sym, model, (32, 64, P))
    assert int(enc.status.abs().sum()) == 0
    rows = model.cdfs_device().clone()
    enc.jump = None                                         # (the words alone travel)
    rebuilt = B.Model.from_cdf_rows_per_stream(rows, lo, P)
    dec, st = B.ans_decode(enc, rebuilt, n_per)
    assert int(st.abs().sum()) == 0 and torch.equal(dec, sym)
    # fitted tables are shorter than a table that knows nothing: fewer words than the uniform rows would take
    uniform = B.Model.from_cdf_rows_per_stream(B.fit_cdf_rows(torch.zeros((n_streams, hi - lo + 1), dtype=torch.int32, device="cuda"), P), lo, P)
    assert int(enc.n_words.sum()) < int(B.ans_encode(sym, uniform, (32, 64, P)).n_words.sum())


def test_table_set_fit_end_to_end(B):
    rng = np.random.default_rng(6)
    n_streams, n_per, lo, hi, P, K = 130, 100, -30, 33, 12, 64
    idx_np = rng.integers(0, K - 1, (n_streams, n_per)).astype(np.uint8)          # class K - 1 is named by nobody
    sym_np = np.clip(np.round(rng.normal(idx_np.astype(np.float64) - 30, 1 + idx_np % 5)), lo, hi).astype(np.int32)
    sym, idx = dev(sym_np), dev(idx_np)
    tables = B.TableSet.fit(sym, idx, K, lo, hi, P)
    assert tables.n_tables == K
    enc = B.ans_encode_indexed(sym, idx, tables, (32, 64, P))
    assert int(enc.status.abs().sum()) == 0
    rebuilt = B.TableSet.from_cdfs(tables.cdfs(), lo, P)
    dec, st = B.ans_decode_indexed(enc, idx, rebuilt, n_per)
    assert int(st.abs().sum()) == 0 and torch.equal(dec, sym)


def test_invalid_device_rows_are_refused(B):
    good = cdfs_of(rest_on(5, 9, 12, np.array([0, 3, 8, 4, 4])))
    B.Model.from_cdf_rows_per_stream(dev(good.view(np.int32)), 0, 12)
    for row, col, value in ((2, 4, None), (4, 9, 4095), (1, 9, 4097), (3, 0, 1), (0, 9, 0)):
        bad = good.copy()                                   # a zero probability, last entry not 2^P (twice), cdf[0] != 0, a wrapped end
        bad[row, col] = bad[row, col - 1] if value is None else value
        with pytest.raises(ValueError):
            B.Model.from_cdf_rows_per_stream(dev(bad.view(np.int32)), 0, 12)
    decreasing = good.copy()
    decreasing[3, 5], decreasing[3, 6] = good[3, 6], good[3, 5]
    with pytest.raises(ValueError):
        B.Model.from_cdf_rows_per_stream(dev(decreasing.view(np.int32)), 0, 12)
