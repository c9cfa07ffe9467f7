"""GPU tests of what the helper waves of the producer / consumer encoder (cst_ans_pc.hip) took over from the coder waves in round 7:
the loader stages TABLE ADDRESSES (symbols clamped into the model's support) and keeps the range check of every row it stages; at the
end the 8 lanes that hold a row reduce it and write the row's largest raw table index to the hand-off area.  Impossible symbols in
every position a lane, a row block or a tile can put them, streams at the maximum word rate, slabs that are too small, the partial
workgroup and the first (combined) helper form: words, counts and status against the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ALT = any(os.environ.get(k) for k in ("CST_NO_PC_ENCODER", "CST_SMALL_KERNELS", "CST_PC_COMBINED", "CST_NO_PC_WIDE"))    # (A/B runs: scripts/alt_paths.sh)


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


def dev(a):
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert d.data_ptr() % 128 == 0          # (the kernel takes rows that are whole 128-byte aligned tiles)
    return d


def _encode(B, model, sym, P, stride):
    """cst_ans_encode_batch into slabs of `stride` words, with a guard region behind the last slab"""
    from constriction_amd import _native as N
    n_streams, n_per = sym.shape
    words = torch.full((n_streams * stride + 4096,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    d = dev(sym)
    N.check(N.lib().cst_ans_encode_batch(model._h, N.CoderConfig(32, 64, P), C.c_void_p(d.data_ptr()), n_streams, n_per, 0,
                                         C.c_void_p(words.data_ptr()), stride, C.c_void_p(n_words.data_ptr()), None,
                                         C.c_void_p(status.data_ptr()), 0, None), "cst_ans_encode_batch")
    torch.cuda.synchronize()
    if not ALT:
        assert B.last_kernel().startswith("ans_encode_pc_kernel")
    w = words.cpu().numpy().view(np.uint32)
    assert (w[n_streams * stride:] == 0x5A5A5A5A).all(), "words were written behind the last slab"
    return w[: n_streams * stride].reshape(n_streams, stride), n_words.cpu().numpy(), status.cpu().numpy()


def _check(O, sym, lo, cdf, P, words, n_words, status, stride):
    want_words, want_n, want_status = O.ans_encode_batch(sym, lo, cdf, P)
    want_status = np.where((want_status == 0) & (want_n > stride), 2, want_status)      # CST_STREAM_CAPACITY
    assert status.tolist() == want_status.tolist()
    ok = status == 0
    assert n_words[ok].tolist() == want_n[ok].tolist() and (n_words[~ok] == 0).all()
    for s in np.flatnonzero(ok):
        assert words[s, : n_words[s]].tolist() == want_words[s, : want_n[s]].tolist(), s
    return want_status


def _gauss(B, O, P, lo=-60, hi=60):
    cdf = O.GaussianModel(lo, hi, 2.5, 7.0, P, 32).cdf_table()
    return cdf, B.Model.from_cdf(cdf, lo, P)


def _impossible(rng, sym, lo, hi):
    """impossible symbols in the first, a middle and the last tile, at the first and the last step of a tile, in rows of every
    row block k = (lane / 8) and of both coder waves of a loader; values just outside the support and far away"""
    n_streams, n_per = sym.shape
    tiles = n_per // 32
    bad = {}
    values = [hi + 1, lo - 1, 2 ** 31 - 1, -2 ** 31, hi + 2 ** 28, lo - 2 ** 28, 2 ** 30]
    positions = [0, 31, 32 * (tiles // 2), 32 * (tiles // 2) + 31, n_per - 32, n_per - 1]
    for j, s in enumerate(range(1, n_streams, 7)):
        if j % 3 == 2:
            continue                                     # (some rows stay clean between flagged ones)
        pos = positions[j % len(positions)]
        sym[s, pos] = values[j % len(values)]
        bad[s] = pos
    return sorted(bad)


@pytest.mark.parametrize("P", [12, 24])
@pytest.mark.parametrize("n_streams,n_per", [(256, 128), (512, 96), (300, 160)])
def test_impossible_symbols_in_every_position(B, O, P, n_streams, n_per):
    lo, hi = -60, 60
    cdf, model = _gauss(B, O, P, lo, hi)
    rng = np.random.default_rng(P * 1000 + n_streams)
    sym = O.synth_symbols(0x5EED + P, 0, n_streams, n_per, lo, cdf, P)
    flagged = _impossible(rng, sym, lo, hi)
    stride = B.max_words(n_per, (32, 64, P))
    words, n_words, status = _encode(B, model, sym, P, stride)
    want = _check(O, sym, lo, cdf, P, words, n_words, status, stride)
    assert np.flatnonzero(want == 1).tolist() == flagged


@pytest.mark.parametrize("lo", [-2 ** 31, 2 ** 31 - 101, 0])
def test_support_at_the_ends_of_int32(B, O, lo):
    """a support that touches INT32_MIN or INT32_MAX: the loader's clamp and the (unsigned) largest table index must not wrap"""
    P, n = 12, 101
    hi = lo + n - 1
    cdf = O.GaussianModel(lo, hi, lo + 50.5, 9.0, P, 32).cdf_table()
    model = B.Model.from_cdf(cdf, lo, P)
    n_streams, n_per = 256, 64
    sym = O.synth_symbols(0xE17D, 0, n_streams, n_per, lo, cdf, P)
    far = [v for v in (-2 ** 31, 2 ** 31 - 1, lo - 1, hi + 1, lo + 2 ** 31 - 1, lo - 2 ** 31, 0) if -2 ** 31 <= v < 2 ** 31 and not lo <= v <= hi]
    for j, s in enumerate(range(3, n_streams, 11)):
        sym[s, (5 * j) % n_per] = far[j % len(far)]
    stride = B.max_words(n_per, (32, 64, P))
    words, n_words, status = _encode(B, model, sym, P, stride)
    want = _check(O, sym, lo, cdf, P, words, n_words, status, stride)
    assert (want == 1).sum() == len(range(3, n_streams, 11))


def spiky_cdf(n, P):
    """symbol 0 takes everything the n - 1 others (probability 2^-P each) leave"""
    cdf = np.zeros(n + 1, np.uint32)
    cdf[1] = (1 << P) - (n - 1)
    cdf[2:] = cdf[1] + np.arange(1, n, dtype=np.uint32)
    return cdf


@pytest.mark.parametrize("P", [8, 12, 24])
def test_maximum_word_rate(B, O, P):
    """every symbol costs P bits (the most a symbol can cost): the streams emit as many words per tile as they can, with an
    impossible symbol at the first and the last step of a tile in some of them"""
    n = 101
    cdf = spiky_cdf(n, P)
    model = B.Model.from_cdf(cdf, 0, P)
    n_streams, n_per = 512, 256
    rng = np.random.default_rng(P)
    sym = rng.integers(1, n, (n_streams, n_per), dtype=np.int32)
    sym[7, 32] = n
    sym[130, 63] = -1
    sym[511, n_per - 1] = n + 1000
    stride = B.max_words(n_per, (32, 64, P))
    words, n_words, status = _encode(B, model, sym, P, stride)
    want = _check(O, sym, 0, cdf, P, words, n_words, status, stride)
    assert np.flatnonzero(want).tolist() == [7, 130, 511]
    assert n_words.max() >= (n_per * P) // 32 - 1


@pytest.mark.parametrize("P", [12, 24])
def test_slabs_that_are_too_small(B, O, P):
    """slabs of 16 words, and slabs that some streams of the batch fit and others do not; a stream with an impossible symbol
    reports that whatever its slab"""
    lo, hi = -60, 60
    cdf, model = _gauss(B, O, P, lo, hi)
    n_streams, n_per = 512, 256
    sym = O.synth_symbols(0x51AB + P, 0, n_streams, n_per, lo, cdf, P)
    sym[1::4] = hi                                       # (the tail of the support: ~P bits per symbol, more words than 64)
    sym[0, 0] = hi + 1
    sym[300, n_per - 1] = lo - 1
    mid = 64
    for stride in (16, mid):
        words, n_words, status = _encode(B, model, sym, P, stride)
        want = _check(O, sym, lo, cdf, P, words, n_words, status, stride)
        assert want[0] == 1 and want[300] == 1
        if stride == mid:
            assert (want == 0).any() and (want == 2).any()
        else:
            assert (want[want != 1] == 2).all()


def test_combined_helper_form(B, O):
    """CST_PC_COMBINED=1: every helper wave loads, stages (addresses, range check) and flushes for its own coder wave"""
    from constriction_amd import _native
    lo, hi = -60, 60
    P = 12
    cdf, model = _gauss(B, O, P, lo, hi)
    n_streams, n_per = 512, 192
    sym = O.synth_symbols(0xC0B, 0, n_streams, n_per, lo, cdf, P)
    flagged = _impossible(np.random.default_rng(1), sym, lo, hi)
    stride = B.max_words(n_per, (32, 64, P))
    os.environ["CST_PC_COMBINED"] = "1"
    _native.reload_knobs()
    try:
        words, n_words, status = _encode(B, model, sym, P, stride)
    finally:
        del os.environ["CST_PC_COMBINED"]
        _native.reload_knobs()
    want = _check(O, sym, lo, cdf, P, words, n_words, status, stride)
    assert np.flatnonzero(want == 1).tolist() == flagged
