"""GPU tests of Categorical(perfect=True) quantised on the device (csrc/cst_categorical_perfect.hip): the rows
kernel, the four batched coder calls of `batched.*_categorical(..., perfect=True)` and the drop-in coders that use them.

Every expected row comes from the CPU: the library's sorted-vector host function cst_categorical_perfect_cdf AND the oracle's
restatement oracle.categorical_perfect_cdf; every expected word from one oracle coder per stream over the oracle's rows.  Move
counts come from the host form of the kernel's formulation, which tests/test_categorical_perfect_cpu.py ties to a line-by-line
restatement of the reference.  Bad rows are data errors the kernel reports in-band: nothing here can fault."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import categorical_perfect_rows as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KERNEL = "categorical_perfect_kernel"
# (n_streams, n_per_stream, K, dtype): K = 300 takes the piece decoder, the others decode_rows_wave_kernel
CODER_CASES = [(3, 40, 5, "f32"), (70, 33, 64, "f64"), (1, 300, 300, "f32")]
CONFIGS = [(32, 64, 24), (16, 32, 12)]


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


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native
    return _native.load_library()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def device_rows(lib, probs, P):
    """cst_categorical_perfect_cdf_rows through the raw entry point: (rows, codes, moves), nothing raised for a bad row"""
    n, k = probs.shape
    d_probs = dev(probs)
    rows = torch.zeros((n, k + 1), dtype=torch.int32, device="cuda")
    bad = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    moves = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = lib.cst_categorical_perfect_cdf_rows(P, _ptr(d_probs), probs.itemsize, n, k, _ptr(rows), _ptr(bad), _ptr(moves), None)
    assert rc == 0
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint32), bad.cpu().numpy(), moves.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.ROW_CASES, ids=R.case_id)
def test_rows_equal_the_host_function_and_the_oracle(B, O, lib, case):
    k, n, P, _ = case
    probs = R.case_rows(case)
    rows, moves = B.categorical_cdf_rows(dev(probs), P, perfect=True, return_moves=True)        # (raises for a code 1 or 2)
    torch.cuda.synchronize()
    assert B.last_kernel() == KERNEL
    assert tuple(rows.shape) == (n, k + 1) and tuple(moves.shape) == (n,)
    rows, moves = rows.cpu().numpy().view(np.uint32), moves.cpu().numpy().view(np.uint32)
    _, codes, want_moves = R.host_perfect(lib, probs, P)
    assert (codes == 0).all()
    for r in range(n):
        rc, want = R.sorted_vector_perfect(lib, probs[r], P)
        assert rc == 0 and rows[r].tolist() == want.tolist(), r
        assert rows[r].tolist() == O.categorical_perfect_cdf(probs[r], P).tolist(), r
    print(f"{R.case_id(case)}: moves max {int(moves.max())} mean {moves.mean():.2f} (cap {R.move_cap(k)})")
    assert moves.tolist() == want_moves.tolist()
    assert int(moves.max()) < R.move_cap(k) // 4


def test_rows_keep_the_leading_axes(B, lib):
    probs = R.make_rows(6 * 11, 65, np.float32, 5).reshape(6, 11, 65)
    rows = B.categorical_cdf_rows(dev(probs), 24, perfect=True)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (6, 11, 66)
    want, _, _ = R.host_perfect(lib, probs.reshape(66, 65), 24)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32).reshape(66, 66), want)
    assert B.categorical_cdf_rows(dev(probs[:0]), 24, perfect=True).shape == (0, 11, 66)


@pytest.mark.parametrize("k", [7, 300])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_bad_rows_are_flagged_where_the_host_refuses_and_neighbours_stand(B, lib, dtype, k):
    from constriction_amd import _native as N
    P, n = 24, 70
    probs = R.make_rows(n, k, R.DTYPES[dtype], 13 * k)
    spoiled = {4: "negative", 5: "nan", 31: "inf", 63: "zeros", 64: "nan", 69: "negative"}
    for r, what in spoiled.items():
        if what == "negative":
            probs[r, k // 2] = -0.25
        elif what == "nan":
            probs[r, k - 1] = np.nan
        elif what == "inf":
            probs[r, 0] = np.inf
        else:
            probs[r, :] = 0.0
    rows, codes, moves = device_rows(lib, probs, P)
    for r in range(n):
        rc, want = R.sorted_vector_perfect(lib, probs[r], P)
        assert (rc == N.CST_ERR_MODEL) == (r in spoiled) and rc in (0, N.CST_ERR_MODEL), r
        assert codes[r] == (1 if r in spoiled else 0), r
        if r in spoiled:
            assert rows[r].tolist() == [0xFFFFFFFF] + [1 << P] * k and moves[r] == 0, r
        else:
            assert rows[r].tolist() == want.tolist(), r
    with pytest.raises(ValueError, match="not normalizable"):
        B.categorical_cdf_rows(dev(probs), P, perfect=True)


def _weights(cdf, P):
    return np.diff(cdf.astype(np.int64))


def _kl(weights, hist, P):
    hist = np.asarray(hist, dtype=np.float64)
    assert int(weights.sum()) == 1 << P and (weights > 0).all()
    p = hist / hist.sum()
    nz = p > 0
    return float(np.sum(p[nz] * (np.log2(p[nz]) - np.log2(weights[nz].astype(np.float64)))) + P)


@pytest.mark.parametrize("vec", json.loads((Path(__file__).parent / "golden" / "perfect_categorical.json").read_text())["vectors"],
                         ids=lambda v: v["id"])
def test_reference_known_answers_through_the_device(B, O, vec):
    """tests/golden/perfect_categorical.json (the reference's own unit tests, contiguous.rs:709-873) at the precisions the device
    call takes (P <= 31; a vector given for P = 32 runs at 31 and 24): the device row is the oracle's row, and what the reference
    asserts about it holds"""
    dtype = np.float32 if vec["dtype"] == "f32" else np.float64
    values = np.array(vec["hist"] if "hist" in vec else vec["probs"], dtype=np.float64).astype(dtype)
    precisions = sorted({min(p, 31) for p in vec.get("precisions", [vec.get("precision", 24)])} | {24})
    for P in precisions:
        row = B.categorical_cdf_rows(dev(values[None, :]), P, perfect=True)[0].cpu().numpy().view(np.uint32)
        assert row.tolist() == O.categorical_perfect_cdf(values, P).tolist(), P
        w = _weights(row, P)
        if vec["expect"] == "weights_equal_hist":
            # the histogram sums to 2^32: at P bits the optimum keeps its proportions (to within the rounding of a unit)
            assert np.abs(w * float(1 << (32 - P)) - values.astype(np.float64)).max() <= float(1 << (32 - P))
        elif vec["expect"] == "kl_perfect_below_kl_fast":
            assert _kl(w, values, P) < _kl(_weights(O.categorical_fast_cdf(values, P), P), values, P) < vec["kl_tolerance"]
        else:
            if vec["expect"].endswith("within_1"):
                assert -1 <= int(w[0]) - int(w[2]) <= 1
            assert _kl(w, values, P) < vec["kl_tolerance"]


# ---------------------------------------------------------------------------------------------------------------------
# coders
# ---------------------------------------------------------------------------------------------------------------------

def workload(case, P):
    n_streams, n_per, k, dtype = case
    probs = R.make_rows(n_streams * n_per, k, R.DTYPES[dtype], 101 * k + P).reshape(n_streams, n_per, k)
    rng = np.random.default_rng(k + P)
    sym = rng.integers(0, k, (n_streams, n_per)).astype(np.int32)
    sym[:, 0], sym[:, 1] = 0, k - 1
    return sym, probs


def oracle_words(O, coder, cfg, sym, models):
    W, S, P = cfg
    if coder == "ans":
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return c.get_compressed()


_expected = {}


def expected(O, case, coder, cfg):
    """(symbols, probabilities, the oracle's perfect rows [n_streams, n_per, K + 1], the oracle coder's words per stream) -- computed
    once and shared"""
    mkey = (case, cfg[2])
    if mkey not in _expected:
        sym, probs = workload(case, cfg[2])
        rows = np.stack([np.stack([O.categorical_perfect_cdf(row, cfg[2]) for row in stream]) for stream in probs])
        _expected[mkey] = (sym, probs, rows)
    sym, probs, rows = _expected[mkey]
    key = (case, coder, cfg)
    if key not in _expected:
        _expected[key] = [oracle_words(O, coder, cfg, sym[s], [O.TableModel(r, 0, cfg[2]) for r in rows[s]]) for s in range(case[0])]
    return sym, probs, rows, _expected[key]


def in_layout(layout, *arrays):
    if layout == "symbol_major":
        return [dev(np.swapaxes(a, 0, 1)) for a in arrays]
    return [dev(a) for a in arrays]


def tabulated_route(B, coder, cfg, layout, d_sym, d_probs, n_streams, n_per, k):
    """the route that existed before: device rows (perfect=True), (left, probability) gathered from them, cst_*_encode_cp_batch; then
    cst_*_decode_rows_batch over the same rows.  Returns (words, n_words, decoded symbols)."""
    from constriction_amd import _native as N
    L = N.lib()
    lay = N.LAYOUT_SYMBOL_MAJOR if layout == "symbol_major" else N.LAYOUT_STREAM_MAJOR
    rows = B.categorical_cdf_rows(d_probs, cfg[2], perfect=True).view(-1, k + 1).to(torch.int64) & 0xFFFFFFFF
    flat = d_sym.reshape(-1).to(torch.int64)
    left = rows.gather(1, flat[:, None])[:, 0]
    prob = rows.gather(1, flat[:, None] + 1)[:, 0] - left
    d_left, d_prob = left.to(torch.int32).contiguous(), prob.to(torch.int32).contiguous()
    d_rows = rows.to(torch.int32).contiguous()
    stride = (B.max_words if coder == "ans" else B.range_max_words)(n_per, cfg)
    words = torch.zeros((n_streams, stride), dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(d_sym)
    c = N.CoderConfig(*cfg)
    N.check(getattr(L, f"cst_{coder}_encode_cp_batch")(c, _ptr(d_left), _ptr(d_prob), n_streams, n_per, lay, _ptr(words), stride, _ptr(n_words), None,
                                                       _ptr(status), N.FLAG_NONE, None), "cp")
    assert (status.cpu().numpy() == 0).all()
    if coder == "ans":
        N.check(L.cst_ans_decode_rows_batch(c, _ptr(words), None, stride, words.numel(), _ptr(n_words), _ptr(d_rows), k, 0, _ptr(out), n_streams, n_per,
                                            lay, None, None, _ptr(status), N.FLAG_NONE, None), "rows")
    else:
        N.check(L.cst_range_decode_rows_batch(c, _ptr(words), None, stride, words.numel(), _ptr(n_words), _ptr(d_rows), k, 0, _ptr(out), n_streams, n_per,
                                              lay, None, _ptr(status), N.FLAG_NONE, None), "rows")
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    return words.cpu().numpy().view(np.uint32), n_words.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "W%dS%dP%d" % c)
@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case", CODER_CASES, ids=lambda c: "%dx%dxK%d_%s" % c)
def test_coder_parity(B, O, case, coder, cfg):
    n_streams, n_per, k, _ = case
    sym, probs, _, want = expected(O, case, coder, cfg)
    for layout in ("stream_major", "symbol_major"):
        d_sym, d_probs = in_layout(layout, sym, probs)
        enc = getattr(B, f"{coder}_encode_categorical")(d_sym, d_probs, cfg, layout, perfect=True)
        torch.cuda.synchronize()
        assert B.last_kernel() == f"{coder}_encode_categorical_perfect_two_pass"
        words, n_words, status = enc.to_numpy()
        assert (status == 0).all()
        assert n_words.tolist() == [len(w) for w in want]
        for s in range(n_streams):
            assert words[s, : n_words[s]].tolist() == want[s].tolist(), f"stream {s} ({layout})"
        dec, dstatus = getattr(B, f"{coder}_decode_categorical")(enc, d_probs, layout, perfect=True)
        torch.cuda.synchronize()
        assert B.last_kernel() == "decode_categorical_perfect_by_rows"
        assert (dstatus.cpu().numpy() == 0).all(), layout
        got = dec.cpu().numpy()
        assert np.array_equal(got.T if layout == "symbol_major" else got, sym), layout
        # the tabulated device route gives the same words and symbols
        t_words, t_n, t_sym = tabulated_route(B, coder, cfg, layout, d_sym, d_probs, n_streams, n_per, k)
        assert t_n.tolist() == n_words.tolist()
        for s in range(n_streams):
            assert t_words[s, : t_n[s]].tolist() == want[s].tolist(), f"tabulated, stream {s} ({layout})"
        assert np.array_equal(t_sym, d_sym.cpu().numpy())


@pytest.mark.parametrize("coder", ["ans", "range"])
def test_a_compacted_batch_decodes(B, O, coder):
    case, cfg = CODER_CASES[1], (32, 64, 24)
    sym, probs, _, want = expected(O, case, coder, cfg)
    enc = getattr(B, f"{coder}_encode_categorical")(dev(sym), dev(probs), cfg, perfect=True)
    packed, offsets = B.compact(enc)
    torch.cuda.synchronize()
    assert int(offsets[-1]) == sum(len(w) for w in want)
    dec, st = getattr(B, f"{coder}_decode_categorical")((packed, enc.n_words), dev(probs), offsets=offsets, config=cfg, perfect=True)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


@pytest.mark.parametrize("case", CODER_CASES[1:], ids=lambda c: "%dx%dxK%d_%s" % c)
@pytest.mark.parametrize("coder", ["ans", "range"])
def test_failures_stay_in_their_stream(B, O, coder, case):
    """a bad row and a symbol equal to K give CST_STREAM_IMPOSSIBLE_SYMBOL for their stream only; the neighbours keep the oracle's
    words and decode (the one-stream case: the call reports it and writes no words for it)"""
    cfg = (32, 64, 24)
    n_streams, n_per, k, _ = case
    sym, probs, _, want = expected(O, case, coder, cfg)
    bad_p, bad_s = probs.copy(), sym.copy()
    row_stream, sym_stream = (0, None) if n_streams == 1 else (11, 40)
    bad_p[row_stream, n_per // 2, k // 3] = np.nan
    if sym_stream is not None:
        bad_s[sym_stream, n_per - 1] = k
    failing = [s for s in (row_stream, sym_stream) if s is not None]
    enc = getattr(B, f"{coder}_encode_categorical")(dev(bad_s), dev(bad_p), cfg, perfect=True)
    torch.cuda.synchronize()
    words, n_words, status = enc.to_numpy()
    assert status[failing].tolist() == [1] * len(failing) and (np.delete(status, failing) == 0).all()
    for s in range(n_streams):
        if s not in failing:
            assert words[s, : n_words[s]].tolist() == want[s].tolist(), s
    good = getattr(B, f"{coder}_encode_categorical")(dev(sym), dev(probs), cfg, perfect=True)
    dec, st = getattr(B, f"{coder}_decode_categorical")(good, dev(bad_p), perfect=True)
    torch.cuda.synchronize()
    st, got = st.cpu().numpy(), dec.cpu().numpy()
    assert st[row_stream] == 1 and (np.delete(st, row_stream) == 0).all()
    assert np.array_equal(np.delete(got, row_stream, axis=0), np.delete(sym, row_stream, axis=0))
    if coder == "range":                    # what was decoded in front of the bad row stands (ANS decodes from the front too)
        assert np.array_equal(got[row_stream, : n_per // 2], sym[row_stream, : n_per // 2])


def test_arguments_are_checked(B):
    sym, probs = workload(CODER_CASES[0], 24)
    with pytest.raises(ValueError, match="shape of the symbol matrix"):
        B.ans_encode_categorical(dev(sym), dev(probs[:, :5]), perfect=True)
    with pytest.raises(TypeError):
        B.range_encode_categorical(dev(sym), dev(probs.astype(np.float16)), perfect=True)
    with pytest.raises(ValueError, match="2 <= K"):
        B.range_encode_categorical(dev(sym), dev(probs[..., :1]), perfect=True)
    with pytest.raises(ValueError, match="1024"):
        B.ans_encode_categorical(dev(sym), dev(np.ones((3, 40, 1025), np.float32)), perfect=True)
    enc = B.ans_encode_categorical(dev(sym), dev(probs), perfect=True)
    with pytest.raises(ValueError):
        B.ans_decode_categorical(enc, dev(probs[:2]), perfect=True)


# ---------------------------------------------------------------------------------------------------------------------
# drop-in coders
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("which", ["categorical_f32", "categorical_f64", "bernoulli"])
def test_drop_in(B, which, coder, monkeypatch):
    """stream.stack.AnsCoder and the queue pair with Categorical(perfect=True) / Bernoulli(perfect=True) and per-symbol parameters
    quantise on the device and produce the words of the host route (family_rows, coded through the "rows" kind)"""
    import constriction_amd
    from constriction_amd import stream  # noqa: F401
    mod, stack, queue, single = (constriction_amd.stream.model, constriction_amd.stream.stack, constriction_amd.stream.queue,
                                 constriction_amd.stream._single)
    rng = np.random.default_rng(41)
    n = 400
    if which == "bernoulli":
        ps = rng.uniform(0.0, 1.0, n)
        ps[:2] = (0.0, 1.0)
        sym = (rng.random(n) < ps).astype(np.int32)
        model, params = mod.Bernoulli(perfect=True), ps
    else:
        k, dtype = (300, np.float32) if which == "categorical_f32" else (12, np.float64)
        params = R.make_rows(n, k, dtype, 77)
        sym = rng.integers(0, k, n).astype(np.int32)              # (an entry that is exactly 0 still gets its unit of weight)
        model = mod.Categorical(perfect=True)
    assert single.model_args(model, (params,), families=True, device_perfect=True)[0] == "categorical_perfect"

    def run():
        if coder == "ans":
            enc = stack.AnsCoder()
            enc.encode_reverse(sym, model, params)
            return enc.get_compressed(), stack.AnsCoder
        enc = queue.RangeEncoder()
        enc.encode(sym, model, params)
        return enc.get_compressed(), queue.RangeDecoder

    words, decoder = run()
    assert B.last_kernel() == f"{coder}_encode_categorical_perfect_two_pass"
    dec = decoder(words)
    a = dec.decode(model, params[:151])
    assert B.last_kernel() == "decode_categorical_perfect_by_rows"
    b = dec.decode(model, params[151:])
    assert np.array_equal(np.concatenate([a, b]), sym)
    # the host route: the classification without device_perfect -- family_rows on the host, coded through the "rows" kind
    classify = single.model_args
    monkeypatch.setattr(single, "model_args", lambda m, p, n_expected=None, families=False, device_perfect=False: classify(m, p, n_expected, families))
    assert single.model_args(model, (params,), families=True, device_perfect=True)[0] == "rows"
    want, _ = run()
    assert words.tolist() == want.tolist()
    assert np.array_equal(decoder(want).decode(model, params), sym)
