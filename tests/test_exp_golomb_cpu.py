"""CPU-only: the plain-Python restatement of the Exponential-Golomb code (tests/exp_golomb_ref.py) against the reference's known
answers (tests/golden/exp_golomb_vectors.json), and the host side of the cst_exp_golomb_* entry points: the slab bound and every
argument error, which must be reported before a device is touched (there is none here)."""
import json
from pathlib import Path

import numpy as np
import pytest

import exp_golomb_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "exp_golomb_vectors.json").read_text())
STACK, QUEUE = 0, 1
INVALID = -1     # CST_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native, build
    build.build_library()
    assert _native.CST_ERR_INVALID_ARGUMENT == INVALID
    return _native.load_library()


def test_explicit_examples_in_both_bit_orders():
    assert len(GOLDEN["explicit_examples"]) == 11
    for case in GOLDEN["explicit_examples"]:
        assert R.prefix_codeword(case["symbol"], 32) == case["bits"], case
        assert R.suffix_codeword(case["symbol"], 32) == case["bits"][::-1], case
        assert R.decode_symbol(case["bits"], 0, 32) == (case["symbol"], len(case["bits"]))


def test_doc_example():
    d = GOLDEN["doc_example"]
    words, n_bits = R.queue_encode(d["symbols"], d["bits"])
    assert R.read_bits(words, "queue") == d["queue_bit_string"] and n_bits == 16
    assert R.decode(words, 4, "queue", d["bits"]) == (d["symbols"], True, 16)


@pytest.mark.parametrize("case", GOLDEN["known_answers"], ids=lambda c: f"{c['semantics']}-u{c['bits']}-{c['symbols'][0]}x{len(c['symbols'])}")
def test_known_answers(case):
    enc = R.stack_encode if case["semantics"] == "stack" else R.queue_encode
    assert enc(case["symbols"], case["bits"]) == (case["words"], case["n_bits"])
    symbols, ok, left = R.decode(case["words"], len(case["symbols"]), case["semantics"], case["bits"])
    assert ok and symbols == case["symbols"]
    assert left == (0 if case["semantics"] == "stack" else 32 * len(case["words"]) - case["n_bits"])


@pytest.mark.parametrize("bits", [8, 16, 32])
def test_widths_wrap_and_grow_where_they_should(bits):
    top = (1 << bits) - 1
    assert R.prefix_codeword(top, bits) == "0" * bits + "1" + "0" * bits
    assert R.prefix_codeword(top - 1, bits) == "0" * (bits - 1) + "1" * bits
    for k in range(1, bits + 1):
        for x in ((1 << k) - 2, (1 << k) - 1, (1 << k) & top):
            word = R.prefix_codeword(x, bits)
            assert R.decode_symbol(word, 0, bits) == (x, len(word))
            assert len(word) == (2 * bits + 1 if x == top else 2 * (x + 1).bit_length() - 1)


def test_round_trip_iid_queue_and_stack():
    """the shape of the reference's encode_decode_iid_queue / _stack: 1000 symbols rng % 8"""
    rng = np.random.default_rng(123)
    symbols = (rng.integers(0, 1 << 32, 1000) % 8).tolist()
    words, n_bits = R.queue_encode(symbols)
    decoded, ok, left = R.decode(words, 1000, "queue")
    assert ok and decoded == symbols and left == 32 * len(words) - n_bits < 32      # maybe_exhausted: only padding is left
    assert R.decode(words, 1001, "queue")[:2] == (symbols + [0], False)             # (reading on walks into the zero padding)
    words, n_bits = R.stack_encode(symbols)
    decoded, ok, left = R.decode(words, 1000, "stack")
    assert ok and decoded == symbols and left == 0                                  # is_empty
    assert len(words) == n_bits // 32 + 1


def test_the_four_invalid_codewords():
    for bits in (8, 32):
        assert R.decode_symbol("0" * 5, 0, bits) == (None, 0)                                   # the bits run out in the zero run
        assert R.decode_symbol("0" * (bits + 1) + "1" + "0" * 40, 0, bits) == (None, 0)         # len > B
        assert R.decode_symbol("0001" + "01", 0, bits) == (None, 0)                             # the bits run out within the value
        assert R.decode_symbol("0" * bits + "1" + "0" * (bits - 1) + "1", 0, bits) == (None, 0)  # len == B, value not zero
        assert R.decode_symbol("0" * bits + "1" + "0" * bits, 0, bits) == ((1 << bits) - 1, 2 * bits + 1)
    # a queue read past its last symbol walks into the zero padding; a stack without a seal is no stack
    assert R.decode([20740], 5, "queue") == ([3, 7, 0, 1, 0], False, 16)
    assert R.decode([], 1, "stack") == ([0], False, 0) and R.decode([5, 0], 1, "stack") == ([0], False, 0)


def test_max_words(lib):
    for symbol_bytes in (1, 2, 4):
        for semantics in (STACK, QUEUE):
            for n in (0, 1, 31, 32, 33, 100, 4096, 1 << 20):
                bits = n * (16 * symbol_bytes + 1) + 31 + 1       # every codeword 2 B + 1 bits, a continued call's 31 bits, the seal
                words = (bits + 31) // 32
                assert lib.cst_exp_golomb_max_words(n, symbol_bytes, semantics) == (words + 15) // 16 * 16
    for bad in (0, 3, 8, -1):
        assert lib.cst_exp_golomb_max_words(10, bad, STACK) == 0
    assert lib.cst_exp_golomb_max_words(10, 4, 2) == 0 and lib.cst_exp_golomb_max_words(10, 4, -1) == 0
    assert lib.cst_exp_golomb_max_words(2 ** 64 - 1, 4, STACK) == 0        # (the bound does not fit size_t)


P = 0x1000      # stands for a device pointer: an argument error returns before anything is read


def test_count_bits_argument_errors(lib):
    f = lib.cst_exp_golomb_count_bits
    assert f(P, 4, None, 3, 5, None, None) == INVALID
    assert f(None, 4, None, 3, 5, P, None) == INVALID
    assert f(None, 4, P, 3, 0, P, None) == INVALID
    for bad in (0, 3, 8):
        assert f(P, bad, None, 3, 5, P, None) == INVALID
    assert f(P, 4, None, 0, 5, P, None) == 0                 # no streams: nothing to do


def test_encode_batch_argument_errors(lib):
    f = lib.cst_exp_golomb_encode_batch
    ok = dict(semantics=STACK, sym=P, sb=4, n=3, per=5, words=P, stride=8, n_words=P, n_bits=P, cont=None, status=P)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["semantics"], a["sym"], a["sb"], a["n"], a["per"], a["words"], a["stride"], a["n_words"], a["n_bits"], a["cont"], a["status"], None)

    assert call(n=0) == 0
    for kw in (dict(sym=None), dict(words=None), dict(n_words=None), dict(status=None), dict(sb=0), dict(sb=3), dict(sb=8), dict(semantics=2),
               dict(semantics=-1)):
        assert call(**kw) == INVALID, kw
        assert call(n=0, **kw) == INVALID, kw                  # (before the count of streams is looked at)


def test_decode_batch_argument_errors(lib):
    f = lib.cst_exp_golomb_decode_batch
    ok = dict(semantics=QUEUE, words=P, offsets=None, stride=8, cap=24, n_words=P, sym=P, sb=1, n=3, per=5, cont=None, n_out=None, status=P)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["semantics"], a["words"], a["offsets"], a["stride"], a["cap"], a["n_words"], a["sym"], a["sb"], a["n"], a["per"], a["cont"],
                 a["n_out"], a["status"], None)

    assert call(n=0) == 0
    for kw in (dict(sym=None), dict(words=None), dict(words=None, stride=0, offsets=P), dict(n_words=None), dict(status=None), dict(sb=0),
               dict(sb=3), dict(semantics=2)):
        assert call(**kw) == INVALID, kw
        assert call(n=0, **kw) == INVALID, kw


def test_ragged_argument_errors(lib):
    enc, dec = lib.cst_exp_golomb_encode_ragged, lib.cst_exp_golomb_decode_ragged
    e_ok = dict(semantics=STACK, sym=P, sb=2, so=P, n=3, words=P, wo=P, stride=0, n_words=P, n_bits=None, status=P)
    d_ok = dict(semantics=STACK, words=P, wo=P, stride=0, cap=100, n_words=P, sym=P, sb=2, so=P, n=3, status=P)

    def e(**kw):
        a = dict(e_ok, **kw)
        return enc(a["semantics"], a["sym"], a["sb"], a["so"], a["n"], a["words"], a["wo"], a["stride"], a["n_words"], a["n_bits"], a["status"], None)

    def d(**kw):
        a = dict(d_ok, **kw)
        return dec(a["semantics"], a["words"], a["wo"], a["stride"], a["cap"], a["n_words"], a["sym"], a["sb"], a["so"], a["n"], a["status"], None)

    assert e(n=0) == 0 and d(n=0) == 0
    for kw in (dict(sym=None), dict(so=None), dict(words=None), dict(n_words=None), dict(status=None), dict(sb=0), dict(sb=3), dict(semantics=7)):
        assert e(**kw) == INVALID and e(n=0, **kw) == INVALID, kw
        assert d(**kw) == INVALID and d(n=0, **kw) == INVALID, kw


def test_python_argument_errors():
    torch = pytest.importorskip("torch")
    from constriction_amd import batched as B
    from constriction_amd.symbol.exp_golomb import ExpGolomb
    assert B.exp_golomb_max_words(100, torch.uint8, "queue") == 64
    with pytest.raises(TypeError):
        B.exp_golomb_max_words(100, torch.float32)
    with pytest.raises(ValueError):
        B.exp_golomb_max_words(100, torch.int32, "heap")
    with pytest.raises(ValueError):
        B.exp_golomb_encode(torch.zeros((2, 2), dtype=torch.int32))        # host memory
    assert ExpGolomb().bits == 32 and ExpGolomb(8).num_symbols() == 256
    with pytest.raises(ValueError):
        ExpGolomb(12)
    with pytest.raises(TypeError):
        ExpGolomb("32")
