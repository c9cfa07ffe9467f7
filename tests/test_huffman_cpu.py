"""CPU-only: cst_huffman_tree (the host half of the Huffman codebooks) against the reference's known answers
(tests/golden/huffman_vectors.json) and against the plain-Python restatement in tests/huffman_ref.py."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

import huffman_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "huffman_vectors.json").read_text())


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import _native, build
    build.build_library()
    return _native.load_library()


def tree(lib, probs, f32):
    from constriction_amd import _native as N
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float32 if f32 else np.float64), dtype=np.float64)
    nodes = np.zeros(max(2 * p.size - 1, 1), dtype=np.uint64)
    st = lib.cst_huffman_tree(p.ctypes.data, p.size, int(f32), nodes.ctypes.data)
    return st, (nodes.tolist() if st == N.CST_OK else None)


@pytest.mark.parametrize("case", GOLDEN["encoder_trees"], ids=lambda c: c["where"])
def test_golden_encoder_trees(lib, case):
    st, nodes = tree(lib, case["probabilities"], case["dtype"] == "float32")
    assert st == 0 and nodes == case["nodes"]
    assert R.prefix_codewords(nodes) == case["prefix_codewords"]


@pytest.mark.parametrize("case", GOLDEN["decoder_trees"], ids=lambda c: c["where"])
def test_golden_decoder_trees(lib, case):
    # the decoder's tree is the same construction: inner node n + k has the children that were popped in round k
    st, nodes = tree(lib, case["probabilities"], case["dtype"] == "float32")
    assert st == 0 and [list(c) for c in R.children(nodes)] == case["children"]


def test_restatement_reproduces_the_doc_vectors():
    d = GOLDEN["doc_examples"]
    nodes = R.tree(np.array(d["probabilities"], dtype=np.float32), True)
    assert R.queue_encode(nodes, d["message"]) == (d["queue"]["words"], d["queue"]["bitrate"])
    st = d["stack_encoded_in_reverse"]
    assert R.stack_encode(nodes, d["message"]) == (st["words"], st["bitrate"])
    assert R.decode(nodes, st["words"], len(d["message"]), "stack") == (d["message"], False)
    assert R.decode(nodes, d["queue"]["words"], len(d["message"]), "queue") == (d["message"], False)


def test_f32_sums_change_the_tree(lib):
    p = [0.3, 0.2, 0.4, 0.1]
    assert tree(lib, p, True)[1] == [10, 9, 12, 8, 11, 13, 0]
    # the same f32 values added in f64: 0.1f + 0.2f < 0.3f, the sum pops before symbol 0
    assert tree(lib, np.float32(p).astype(np.float64), False)[1] == [11, 9, 12, 8, 10, 13, 0]


def test_one_symbol_ties_and_zeros(lib):
    assert tree(lib, [0.7], False) == (0, [0])
    assert tree(lib, [0.0], True) == (0, [0])
    assert tree(lib, [1, 1, 1, 1], False)[1] == R.tree([1, 1, 1, 1], False)
    z = [0.0, 0.5, 0.0, 0.0, 0.5]
    st, nodes = tree(lib, z, False)
    assert st == 0 and nodes == R.tree(z, False)
    assert tree(lib, [-0.0, 1.0], False)[1] == [4, 5, 0]


@pytest.mark.parametrize("bad", [[0.5, float("nan")], [0.5, -0.1], [0.5, float("inf")], [3.5e38 * 2, 1.0]])
def test_invalid_probabilities_are_rejected(lib, bad):
    from constriction_amd import _native as N
    p = np.asarray(bad, dtype=np.float64)
    nodes = np.zeros(2 * p.size - 1, dtype=np.uint64)
    assert lib.cst_huffman_tree(p.ctypes.data, p.size, 0, nodes.ctypes.data) == N.CST_ERR_MODEL or bad[0] > 3.4e38
    assert lib.cst_huffman_tree(p.ctypes.data, p.size, 1, nodes.ctypes.data) == N.CST_ERR_MODEL   # (7e38 is inf as f32)
    assert lib.cst_huffman_tree(p.ctypes.data, 0, 0, nodes.ctypes.data) == N.CST_ERR_MODEL


def test_python_errors():
    from constriction_amd import batched as B
    with pytest.raises(FloatingPointError):
        B.huffman_tree(np.array([0.5, np.nan], dtype=np.float32))
    with pytest.raises(ValueError):
        B.huffman_tree(np.array([0.5, -1.0]))
    with pytest.raises(ValueError):
        B.huffman_tree(np.array([0.5, np.inf]))
    with pytest.raises(TypeError):
        B.huffman_tree(np.array([1, 2]))


def _kraft_and_bound(nodes, probs):
    lengths = [len(c) for c in R.suffix_codewords(nodes)]
    n = len(lengths)
    if n > 1:
        assert sum(2.0 ** -l for l in lengths) == 1.0            # a full binary tree
    assert max(lengths) <= n - 1
    # a codeword of length l needs a probability of at most ~ F(l+2)^-1 of the total (the Fibonacci bound)
    total, fib = float(np.sum(probs)), [1, 1]
    while len(fib) < max(lengths) + 3:
        fib.append(fib[-1] + fib[-2])
    for p, l in zip(probs, lengths):
        if p > 0 and total > 0 and l >= 2:
            assert p / total <= 1.0 / fib[l] * (1 + 1e-6)


def test_random_trees_match_the_restatement(lib):
    rng = np.random.default_rng(20261016)
    for k in range(2000):
        n = int(rng.integers(1, 40))
        kind = k % 4
        if kind == 0:
            p = rng.random(n)
        elif kind == 1:
            p = rng.integers(0, 4, n).astype(np.float64)          # many ties and zeros
        elif kind == 2:
            p = np.exp(rng.normal(0, 6, n))                        # skewed
        else:
            p = rng.dirichlet(np.ones(n) * 0.3)
        f32 = bool(k & 1)
        if f32:
            p = p.astype(np.float32)
        st, nodes = tree(lib, p, f32)
        assert st == 0
        assert nodes == R.tree(p, f32), (k, p.tolist(), f32)
        if kind != 1:
            _kraft_and_bound(nodes, np.asarray(p, dtype=np.float64))


def test_fibonacci_probabilities_give_long_codes(lib):
    fib = [1.0, 1.0]
    while len(fib) < 200:
        fib.append(fib[-1] + fib[-2])
    st, nodes = tree(lib, fib, False)
    lengths = [len(c) for c in R.suffix_codewords(nodes)]
    assert st == 0 and max(lengths) > 100 and nodes == R.tree(fib, False)
    assert math.isclose(sum(2.0 ** -l for l in lengths), 1.0)
