"""Shared by tests/test_categorical_perfect_ragged_cpu.py and tests/test_gpu_categorical_perfect_ragged.py: the ragged batches both files
look at, and their oracle results.

Rows and symbols are drawn by the recipe of tests/test_gpu_categorical_ragged.py::workload: unnormalised Dirichlet(0.3) rows with exact
zeros inside, a last entry of at least 2e-3 of the sum, uniform symbols (so they sit on exact-zero entries too: perfect=True gives every
entry at least one unit of weight, so none of them is impossible), and symbols 0 and K - 1 in front of every stream.  The CPU file
checks the condition the GPU file rests on: the library's host quantiser gives every such row code 0 and the words of
oracle.categorical_perfect_cdf.  A batch and its oracle results are built once per key, shared, and never modified; the oracle
quantises a batch in about a second at K <= 257 and in about two at K = 1024 (1190 rows)."""
import numpy as np

from persymbol_jump_oracle import ans_table, range_table

CONFIGS = [(32, 64, 24), (16, 32, 12)]
CODERS = ["ans", "range"]
DTYPES = {"f32": np.float32, "f64": np.float64}
# paired, not a cross product: the edges of the quantiser's 64 / 256 / 1024 slot capacities, both dtypes
MODELS = [(2, "f64"), (5, "f32"), (64, "f64"), (65, "f32"), (256, "f32"), (257, "f64")]
# 70 streams of 0 .. 300 symbols, 2955 rows: more units than one workgroup of the piece decoder holds, empty streams at both ends
PARITY_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300, 0] * 5
# 9 streams, 1190 rows
LOCAL_LENGTHS = [100, 0, 200, 47, 48, 150, 49, 500, 96]
OK, IMPOSSIBLE, CAPACITY, INVALID = 0, 1, 2, 3
cfg_id = lambda c: "W%dS%dP%d" % c
model_id = lambda m: "K%d-%s" % m


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def workload(lengths, k, dtype, seed):
    """flat probabilities [sum(lengths), k] and flat symbols: uniform draws, with symbol 0 and symbol k - 1 in front of every stream
    (alternating over the streams where a stream has one symbol)"""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    probs = rng.dirichlet(np.full(k, 0.3), size=n)
    if k > 2:
        probs[:, 1:-1][rng.random((n, k - 2)) < 0.3] = 0.0
    probs[:, -1] = np.maximum(probs[:, -1], 2e-3)               # (the sum stays below 1.002: at least 1e-3 of it)
    probs *= np.exp(rng.uniform(-3.0, 3.0, (n, 1)))              # not normalised
    probs = np.ascontiguousarray(probs.astype(dtype))
    sym = rng.integers(0, k, n).astype(np.int32)
    off = offsets_of(lengths)
    for s, length in enumerate(lengths):
        if length >= 2:
            sym[off[s]], sym[off[s] + 1] = 0, k - 1
        elif length == 1:
            sym[off[s]] = k - 1 if s % 2 == 0 else 0
    return sym, probs


def models_of(O, probs, P):
    """one tabulated model per row: f32 rows are widened to f64 first, as the reference's `F: Into<f64>` does"""
    return [O.TableModel(O.categorical_perfect_cdf(np.asarray(row, dtype=np.float64), P), 0, P) for row in probs]


def oracle_words(O, coder, cfg, sym, models):
    """get_compressed() of one oracle coder (a zero-length stream: no words from either coder)"""
    W, S, P = cfg
    if coder == "ans":
        if len(sym) == 0:
            return np.zeros(0, np.uint32)
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return np.asarray(c.get_compressed())


_BATCHES = {}       # (name, k, dtype, P) -> (sym, probs, off, models per stream)
_WORDS = {}         # (batch key, coder, cfg) -> oracle words per stream
_TABLES = {}        # (batch key, coder, cfg, every) -> [(words, table)] per stream


def batch(O, name, lengths, k, dtype, P):
    key = (name, k, dtype, P)
    if key not in _BATCHES:
        sym, probs = workload(lengths, k, DTYPES[dtype], 17 * k + P + len(lengths))
        off = offsets_of(lengths)
        models = models_of(O, probs, P)
        _BATCHES[key] = (sym, probs, off, [models[off[s]: off[s + 1]] for s in range(len(lengths))])
    return key, _BATCHES[key]


def words_of(O, key, coder, cfg):
    if (key, coder, cfg) not in _WORDS:
        sym, _, off, models = _BATCHES[key]
        _WORDS[(key, coder, cfg)] = [oracle_words(O, coder, cfg, sym[off[s]: off[s + 1]], models[s]) for s in range(len(models))]
    return _WORDS[(key, coder, cfg)]


def tables_of(O, key, coder, cfg, every):
    if (key, coder, cfg, every) not in _TABLES:
        sym, _, off, models = _BATCHES[key]
        table_of = ans_table if coder == "ans" else range_table
        _TABLES[(key, coder, cfg, every)] = [table_of(O, cfg, sym[off[s]: off[s + 1]], models[s], every) for s in range(len(models))]
    return _TABLES[(key, coder, cfg, every)]
