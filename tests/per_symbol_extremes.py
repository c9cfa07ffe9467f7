"""The shared workload of the per-symbol "extremes" tests: a ZOO of hard models and hard symbols, and what the CPU oracle makes of it.

No GPU here.  tests/test_per_symbol_extremes_cpu.py checks the zoo itself (every hard value is in the batch, every model has a valid
table, the oracle's coders round-trip it); tests/test_gpu_per_symbol_extremes.py runs every per-symbol kernel on it.  Every
expectation comes from the oracle alone: the Gaussian from AnsCoder.encode_gaussian_reverse / GaussianModel (prob_bits 32 for W = 32,
16 for W = 16), Laplace and Cauchy from TableModel(leaky_family_cdf(...)) as in tests/test_gpu_family_batch.py.

A zoo and the oracle's words for it are built once per (family, support, shape, preset) and shared by coders, layouts and tests;
nothing that is handed out is ever modified (tests that need a variant copy first)."""
import numpy as np

from oracle import oracle as O
from persymbol_jump_oracle import ans_table, range_table

DBL_MAX = 1.7976931348623157e308
DBL_MIN = 2.2250738585072014e-308              # the smallest normal number
DENORM_MIN = 5e-324
FAMILIES = ("gaussian", "laplace", "cauchy")
PRESETS = [(32, 64, 24), (16, 32, 12)]
HARD_SCALES = (1e-300, 1e300, DENORM_MIN, DBL_MIN, 1.3e308, DBL_MAX)       # (1.3e308 sqrt 2 overflows: the Gaussian's argument)
EDGE_SCALE = 1e-310                            # the scale of the column whose location is a bin edge: its reciprocal is infinite
N_HARD = 4 + len(HARD_SCALES) + 1


def supports(P):
    return [(-100, 100), (0, 1), (-5, 2000 if P == 24 else 900), (-127, 127)]


def hard_locations(lo, hi):
    return (lo - 1e9, hi + 1e9, DBL_MAX, -DBL_MAX)


def prob_bits_of(W):
    return 32 if W == 32 else 16


def table(family, lo, hi, a, b, P, prob_bits=None):
    """the oracle's cdf of one model: n + 1 left cumulatives, the last one 2^P"""
    if family == "gaussian":
        return O.GaussianModel(lo, hi, float(a), float(b), P, prob_bits or (32 if P > 16 else 16)).cdf_table()
    return O.leaky_family_cdf(O.FAMILY_LAPLACE if family == "laplace" else O.FAMILY_CAUCHY, lo, hi, float(a), float(b), P)


def models_of(family, lo, hi, a, b, P, W):
    """one oracle model per symbol of a stream"""
    if family == "gaussian":
        return [O.GaussianModel(lo, hi, float(x), float(y), P, prob_bits_of(W)) for x, y in zip(a, b)]
    return [O.TableModel(table(family, lo, hi, x, y, P), lo, P) for x, y in zip(a, b)]


def zoo_stream(family, lo, hi, n, P, rng, s=0):
    """one stream of n symbols: (sym, a, b).  Location uniform in [lo - 50, hi + 50], scale log-uniform in [1e-7, 1e6]; the hard values
    in the first N_HARD columns, one per column (rotated by the stream's index `s` where the stream is shorter than the list); symbols
    cycling through: the oracle table's symbol for a random quantile, one of its least probable symbols, one of its most probable ones, a uniform one
    (the cycle starts at `s`, so that every hard column meets every choice in a batch); lo and hi at two random positions."""
    a = rng.uniform(lo - 50.0, hi + 50.0, n)
    b = np.exp(rng.uniform(np.log(1e-7), np.log(1e6), n))
    hard = [("a", v) for v in hard_locations(lo, hi)] + [("b", v) for v in HARD_SCALES] + [("edge", None)]
    for j in range(min(n, N_HARD)):
        kind, v = hard[(j + (s if n < N_HARD else 0)) % N_HARD]
        if kind == "a":
            a[j] = v
        elif kind == "b":
            b[j] = v
        else:
            a[j], b[j] = float(rng.integers(lo + 1, hi + 1)) - 0.5, EDGE_SCALE
    sym = np.empty(n, np.int32)
    for j in range(n):
        cdf = table(family, lo, hi, a[j], b[j], P).astype(np.int64)
        probs = np.diff(cdf)
        choice = (j + s) % 4
        if choice == 0:
            i = int(np.searchsorted(cdf[:-1], int(rng.integers(0, 1 << P)), side="right")) - 1
        elif choice == 1:
            i = int(rng.choice(np.flatnonzero(probs == probs.min())))
        elif choice == 2:
            i = int(rng.choice(np.flatnonzero(probs == probs.max())))
        else:
            i = int(rng.integers(0, hi - lo + 1))
        sym[j] = lo + i
    if n >= 2:
        at = rng.choice(n, 2, replace=False)
        sym[at[0]], sym[at[1]] = lo, hi
    elif n == 1:
        sym[0] = hi if s % 2 else lo
    return sym, a, b


def zoo_ragged(family, lo, hi, lengths, P, seed):
    """streams of unequal lengths: three lists (sym, a, b)"""
    rng = np.random.default_rng(seed)
    streams = [zoo_stream(family, lo, hi, int(n), P, rng, s) for s, n in enumerate(lengths)]
    return [x[0] for x in streams], [x[1] for x in streams], [x[2] for x in streams]


def zoo(family, lo, hi, n_streams, n_per, P, seed):
    """a rectangular batch: three matrices (sym, a, b) of shape (n_streams, n_per)"""
    sym, a, b = zoo_ragged(family, lo, hi, [n_per] * n_streams, P, seed)
    return np.stack(sym), np.stack(a), np.stack(b)


def hard_values_present(lo, hi, a, b):
    """whether every hard value of the list occurs in the flat arrays a / b"""
    a, b = np.asarray(a), np.asarray(b)
    edge = (b == EDGE_SCALE) & (a - np.floor(a) == 0.5) & (a > lo) & (a < hi + 1)
    return all((a == v).any() for v in hard_locations(lo, hi)) and all((b == v).any() for v in HARD_SCALES) and bool(edge.any())


def oracle_words(coder, cfg, family, lo, hi, sym, a, b, models=None):
    """get_compressed() of one oracle coder for one stream (no symbols: no words, from either coder)"""
    W, S, P = cfg
    if len(sym) == 0:
        return np.zeros(0, np.uint32)
    if coder == "ans" and family == "gaussian":
        c = O.AnsCoder(W=W, S=S)
        c.encode_gaussian_reverse(sym, lo, hi, a, b, P, prob_bits_of(W))
        return np.asarray(c.get_compressed())
    models = models if models is not None else models_of(family, lo, hi, a, b, P, W)
    if coder == "ans":
        c = O.AnsCoder(W=W, S=S)
        c.encode_reverse(sym, models, P)
    else:
        c = O.RangeEncoder(W=W, S=S)
        c.encode(sym, models, P)
    return np.asarray(c.get_compressed())


def oracle_decode(coder, cfg, words, models):
    W, S, P = cfg
    if len(models) == 0:
        return np.zeros(0, np.int32)
    c = O.AnsCoder(words, W=W, S=S) if coder == "ans" else O.RangeDecoder(words, W=W, S=S)
    return c.decode(models, P=P)


_ZOOS = {}          # (family, lo, hi, P, shape or lengths) -> (sym, a, b)
_WORDS = {}         # (family, lo, hi, cfg, shape or lengths, every) -> {coder: [words or (words, table) per stream]}


def rect_zoo(family, lo, hi, P, n_streams, n_per):
    key = (family, lo, hi, P, n_streams, n_per)
    if key not in _ZOOS:
        _ZOOS[key] = zoo(family, lo, hi, n_streams, n_per, P, n_streams * 13 + n_per + P + (hi - lo))
    return _ZOOS[key]


def ragged_zoo(family, lo, hi, P, lengths):
    key = (family, lo, hi, P, tuple(lengths))
    if key not in _ZOOS:
        _ZOOS[key] = zoo_ragged(family, lo, hi, lengths, P, len(lengths) * 7 + P + (hi - lo))
    return _ZOOS[key]


def _expect(key, family, lo, hi, cfg, streams, every, which):
    """both coders' expectations for the streams `which` of [(sym, a, b)]: words, or (words, jump table) with a jump point every
    `every` symbols; the models of a stream are built once and serve both coders"""
    if key not in _WORDS:
        W, S, P = cfg
        out = {"ans": [None] * len(streams), "range": [None] * len(streams)}
        for s in which:
            sym, a, b = streams[s]
            models = models_of(family, lo, hi, a, b, P, W)
            if every:
                out["ans"][s] = ans_table(O, cfg, sym, models, every)
                out["range"][s] = range_table(O, cfg, sym, models, every)
            else:
                out["ans"][s] = oracle_words("ans", cfg, family, lo, hi, sym, a, b, models)
                out["range"][s] = oracle_words("range", cfg, family, lo, hi, sym, a, b, models)
        _WORDS[key] = out
    return _WORDS[key]


def rect_expected(family, lo, hi, cfg, n_streams, n_per, every=0):
    """(sym, a, b, {coder: per stream words, or (words, table) if every}): every stream is compared, on the 2006-symbol support too"""
    sym, a, b = rect_zoo(family, lo, hi, cfg[2], n_streams, n_per)
    want = _expect((family, lo, hi, cfg, n_streams, n_per, every), family, lo, hi, cfg, list(zip(sym, a, b)), every,
                   range(n_streams))
    return sym, a, b, want


def ragged_expected(family, lo, hi, cfg, lengths, every=0):
    """(syms, locs, scales, {coder: per stream words, or (words, table) if every}): every stream is compared"""
    syms, locs, scales = ragged_zoo(family, lo, hi, cfg[2], lengths)
    want = _expect((family, lo, hi, cfg, tuple(lengths), every), family, lo, hi, cfg, list(zip(syms, locs, scales)), every, range(len(lengths)))
    return syms, locs, scales, want


def uniform_batch(lo, hi, n_streams, n_per, seed):
    """zoo parameters (they cannot matter where the support fills the precision) with uniform symbols"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo - 50.0, hi + 50.0, (n_streams, n_per))
    b = np.exp(rng.uniform(np.log(1e-7), np.log(1e6), (n_streams, n_per)))
    k = min(n_per, len(HARD_SCALES))
    b[:, :k] = HARD_SCALES[:k]
    if n_per > k + 1:
        a[:, k], a[:, k + 1] = DBL_MAX, -DBL_MAX
    return rng.integers(lo, hi + 1, (n_streams, n_per)).astype(np.int32), a, b
