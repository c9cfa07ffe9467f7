"""The shared workload of the per-symbol Categorical "extremes" tests: a ZOO of hard probability rows and hard symbols, and what the CPU
oracle makes of it.  The role of tests/per_symbol_extremes.py, for rows of probabilities in place of (location, scale).

No GPU here.  tests/test_categorical_extremes_cpu.py checks the zoo itself (every kind is in every batch, the host twins of the
quantisers give the oracle's rows, the oracle's coders round-trip it); tests/test_gpu_categorical_extremes.py runs every Categorical
kernel on it.  Every expectation comes from the oracle alone: oracle.categorical_fast_cdf (f32 rows in f32, f64 rows in f64) or
oracle.categorical_perfect_cdf, one TableModel per symbol, one oracle coder per stream.

The ORACLE classifies every row, never a list written by hand:
    refused      the quantiser raises
    valid        the table is strictly increasing
    degenerate   the table is accepted and has at least one empty interval (cdf[i] == cdf[i + 1])
and this module asserts that no accepted table decreases anywhere.

A stream of a batch is one of three:
    plain    (most)          every accepted kind in its first columns, rotated by the stream's index, Dirichlet rows behind them; every
                             symbol has a non-empty interval: the oracle's coders code it
    refused  (s % 4 == 3)    a plain stream with ONE refused row put over one of its rows: CST_STREAM_IMPOSSIBLE_SYMBOL
    failing  (s % 8 == 5)    a plain stream in which ONE symbol of a degenerate row is moved into an empty interval: the same status.
                             Such a symbol is never handed to an oracle coder (its division by a zero probability ends the process);
                             the expected status comes from np.diff(table) == 0
A batch, its tables and the oracle's words are built once per key and shared; nothing that is handed out is ever modified."""
import numpy as np

from oracle import oracle as O
from persymbol_jump_oracle import ans_table, range_table

DTYPES = {"f32": np.float32, "f64": np.float64}
PRESETS = [(32, 64, 24), (16, 32, 12)]
CHUNK = 64                                  # kCatChunk: the columns of a row that the fast kernels stage at a time
# K paired with a dtype, not a cross product: one chunk, a full one, one column over (two chunks), a partial third chunk; both dtypes
# on both sides of the chunk boundary
MODELS = [(2, "f64"), (5, "f32"), (64, "f64"), (65, "f32"), (257, "f32"), (257, "f64")]
PERFECT_MODELS = MODELS[:5] + [(300, "f32")]          # K = 300: beyond the 256 entries of the by-rows decoder, the piece decoder
N_STREAMS, N_PER = 70, 20                   # a full wave of streams and a partial one
RAGGED_LENGTHS = ([0, 1, 2, 15, 16, 17, 33, 49, 300] * 8)[:N_STREAMS]
JUMP_EVERY = 16
HARD_SPAN = 34                              # ragged streams hold hard rows in their first 34 columns: around the jump points 16 and 32
OK, IMPOSSIBLE = 0, 1
SPOILS = {"nan": np.nan, "negative": -0.25, "inf": np.inf}          # (negative: see hard_rows)
model_id = lambda m: "K%d-%s" % m
cfg_id = lambda c: "W%dS%dP%d" % c


def quantise(quant, row, P):
    """the oracle's table of one row, or None where the oracle refuses it"""
    try:
        return (O.categorical_fast_cdf if quant == "fast" else O.categorical_perfect_cdf)(row, P)
    except ValueError:
        return None


def classify(table):
    if table is None:
        return "refused"
    steps = np.diff(table.astype(np.int64))
    assert (steps >= 0).all(), "an accepted table decreases"
    return "valid" if (steps > 0).all() else "degenerate"


def dirichlet_row(rng, k, dtype):
    """the recipe of tests/test_gpu_categorical_batch.py: unnormalised Dirichlet(0.3), exact zeros inside, a last entry that keeps the
    last interval"""
    row = rng.dirichlet(np.full(k, 0.3))
    if k > 2:
        row[1:-1][rng.random(k - 2) < 0.3] = 0.0
    row[-1] = max(row[-1], 2e-3)
    return (row * np.exp(rng.uniform(-3.0, 3.0))).astype(dtype)


def hard_rows(dtype, P, k, seed):
    """{kind: row [k] in dtype}, deterministic.  `tiny` is the smallest normal number of the dtype, `big` its largest finite one."""
    F = DTYPES[dtype]
    fi = np.finfo(F)
    tiny, big = F(fi.tiny), F(fi.max)
    rng = np.random.default_rng(seed)
    free = float((1 << P) - k)
    zeros = lambda: np.zeros(k, F)
    rows = {}
    r = zeros()
    r[0] = r[k - 1] = tiny / F(2)
    rows["min_normal_sum"] = r                                   # the sum is exactly `tiny`: accepted, and the scale is infinite
    r = zeros()
    r[k // 2] = np.nextafter(tiny, F(0))
    rows["largest_subnormal_sum"] = r
    inf_sum = free / float(big) / 4.0                           # (2^P - K) / sum = 4 big: infinite
    rows["inf_scale_equal"] = np.full(k, inf_sum / k, F)
    pattern = np.array([0.0, 0.0, 1.0, 4.0, 0.0, 9.0])
    r = np.tile(pattern, -(-k // 6))[:k]
    if k < 3:
        r[-1] = 1.0                                              # (two columns of the pattern are all zeros: keep the zero in front)
    rows["inf_scale_gaps"] = (r * (inf_sum / r.sum())).astype(F)
    rows["scale_huge_finite"] = np.full(k, 16.0 * inf_sum / k, F)    # sum = 4 (2^P - K) / big: a finite scale near big / 4
    rows["near_max_sum"] = np.full(k, float(big) / k * 0.999, F)
    r = np.full(k, float(big) / k, F)
    r[-1] = big / F(2)
    rows["overflow_at_last_column"] = r                          # (K = 2: big / 2 twice, a finite sum)
    r = np.full(k, 1e-9 if dtype == "f32" else 1e-18, F)
    r[0] = 1.0
    rows["absorbed_after_first"] = r
    r = zeros()
    r[0] = 1.0
    rows["all_in_first"] = r
    r = zeros()
    r[-1] = 1.0
    rows["all_in_last"] = r
    r = np.full(k, -0.0, F)
    r[::2] = 1.0
    rows["negative_zeros"] = r
    e = np.linspace(fi.minexp - fi.nmant, fi.maxexp - 2, k)      # from the smallest subnormal's exponent
    rows["range_ascending"] = np.exp2(e).astype(F)
    rows["range_descending"] = np.exp2(e[::-1]).astype(F)
    if dtype == "f32" and P == 24:
        while True:                                              # (about 15 % of the sums in a binade qualify)
            r = rng.dirichlet(np.full(k, 0.3)).astype(F)
            r[-1] = 0.0
            t = quantise("fast", r, P)
            if t is not None and t[k - 1] == 1 << P:
                break
        rows["empty_last_interval"] = r
    for name, value in SPOILS.items():
        for where, col in (("first", 0), ("chunk", CHUNK), ("last", k - 1)):
            if col < k and not (where == "chunk" and col == k - 1):
                r = dirichlet_row(rng, k, F)
                r[col] = value
                if name == "negative":
                    # The fast quantiser of the reference looks at the SUM alone, so the entry outweighs the rest of the row.  (A
                    # small negative entry with a positive sum is a row the oracle tabulates, with a table that decreases; the
                    # library refuses every negative entry -- DESIGN.md 4.17, tests/test_categorical_batch_cpu.py -- and no
                    # oracle can judge that.)
                    r[col] = -2.0 * (float(np.sum(r.astype(np.float64))) + 0.25)
                rows[f"{name}_{where}"] = r
    for r in rows.values():
        assert r.dtype == F and r.shape == (k,)
    return rows


class Zoo:
    """the hard rows of one (quantiser, K, dtype, P) and the oracle's verdicts: rows, tables, kinds by class"""

    def __init__(self, quant, k, dtype, P):
        self.quant, self.k, self.dtype, self.P = quant, k, dtype, P
        self.rows = hard_rows(dtype, P, k, 1000 * k + P + (dtype == "f64"))
        self.tables = {kind: quantise(quant, row, P) for kind, row in self.rows.items()}
        self.classes = {kind: classify(t) for kind, t in self.tables.items()}
        self.accepted = [kind for kind, c in self.classes.items() if c != "refused"]
        self.refused = [kind for kind, c in self.classes.items() if c == "refused"]


_ZOOS, _BATCHES, _WORDS = {}, {}, {}


def zoo(quant, k, dtype, P):
    key = (quant, k, dtype, P)
    if key not in _ZOOS:
        _ZOOS[key] = Zoo(*key)
    return _ZOOS[key]


def pick_symbol(table, choice, turn, rng):
    """a symbol with a non-empty interval: 0 the table's symbol of a random quantile, 1 one of the least probable, 2 one of the most
    probable, 3 the first (turn even) or the last (turn odd) non-empty entry"""
    cdf = table.astype(np.int64)
    probs = np.diff(cdf)
    live = np.flatnonzero(probs > 0)
    if choice == 0:
        return int(np.searchsorted(cdf[:-1], int(rng.integers(0, cdf[-1])), side="right")) - 1
    if choice == 1:
        return int(rng.choice(live[probs[live] == probs[live].min()]))
    if choice == 2:
        return int(rng.choice(np.flatnonzero(probs == probs.max())))
    return int(live[-1] if turn % 2 else live[0])


class Batch:
    """streams of the zoo: per stream symbols `syms`, rows `probs` [n, K], oracle `tables` [n, K + 1] (a refused row's: the in-band
    row 0xffffffff, 2^P, ...), `kinds` (None for a filler row) and `choices`; `refused` {stream: column} and `failing`
    {stream: column}: the streams that must report IMPOSSIBLE_SYMBOL, and why"""

    def __init__(self, quant, k, dtype, P, lengths, span):
        z = zoo(quant, k, dtype, P)
        F = DTYPES[dtype]
        self.zoo, self.quant, self.k, self.dtype, self.P, self.lengths = z, quant, k, dtype, P, [int(n) for n in lengths]
        rng = np.random.default_rng(31 * k + P + len(lengths) + sum(self.lengths) + (quant == "perfect"))
        rect = len(set(self.lengths)) == 1
        n_acc = len(z.accepted)
        bad_row = np.array([0xFFFFFFFF] + [1 << P] * k, dtype=np.uint32)
        self.syms, self.probs, self.tables, self.kinds, self.choices, self.refused, self.failing = [], [], [], [], [], {}, {}
        n_refused = n_failing = turn = 0
        for s, n in enumerate(self.lengths):
            probs, tables, kinds, choices, sym = np.empty((n, k), F), np.empty((n, k + 1), np.uint32), [None] * n, [0] * n, np.empty(n, np.int32)
            # the rotation: the stream's index, or (ragged) the number of plain streams in front of it that reach a jump point -- the
            # lengths repeat with a period of their own, and every kind is to meet every jump point in a stream that codes
            rot = s if rect else turn
            turn += n > JUMP_EVERY and s % 4 != 3 and s % 8 != 5
            for j in range(n):
                if j < span:
                    kinds[j] = z.accepted[(j + rot) % n_acc]
                    probs[j], tables[j] = z.rows[kinds[j]], z.tables[kinds[j]]
                else:
                    probs[j] = dirichlet_row(rng, k, F)
                    tables[j] = quantise(quant, probs[j], P)
                choices[j] = (j + 2 * rot + rot // 4) % 4       # (not in step with the kinds, nor with the streams that fail)
                sym[j] = pick_symbol(tables[j], choices[j], (j + s) // 4, rng)
            if s % 4 == 3 and n:
                # one refused row, over a filler row where the stream has one (the kinds come in turn, the column moves)
                kind = z.refused[n_refused % len(z.refused)]
                fillers = [j for j in range(n) if kinds[j] is None]
                col = fillers[n_refused % len(fillers)] if fillers else n_refused % n
                kinds[col], probs[col], tables[col] = kind, z.rows[kind], bad_row
                self.refused[s] = col
                n_refused += 1
            elif s % 8 == 5:
                cols = [j for j in range(n) if (np.diff(tables[j].astype(np.int64)) == 0).any()]
                if cols:
                    col = cols[n_failing % len(cols)]
                    empty = np.flatnonzero(np.diff(tables[col].astype(np.int64)) == 0)
                    sym[col] = empty[-1] if n_failing % 2 else empty[0]
                    self.failing[s] = col
                    n_failing += 1
            self.syms.append(sym), self.probs.append(probs), self.tables.append(tables), self.kinds.append(kinds), self.choices.append(choices)
        assert n_refused >= len(z.refused), "more refused kinds than streams that hold one"
        self.bad = sorted(set(self.refused) | set(self.failing))
        self.good = [s for s in range(len(self.lengths)) if s not in self.bad]
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)

    def expected_status(self):
        return [IMPOSSIBLE if s in self.bad else OK for s in range(len(self.lengths))]

    def flat(self):
        """(symbols [n_total], rows [n_total, K]) of the ragged calls"""
        return np.concatenate(self.syms), np.ascontiguousarray(np.concatenate(self.probs))

    def rect(self):
        """(symbols [n_streams, n_per], rows [n_streams, n_per, K]) of the rectangular calls"""
        return np.stack(self.syms), np.ascontiguousarray(np.stack(self.probs))

    def models(self, s):
        return [O.TableModel(t, 0, self.P) for t in self.tables[s]]


def rect_batch(quant, k, dtype, P):
    key = (quant, k, dtype, P, "rect")
    if key not in _BATCHES:
        _BATCHES[key] = Batch(quant, k, dtype, P, [N_PER] * N_STREAMS, len(zoo(quant, k, dtype, P).accepted))
    return _BATCHES[key]


def ragged_batch(quant, k, dtype, P):
    key = (quant, k, dtype, P, "ragged")
    if key not in _BATCHES:
        _BATCHES[key] = Batch(quant, k, dtype, P, RAGGED_LENGTHS, HARD_SPAN)
    return _BATCHES[key]


def oracle_words(coder, cfg, sym, models):
    """get_compressed() of one oracle coder for one stream (no symbols: no words, from either coder)"""
    W, S, P = cfg
    if len(sym) == 0:
        return np.zeros(0, np.uint32)
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


def expected(shape, quant, k, dtype, cfg, every=0):
    """(batch, {coder: per stream the oracle's words, or (words, jump table) with a jump point every `every` symbols; None for a
    stream that must fail}); shape: "rect" or "ragged".  The models of a stream are built once and serve both coders."""
    bt = (rect_batch if shape == "rect" else ragged_batch)(quant, k, dtype, cfg[2])
    key = (shape, quant, k, dtype, cfg, every)
    if key not in _WORDS:
        out = {"ans": [None] * len(bt.lengths), "range": [None] * len(bt.lengths)}
        for s in bt.good:
            models = bt.models(s)
            if every:
                out["ans"][s] = ans_table(O, cfg, bt.syms[s], models, every)
                out["range"][s] = range_table(O, cfg, bt.syms[s], models, every)
            else:
                out["ans"][s] = oracle_words("ans", cfg, bt.syms[s], models)
                out["range"][s] = oracle_words("range", cfg, bt.syms[s], models)
        _WORDS[key] = out
    return bt, _WORDS[key]
