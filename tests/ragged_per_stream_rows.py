"""Shared by tests/test_gpu_ragged_per_stream.py and tests/test_ragged_per_stream_cpu.py: ragged batches with ONE TABLE PER STREAM.  The rows
are those of per_stream_rows.py; the symbols are drawn from them on a rectangle (the oracle's generator) and every row is cut to its
length; the expected words come from the CPU oracle coding document s ALONE with cdfs[s].  Everything is computed once per (case, number
of streams, preset) and handed out read-only."""
import functools

import numpy as np

from per_stream_rows import CASES, case_rows, rows_are_valid, support_lo  # noqa: F401  (re-exported)

PARITY_CASES = ["skewed_fitted", "bimodal", "uniform", "one_last", "n2", "n257", "n_2_to_P", "p16_n300", "p5"]
W16_CASES = ["bimodal", "p16_n300", "p5"]            # the (16, 32) subset
# a partial wave, two waves, two workgroups at every workgroup size the geometry picks
STREAM_COUNTS = [1, 63, 64, 65, 130, 257]
# the group-of-eight tail, the ring wrap, and -- once per batch -- a long chain beside idle lanes
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 515]
LONG = 4099


def lengths_of(n_streams):
    """LENGTHS over and over (started at a different place per batch size), and one stream of LONG symbols among them"""
    n = np.array([LENGTHS[(s + n_streams) % len(LENGTHS)] for s in range(n_streams)], np.int64)
    n[n_streams // 2] = LONG
    return n


@functools.lru_cache(maxsize=None)
def batch(case, n_streams):
    """(lo, P, cdfs [n_streams, n + 1], docs: list of int32 arrays, offsets int64 [n_streams + 1]); the first and last two symbols of
    the support are forced into every stream of four or more symbols"""
    from oracle import oracle as O
    n, P = CASES[case]
    lo = support_lo(case)
    rng = np.random.default_rng(n_streams * 11 + n)
    cdfs = np.ascontiguousarray(case_rows(O, case, n_streams, rng), dtype=np.uint32)
    lengths = lengths_of(n_streams)
    sym = O.synth_symbols(0xA66ED, 0, n_streams, int(lengths.max()), lo, cdfs, P, per_stream_tables=True)
    hi = lo + n - 1
    docs = []
    for s in range(n_streams):
        doc = sym[s, : lengths[s]].copy()
        if len(doc) >= 4:
            doc[:4] = [lo, hi, lo + 1, hi - 1]
        doc.setflags(write=False)
        docs.append(doc)
    offsets = np.zeros(n_streams + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    cdfs.setflags(write=False)
    offsets.setflags(write=False)
    return lo, P, cdfs, docs, offsets


def ans_slab(n, P, W, S):
    """the words batched.ans_encode_ragged allocates for a stream of n symbols, before it rounds slabs up to 16 bytes"""
    return min(n, (n * P + W - 1) // W) + S // W


def range_slab(n, P, W, S):
    return min(n, (n * P + W - 1) // W) + 2


def oracle_ans_words(doc, lo, cdf, P, W=32, S=64):
    from oracle import oracle as O
    coder = O.AnsCoder(W=W, S=S)
    coder.encode_iid_table_reverse(doc, cdf, lo, P)
    return coder.get_compressed()


def oracle_range_words(doc, lo, cdf, P, W=32, S=64):
    """(words, status)"""
    from oracle import oracle as O
    words, n, st = O.rc_encode_batch(np.asarray(doc, np.int32)[None, :], lo, cdf, P, W, S)
    return words[0, : n[0]].copy(), int(st[0])


@functools.lru_cache(maxsize=None)
def oracle_words(coder, case, n_streams, W=32, S=64):
    """tuple of the oracle's words of every document, each coded alone under its own row"""
    lo, P, cdfs, docs, _ = batch(case, n_streams)
    out = []
    for s, doc in enumerate(docs):
        if coder == "ans":
            w = oracle_ans_words(doc, lo, cdfs[s], P, W, S)
        else:
            w, st = oracle_range_words(doc, lo, cdfs[s], P, W, S)
            assert st == 0
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def oracle_jump_table(coder, doc, lo, cdf, P, every, W=32, S=64):
    """the oracle's table of ONE document: (pos, state) resp. (pos, lower, range), each [n_chunks]"""
    from oracle import oracle as O
    fn = O.ans_jump_table if coder == "ans" else O.range_jump_table
    return tuple(x[0] for x in fn(np.asarray(doc, np.int32)[None, :], lo, cdf, P, every, W, S))


def oracle_decode_chunk(coder, words, entry, n, lo, cdf, P, W=32, S=64):
    """n symbols decoded by the oracle alone from one table entry on one document's words: (symbols, status)"""
    from oracle import oracle as O
    if coder == "ans":
        return O.ans_decode_from(words, entry[0], entry[1], n, lo, cdf, P, W, S), 0
    out, st = O.range_decode_from(words, entry[0], entry[1], entry[2], n, lo, cdf, P, W, S)
    return out, int(st)
