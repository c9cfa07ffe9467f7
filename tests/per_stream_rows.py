"""Shared by tests/test_gpu_range_per_stream.py and tests/test_range_per_stream_cpu.py: cdf rows with one table per stream, symbols drawn
from them, and the CPU oracle's range coder run once per stream (its range calls take one cdf).  Everything here is computed once per
(case, shape, preset) and handed out read-only."""
import functools

import numpy as np

from test_gpu_fit_per_stream_models import CASES as FIT_CASES, case_rows as fit_case_rows, cdfs_of

# n_streams, n_per: the smallest batch; a second, partial wave with one tile and a scalar tail; whole waves and tiles; N % 4 == 0 but no
# whole tiles; two workgroups, odd N with unaligned rows, word rings that wrap many times
SHAPES = [(1, 1), (65, 33), (64, 96), (130, 100), (257, 4099)]

# case -> (n_symbols, P): the row families of test_gpu_fit_per_stream_models.py, and two precisions beside the bucket index
CASES = {name: (n, P) for name, (n, P, _) in FIT_CASES.items()}
CASES["p16_n300"] = (300, 16)       # rows that store 2^16 as 0, the bounded search, 64-lane workgroups
CASES["p5"] = (20, 5)               # the bounded search below the bucket index

W16_CASES = ["bimodal", "uniform", "n_2_to_P", "p16_n300", "p5"]        # the (16, 32) subset
W16_SHAPES = [(65, 33), (257, 4099)]

CAPACITY_CASE = ("skewed_fitted", 130, 100)


def case_rows(O, case, n_streams, rng):
    n, P = CASES[case]
    if case in FIT_CASES:
        return fit_case_rows(O, case, max(n_streams, 3), rng)[:n_streams]       # (the n = 2 family pins its first three rows)
    # every probability at least 1, the rest spread by random weights (a few streams get it all on one symbol)
    weights = rng.dirichlet(np.full(n, 0.3), n_streams)
    prob = np.ones((n_streams, n), np.int64)
    rest = (1 << P) - n
    for s in range(n_streams):
        prob[s] += rng.multinomial(rest, weights[s])
    prob[0] = 1
    prob[0, n - 1] += rest
    return cdfs_of(prob)


def support_lo(case):
    return -127 if CASES[case][0] <= 255 else -128


@functools.lru_cache(maxsize=None)
def batch(case, n_streams, n_per):
    """(lo, P, cdfs [n_streams, n + 1], symbols [n_streams, n_per]): symbols drawn from the rows, the first and last two symbols of the
    support forced into every stream"""
    from oracle import oracle as O
    n, P = CASES[case]
    lo = support_lo(case)
    rng = np.random.default_rng(n_streams * 7 + n_per + n)
    cdfs = np.ascontiguousarray(case_rows(O, case, n_streams, rng), dtype=np.uint32)
    sym = O.synth_symbols(0xF17, 0, n_streams, n_per, lo, cdfs, P, per_stream_tables=True)
    hi = lo + n - 1
    sym[:, :4] = np.array([lo, hi, lo + 1, hi - 1])[: sym[:, :4].shape[1]]
    cdfs.setflags(write=False)
    sym.setflags(write=False)
    return lo, P, cdfs, sym


def rows_are_valid(cdfs, P):
    c = cdfs.astype(np.int64)
    return bool((c[:, 0] == 0).all() and (c[:, -1] == 1 << P).all() and (np.diff(c, axis=1) > 0).all())


def oracle_encode_rows(sym, lo, cdfs, P, W, S, stride=None):
    """the oracle's range encoder, one call per stream: (words [n_streams, stride], n_words, status)"""
    from oracle import oracle as O
    n_streams, n_per = sym.shape
    stride = stride or O.range_max_words(n_per, P, W, S)
    words = np.zeros((n_streams, stride), np.uint32)
    n_words, status = np.zeros(n_streams, np.uint32), np.zeros(n_streams, np.int32)
    for s in range(n_streams):
        w, n, st = O.rc_encode_batch(sym[s:s + 1], lo, cdfs[s], P, W, S, stride)
        words[s], n_words[s], status[s] = w[0], n[0], st[0]
    return words, n_words, status


@functools.lru_cache(maxsize=None)
def oracle_encode(case, n_streams, n_per, W=32, S=64):
    lo, P, cdfs, sym = batch(case, n_streams, n_per)
    out = oracle_encode_rows(sym, lo, cdfs, P, W, S)
    for a in out:
        a.setflags(write=False)
    return out


def oracle_decode(words, n_words, n_per, lo, cdfs, P, W=32, S=64):
    from oracle import oracle as O
    out = np.zeros((len(n_words), n_per), np.int32)
    status = np.zeros(len(n_words), np.int32)
    for s in range(len(n_words)):
        d, st = O.rc_decode_batch(words[s:s + 1], n_words[s:s + 1], n_per, lo, cdfs[s], P, W, S)
        out[s], status[s] = d[0], st[0]
    return out, status


def oracle_jump_table(sym, lo, cdfs, P, interval, W=32, S=64):
    """(pos, lower, range), each [n_streams, n_chunks]"""
    from oracle import oracle as O
    parts = [O.range_jump_table(sym[s:s + 1], lo, cdfs[s], P, interval, W, S) for s in range(sym.shape[0])]
    return tuple(np.concatenate([p[k] for p in parts], axis=0) for k in range(3))


def capacity_stride():
    """a slab stride for CAPACITY_CASE under which some streams overflow and some fit, by the oracle's word counts: their median"""
    _, n_words, _ = oracle_encode(*CAPACITY_CASE)
    return int(np.sort(n_words)[len(n_words) // 2])
