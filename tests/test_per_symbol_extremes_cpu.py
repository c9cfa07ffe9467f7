"""The zoo of tests/per_symbol_extremes.py against the CPU oracle alone (no GPU): every hard value is in the batch, every model of the
zoo has a valid table, the oracle's ANS and range coders round-trip its symbols, and the supports that fill the precision give the
tables the GPU tests count on.  This keeps tests/test_gpu_per_symbol_extremes.py honest: a zoo that lost its hard columns, or an
oracle that raised for one of them, fails here."""
import numpy as np
import pytest

import per_symbol_extremes as Z

cfg_id = lambda c: "W%dS%dP%d" % c
SHAPE = (6, 24)                     # (more columns than hard values: every stream has all of them)
SHORT = (14, 5)                     # (fewer: the list is rotated by the stream's index)


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=cfg_id)
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_every_model_of_the_zoo_has_a_valid_table_and_round_trips(family, cfg):
    W, S, P = cfg
    for lo, hi in Z.supports(P):
        for n_streams, n_per in (SHAPE, SHORT):
            sym, a, b = Z.zoo(family, lo, hi, n_streams, n_per, P, 5)
            assert sym.dtype == np.int32 and sym.shape == a.shape == b.shape == (n_streams, n_per)
            assert Z.hard_values_present(lo, hi, a, b), (lo, hi, n_per)
            if n_per >= Z.N_HARD:
                for s in range(n_streams):
                    assert Z.hard_values_present(lo, hi, a[s], b[s]), (lo, hi, s)
            assert sym.min() == lo and sym.max() == hi
            for s in range(n_streams):
                assert lo in sym[s] and hi in sym[s]
            for s in range(0, n_streams, 3 if hi - lo > 1000 else 1):
                for x, y in zip(a[s], b[s]):
                    cdf = Z.table(family, lo, hi, x, y, P, Z.prob_bits_of(W)).astype(np.int64)
                    assert cdf[0] == 0 and cdf[-1] == 1 << P and np.diff(cdf).min() >= 1, (lo, hi, x, y)
                models = Z.models_of(family, lo, hi, a[s], b[s], P, W)
                for coder in ("ans", "range"):
                    words = Z.oracle_words(coder, cfg, family, lo, hi, sym[s], a[s], b[s], models)
                    assert Z.oracle_decode(coder, cfg, words, models).tolist() == sym[s].tolist(), (coder, lo, hi, s)
                # the Gaussian's two oracle paths agree (encode_gaussian_reverse and a list of GaussianModel)
                if family == "gaussian":
                    c = Z.O.AnsCoder(W=W, S=S)
                    c.encode_reverse(sym[s], models, P)
                    assert c.get_compressed().tolist() == Z.oracle_words("ans", cfg, family, lo, hi, sym[s], a[s], b[s]).tolist()


def test_the_ragged_zoo_keeps_the_hard_values_and_the_ends():
    lengths = (0, 1, 15, 16, 17, 70, 300) * 2
    syms, locs, scales = Z.zoo_ragged("laplace", -100, 100, lengths, 24, 3)
    assert [len(x) for x in syms] == list(lengths) == [len(x) for x in locs] == [len(x) for x in scales]
    assert Z.hard_values_present(-100, 100, np.concatenate(locs), np.concatenate(scales))
    for sym in syms:
        assert len(sym) < 2 or (-100 in sym and 100 in sym)
    assert {int(s[0]) for s in syms if len(s) == 1} == {-100, 100}
    # the symbol choices: the least and the most probable symbol of their model are where the cycle puts them
    sym, a, b = syms[6], locs[6], scales[6]
    other = []                      # positions of the two choices that hold something else: only the two that got lo and hi may
    for j in range(len(sym)):
        probs = np.diff(Z.table("laplace", -100, 100, a[j], b[j], 24).astype(np.int64))
        want = {1: probs.min(), 2: probs.max()}.get((j + 6) % 4)
        if want is not None and probs[sym[j] + 100] != want:
            other.append(int(sym[j]))
    assert len(other) <= 2 and set(other) <= {-100, 100}


@pytest.mark.parametrize("cfg", [(16, 32, 12), (32, 64, 12)], ids=cfg_id)
@pytest.mark.parametrize("family", Z.FAMILIES)
def test_supports_that_fill_the_precision(family, cfg):
    """n = 2^P: free weight 0, every probability 1, every symbol costs exactly P bits; n = 2^P - 1: probabilities 1 and 2"""
    W, S, P = cfg
    sym, a, b = Z.uniform_batch(-2048, 2047, 2, 40, 9)
    assert all((b == v).any() for v in Z.HARD_SCALES) and (a == Z.DBL_MAX).any() and (a == -Z.DBL_MAX).any()
    for x, y in zip(a[0], b[0]):
        assert (np.diff(Z.table(family, -2048, 2047, x, y, P, Z.prob_bits_of(W)).astype(np.int64)) == 1).all()
        probs = np.diff(Z.table(family, -2048, 2046, x, y, P, Z.prob_bits_of(W)).astype(np.int64))
        assert len(probs) == 4095 and probs.sum() == 4096 and set(probs.tolist()) == {1, 2}
    for hi in (2047, 2046):
        sym, a, b = Z.uniform_batch(-2048, hi, 2, 40, 9)
        models = Z.models_of(family, -2048, hi, a[1], b[1], P, W)
        for coder in ("ans", "range"):
            words = Z.oracle_words(coder, cfg, family, -2048, hi, sym[1], a[1], b[1], models)
            assert len(words) >= 40 * (P if hi == 2047 else P - 1) // W          # (a probability of 2 costs P - 1 bits)
            assert Z.oracle_decode(coder, cfg, words, models).tolist() == sym[1].tolist()
