"""CPU-only: the zoo of tests/categorical_extremes.py itself, and the oracle's side of it.  Every kind of hard row is in every batch with
the class the oracle gives it; the host twins of the two device quantisers (cst_categorical_fast_cdf_host,
cst_categorical_perfect_cdf_host) give the oracle's rows and bad codes on the whole zoo; for degenerate rows the oracle's lazy model
agrees with its table; the oracle's coders round-trip every stream that is not expected to fail.
tests/test_gpu_categorical_extremes.py runs the kernels on the same batches."""
import ctypes

import numpy as np
import pytest

import categorical_extremes as Z
import categorical_perfect_rows as R
from oracle import oracle as O

CASES = [("fast", k, d) for k, d in Z.MODELS] + [("perfect", k, d) for k, d in Z.PERFECT_MODELS]
case_id = lambda c: "%s-K%d-%s" % c


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build, _native
    build.build_library()
    return _native.load_library()


def host_fast(lib, probs, P):
    probs = np.ascontiguousarray(probs)
    n, k = probs.shape
    rows, bad = np.zeros((n, k + 1), np.uint32), np.full(n, -1, np.int32)
    assert lib.cst_categorical_fast_cdf_host(P, ctypes.c_void_p(probs.ctypes.data), probs.itemsize, n, k, ctypes.c_void_p(rows.ctypes.data),
                                             ctypes.c_void_p(bad.ctypes.data)) == 0
    return rows, bad


# ---------------------------------------------------------------------------------------------- the zoo

@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_what_the_oracle_makes_of_every_kind(case, P):
    """the verdicts the zoo is built for (the classes themselves are the oracle's: this pins what was seen)"""
    quant, k, dtype = case
    z = Z.zoo(quant, k, dtype, P)
    c, total = z.classes, 1 << P
    assert set(c.values()) <= {"valid", "degenerate", "refused"}
    widened = quant == "perfect" and dtype == "f32"         # f32 rows are summed in f64 there: neither subnormal nor overflowing
    assert c["largest_subnormal_sum"] == ("valid" if widened else "refused")
    assert c["overflow_at_last_column"] == ("valid" if k == 2 or widened else "refused")           # K = 2: finfo.max / 2 twice
    for name in Z.SPOILS:
        assert c[f"{name}_first"] == c[f"{name}_last"] == c.get(f"{name}_chunk", "refused") == "refused", name
        assert (f"{name}_chunk" in c) == (k > Z.CHUNK + 1)
    for kind in ("scale_huge_finite", "near_max_sum", "absorbed_after_first", "all_in_first", "all_in_last", "negative_zeros", "range_ascending",
                 "range_descending"):
        assert c[kind] == "valid", kind
    tiny_sum = ("min_normal_sum", "inf_scale_equal", "inf_scale_gaps")
    if quant == "perfect":
        # f32 rows are widened to f64, where their sums are ordinary; the same sums in f64 are refused (`extra > left`)
        assert [c[kind] for kind in tiny_sum] == ["valid" if dtype == "f32" else "refused"] * 3
        assert "degenerate" not in c.values()
        return
    # the fast quantiser: an infinite scale.  0 * inf is NaN and converts to 0, x * inf saturates to u32::MAX, and `+ i` wraps
    assert c["min_normal_sum"] == "degenerate" and c["inf_scale_equal"] == "degenerate"
    assert z.tables["min_normal_sum"].tolist() == [0] + list(range(k - 1)) + [total]
    assert z.tables["inf_scale_equal"].tolist() == [0] + list(range(k - 1)) + [total]
    assert c["inf_scale_gaps"] == ("valid" if k == 2 else "degenerate")
    if k >= 6:
        assert z.tables["inf_scale_gaps"][:6].tolist() == [0, 1, 2, 2, 3, 4]               # [0, 0, t, 4 t, 0, 9 t, ...]
    assert ("empty_last_interval" in c) == (dtype == "f32" and P == 24)
    if "empty_last_interval" in c:
        assert c["empty_last_interval"] == "degenerate" and z.tables["empty_last_interval"][k - 1] == total
    # the text-book cases in three columns
    F = Z.DTYPES[dtype]
    t = F(np.finfo(F).tiny)
    if P == 24:
        assert O.categorical_fast_cdf(np.array([t, 0, 0], F), 24).tolist() == [0, 0, 1, total]
        assert O.categorical_fast_cdf(np.array([0, 0, t, 4 * t, 0, 9 * t], F), 24).tolist() == [0, 1, 2, 2, 3, 4, total]


@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_kind_is_in_every_batch(case, P):
    quant, k, dtype = case
    z = Z.zoo(quant, k, dtype, P)
    for bt in (Z.rect_batch(quant, k, dtype, P), Z.ragged_batch(quant, k, dtype, P)):
        seen = {kind for kinds in bt.kinds for kind in kinds if kind is not None}
        assert seen == set(z.rows), set(z.rows) - seen
        # a refused row only in the streams listed for it, one each; an empty interval is coded only in the streams listed for it
        assert {bt.kinds[s][col] for s, col in bt.refused.items()} == set(z.refused)
        for s, (sym, tables, kinds) in enumerate(zip(bt.syms, bt.tables, bt.kinds)):
            held = [j for j, kind in enumerate(kinds) if kind in z.refused]
            assert held == ([bt.refused[s]] if s in bt.refused else []), s
            width = np.array([int(t[x + 1]) - int(t[x]) for t, x in zip(tables, sym)])
            empty = [j for j in np.flatnonzero(width <= 0) if j not in held]
            assert empty == ([bt.failing[s]] if s in bt.failing else []), s
            assert (sym >= 0).all() and (sym < k).all()
        assert set(bt.refused).isdisjoint(bt.failing)
        assert bool(bt.failing) == ("degenerate" in z.classes.values())
        assert len(bt.good) >= 40 and any(s >= 64 for s in bt.good) and any(s >= 64 for s in bt.bad)      # in both waves
    # rectangular: every accepted kind meets every choice of symbol in a stream that codes
    bt = Z.rect_batch(quant, k, dtype, P)
    met = {(bt.kinds[s][j], bt.choices[s][j]) for s in bt.good for j in range(Z.N_PER)}
    assert {(kind, ch) for kind in z.accepted for ch in range(4)} <= met
    # ragged: every accepted kind directly in front of and directly behind a jump point, in streams that code
    bt = Z.ragged_batch(quant, k, dtype, P)
    assert sorted(set(bt.lengths)) == [0, 1, 2, 15, 16, 17, 33, 49, 300]
    before = {bt.kinds[s][j] for s in bt.good for j in range(Z.JUMP_EVERY - 1, bt.lengths[s] - 1, Z.JUMP_EVERY)}
    after = {bt.kinds[s][j] for s in bt.good for j in range(Z.JUMP_EVERY, bt.lengths[s], Z.JUMP_EVERY)}
    assert set(z.accepted) <= before and set(z.accepted) <= after


# ---------------------------------------------------------------------------------------------- the host twins

@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_twins_give_the_oracles_rows_and_bad_codes(lib, case, P):
    """every row of both batches -- the hard rows, a refused row's in-band form, the fillers -- and the hard rows on their own"""
    quant, k, dtype = case
    z = Z.zoo(quant, k, dtype, P)
    bad_row = [0xFFFFFFFF] + [1 << P] * k
    for bt in (Z.rect_batch(quant, k, dtype, P), Z.ragged_batch(quant, k, dtype, P)):
        _, probs = bt.flat()
        want = np.concatenate(bt.tables)
        if quant == "fast":
            rows, codes = host_fast(lib, probs, P)
        else:
            rows, codes, moves = R.host_perfect(lib, probs, P)
            assert int(moves.max()) < R.move_cap(k) // 4
            assert (moves[codes != 0] == 0).all()
        refused = (want[:, 0] == 0xFFFFFFFF)
        assert refused.sum() == len(bt.refused)
        assert codes.tolist() == refused.astype(np.int32).tolist()
        assert np.array_equal(rows, want)
    kinds = list(z.rows)
    probs = np.stack([z.rows[kind] for kind in kinds])
    rows, codes = host_fast(lib, probs, P) if quant == "fast" else R.host_perfect(lib, probs, P)[:2]
    for r, kind in enumerate(kinds):
        assert codes[r] == (z.classes[kind] == "refused"), kind
        assert rows[r].tolist() == (bad_row if z.tables[kind] is None else z.tables[kind].tolist()), kind


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_same_infinite_scale_values_in_f32_and_f64_through_the_perfect_twin(lib, dtype):
    """the f64 infinite-scale rows are refused through `extra > left`; the f32 rows of the same names are accepted"""
    for k in (5, 64, 257):
        z = Z.zoo("perfect", k, dtype, 24)
        kinds = ["min_normal_sum", "inf_scale_equal", "inf_scale_gaps"]
        _, codes, _ = R.host_perfect(lib, np.stack([z.rows[kind] for kind in kinds]), 24)
        assert codes.tolist() == ([0, 0, 0] if dtype == "f32" else [1, 1, 1])
        assert [z.classes[kind] == "refused" for kind in kinds] == [dtype == "f64"] * 3


# ---------------------------------------------------------------------------------------------- the oracle's own consistency

@pytest.mark.parametrize("P", [24, 12])
@pytest.mark.parametrize("model", Z.MODELS, ids=Z.model_id)
def test_the_lazy_model_agrees_with_the_table_on_degenerate_rows(model, P):
    k, dtype = model
    z = Z.zoo("fast", k, dtype, P)
    rng = np.random.default_rng(k + P)
    degenerate = [kind for kind, c in z.classes.items() if c == "degenerate"]
    assert degenerate
    for kind in degenerate:
        table, lazy, tab = z.tables[kind], O.LazyCategoricalModel(z.rows[kind], P), O.TableModel(z.tables[kind], 0, P)
        for i in range(k):
            assert lazy.lcp(i) == (int(table[i]), int(table[i + 1]) - int(table[i])), (kind, i)
        edges = np.unique(np.concatenate([table[:-1], table[:-1] + 1, table[1:] - 1]).astype(np.int64))
        quantiles = np.concatenate([edges[(edges >= 0) & (edges < 1 << P)], rng.integers(0, 1 << P, 64)])
        for q in quantiles[:: max(1, len(quantiles) // 400)]:
            assert lazy.quantile(int(q)) == tab.quantile(int(q)), (kind, int(q))


@pytest.mark.parametrize("cfg", Z.PRESETS, ids=Z.cfg_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_oracle_coders_round_trip_every_stream_that_codes(case, cfg):
    quant, k, dtype = case
    for shape in ("rect", "ragged"):
        bt, want = Z.expected(shape, quant, k, dtype, cfg)
        _, chunked = Z.expected(shape, quant, k, dtype, cfg, Z.JUMP_EVERY)
        assert bt.expected_status().count(Z.IMPOSSIBLE) == len(bt.bad)
        for coder in ("ans", "range"):
            for s in range(len(bt.lengths)):
                if s in bt.bad:
                    assert want[coder][s] is None and chunked[coder][s] is None
                    continue
                words = want[coder][s]
                assert Z.oracle_decode(coder, cfg, words, bt.models(s)).tolist() == bt.syms[s].tolist(), (shape, coder, s)
                # coded chunk by chunk for the jump table: the same words, one entry per chunk
                w16, table = chunked[coder][s]
                assert w16.tolist() == words.tolist() and len(table) == -(-bt.lengths[s] // Z.JUMP_EVERY), (shape, coder, s)
