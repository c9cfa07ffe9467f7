"""CPU-only: what tests/test_gpu_range_per_stream.py compares the per-stream range coder with is itself sound -- the generated rows are
valid tables, the oracle codes every stream of every case without an error and within range_max_words (a comparison with it can
never be vacuous), the capacity case really has streams on both sides of its stride, and the header still documents every entry
point the Python binding binds."""
import numpy as np
import pytest

import per_stream_rows as R
from test_abi import declared_symbols

ALL = [(case, shape) for case in R.CASES for shape in R.SHAPES]
W16 = [(case, shape) for case in R.W16_CASES for shape in R.W16_SHAPES]


@pytest.mark.parametrize("case", list(R.CASES))
def test_generated_rows_are_valid_tables(case):
    n, P = R.CASES[case]
    for n_streams, n_per in R.SHAPES:
        lo, P_, cdfs, sym = R.batch(case, n_streams, n_per)
        assert P_ == P and cdfs.shape == (n_streams, n + 1) and cdfs.dtype == np.uint32
        assert R.rows_are_valid(cdfs, P)
        assert sym.shape == (n_streams, n_per) and sym.min() >= lo and sym.max() <= lo + n - 1
        if n_per >= 4:          # the first and last two symbols of the support are in every stream
            assert (sym[:, :4] == np.array([lo, lo + n - 1, lo + 1, lo + n - 2])).all()


@pytest.mark.parametrize("case,shape", ALL, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_oracle_codes_every_stream(case, shape):
    from oracle import oracle as O
    presets = [(32, 64)] + ([(16, 32)] if (case, shape) in W16 else [])
    lo, P, cdfs, sym = R.batch(case, *shape)
    for W, S in presets:
        words, n_words, status = R.oracle_encode(case, *shape, W, S)
        assert (status == 0).all()
        assert (n_words <= O.range_max_words(shape[1], P, W, S)).all() and (n_words > 0).all()
        if shape[0] * shape[1] <= 130 * 100:        # (the oracle's own round trip, where it is cheap)
            back, bstatus = R.oracle_decode(words, n_words, shape[1], lo, cdfs, P, W, S)
            assert (bstatus == 0).all() and np.array_equal(back, sym)


def test_capacity_case_has_streams_on_both_sides():
    _, n_words, status = R.oracle_encode(*R.CAPACITY_CASE)
    stride = R.capacity_stride()
    assert (status == 0).all()
    assert (n_words > stride).any() and (n_words <= stride).any()


def test_header_documents_every_bound_entry_point():
    from constriction_amd import _native
    assert sorted(_native.SIGNATURES) == declared_symbols()
