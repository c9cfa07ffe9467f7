"""CPU-only: what tests/test_gpu_ragged_per_stream.py compares the ragged per-stream coders with is itself sound -- the helper's rows are
valid tables, the oracle codes every document of every case ALONE under its own row without an error, inside the slab the binding
allocates for it, and back to its symbols; a chunk of a jump table decodes alone to its own symbols; and the header says which ragged
entry points take a model with one table per stream and which still refuse one."""
import re
from pathlib import Path

import numpy as np
import pytest

import ragged_per_stream_rows as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "constriction_amd.h"

SMALL = [(case, n) for case in R.PARITY_CASES for n in (1, 65)]


@pytest.mark.parametrize("case", R.PARITY_CASES)
def test_generated_rows_are_valid_tables(case):
    n, P = R.CASES[case]
    for n_streams in R.STREAM_COUNTS:
        lo, P_, cdfs, docs, offsets = R.batch(case, n_streams)
        assert P_ == P and cdfs.shape == (n_streams, n + 1) and cdfs.dtype == np.uint32
        assert R.rows_are_valid(cdfs, P)
        lengths = R.lengths_of(n_streams)
        assert [len(d) for d in docs] == lengths.tolist() and offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
        assert R.LONG in lengths and len(docs) <= 300 and int(offsets[-1]) <= 80_000
        if n_streams >= 63:
            assert set(R.LENGTHS) <= set(lengths.tolist())
        for d in docs:
            assert d.dtype == np.int32 and (len(d) == 0 or (d.min() >= lo and d.max() <= lo + n - 1))
            if len(d) >= 4:          # the first and last two symbols of the support are in every stream that is long enough
                assert d[:4].tolist() == [lo, lo + n - 1, lo + 1, lo + n - 2]


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("case,n_streams", SMALL, ids=lambda v: str(v))
def test_oracle_round_trips_every_document_inside_its_slab(coder, case, n_streams):
    from oracle import oracle as O
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    presets = [(32, 64)] + ([(16, 32)] if case in R.W16_CASES else [])
    for W, S in presets:
        words = R.oracle_words(coder, case, n_streams, W, S)
        for s, doc in enumerate(docs):
            w = words[s]
            slab = R.ans_slab(len(doc), P, W, S) if coder == "ans" else R.range_slab(len(doc), P, W, S)
            assert len(w) <= slab, f"stream {s} of {len(doc)} symbols: {len(w)} words in a slab of {slab}"
            if coder == "ans":
                # (a document of first symbols only leaves the coder's state 0: no words, and the empty coder decodes it)
                coder_ = O.AnsCoder(w, W=W, S=S) if len(w) else O.AnsCoder(W=W, S=S)
                back = coder_.decode_iid_table(len(doc), cdfs[s], lo, P)
            else:
                out, st = O.rc_decode_batch(w[None, :] if len(w) else np.zeros((1, 1), np.uint32), np.array([len(w)], np.uint32), len(doc), lo,
                                            cdfs[s], P, W, S)
                assert int(st[0]) == 0
                back = out[0]
            assert back.tolist() == doc.tolist(), f"stream {s}"


@pytest.mark.parametrize("coder", ["ans", "range"])
@pytest.mark.parametrize("every", [8, 64, 256])
def test_a_chunk_of_a_jump_table_decodes_alone(coder, every):
    case, n_streams = "bimodal", 65
    lo, P, cdfs, docs, _ = R.batch(case, n_streams)
    words = R.oracle_words(coder, case, n_streams)
    seen = 0
    for s, doc in enumerate(docs):
        if len(doc) == 0:
            continue
        table = R.oracle_jump_table(coder, doc, lo, cdfs[s], P, every)
        n_chunks = (len(doc) + every - 1) // every
        assert all(len(t) == n_chunks for t in table)
        for j in sorted({0, n_chunks // 2, n_chunks - 1}):
            n = min(every, len(doc) - j * every)
            back, st = R.oracle_decode_chunk(coder, words[s], [t[j] for t in table], n, lo, cdfs[s], P)
            assert st == 0 and back.tolist() == doc[j * every: j * every + n].tolist(), f"stream {s}, chunk {j}"
            seen += 1
    assert seen > n_streams


def _comment_in_front_of(text, name):
    """the block comment that documents `name`: the last one that ends in front of its declaration"""
    at = re.search(r"^cst_status\s+%s\s*\(" % re.escape(name), text, re.M).start()
    comments = [m for m in re.finditer(r"/\*.*?\*/", text, re.S) if m.end() <= at]
    return comments[-1].group(0)


TAKE = ["cst_ans_encode_ragged", "cst_ans_decode_ragged", "cst_ans_encode_ragged_ordered", "cst_ans_decode_ragged_ordered",
        "cst_ans_encode_ragged_jump", "cst_ans_decode_ragged_jump", "cst_range_encode_ragged", "cst_range_decode_ragged",
        "cst_range_encode_ragged_jump", "cst_range_decode_ragged_jump"]
REFUSE = ["cst_ans_count_until", "cst_range_count_until", "cst_ans_decode_ragged_select", "cst_range_decode_ragged_select"]


@pytest.mark.parametrize("name", TAKE + REFUSE)
def test_header_says_what_becomes_of_a_per_stream_model(name):
    comment = _comment_in_front_of(HEADER.read_text(), name)
    assert re.search(r"per-stream model|table per stream", comment, re.I), f"{name}: the comment does not mention models with one table per stream"
    if name in TAKE:
        assert "n_tables" in comment and "n_streams" in comment
    else:
        assert "CST_ERR_INVALID_ARGUMENT" in comment or "refus" in comment
