#!/usr/bin/env python3
"""What `--select N` of scripts/bench_exp_golomb.py and scripts/bench_huffman.py --ragged measures: random access
into a ragged batch of a symbol code against decoding everything and gathering.  Not a program of its own.

For one batch (encoded with a jump table every `interval` symbols, and without one) the calls take turns, REPEATS event timings
of 20 launches each:
  docs_*    N whole documents drawn at random: select with the table, select without it, and the full jump decode followed by a
            torch gather of the same symbols (the gather's index is built once, outside the timing);
  ranges_*  N ranges of 64 symbols at random depths of documents that have 64: the same three;
  all_*     every document through select against the jump decoder: the cost of the piece indirection;
  fixed     one query of one symbol: launches, prefix sums and the read-back of a call."""
import numpy as np
import torch

import bench

REPEATS = 5


def timed_alternating(calls):
    """{name: fn} -> {name: (median ms, [min, max])}, the calls taking turns"""
    t = {name: [] for name in calls}
    for _ in range(REPEATS):
        for name, fn in calls.items():
            t[name].append(bench.event_ms(fn, 20))
    return {name: (round(sorted(v)[len(v) // 2], 4), [round(min(v), 4), round(max(v), 4)]) for name, v in t.items()}


def gather_index(offsets, streams, first, count):
    """flat positions of the symbols the queries ask for, in query order (device int64)"""
    starts = offsets[streams] + first
    out_offsets = torch.zeros(count.numel() + 1, dtype=torch.int64, device=count.device)
    torch.cumsum(count, 0, out=out_offsets[1:])
    total = int(out_offsets[-1])
    owner = torch.repeat_interleave(torch.arange(count.numel(), device=count.device), count, output_size=total)
    return starts[owner] + (torch.arange(total, device=count.device) - out_offsets[owner])


def select_rows(flat, offsets, with_table, without_table, decode, select, n_select, seed=5):
    """`decode(batch, out)` decodes everything, `select(batch, streams, first, count, out)` the queries -> one dict of timings"""
    rng = np.random.default_rng(seed)
    lengths = (offsets[1:] - offsets[:-1]).cpu().numpy()
    n_docs = lengths.size
    docs = torch.from_numpy(rng.integers(0, n_docs, n_select)).cuda()
    deep = np.flatnonzero(lengths >= 64)
    r_docs_h = deep[rng.integers(0, deep.size, n_select)]
    r_first = torch.from_numpy(rng.integers(0, lengths[r_docs_h] - 64 + 1)).cuda()
    r_docs = torch.from_numpy(r_docs_h).cuda()
    r_count = torch.full_like(r_first, 64)
    everyone = torch.arange(n_docs, device="cuda")
    full = torch.empty_like(flat)
    zero = torch.zeros_like(docs)
    idx_docs = gather_index(offsets, docs, zero, lengths_t(offsets)[docs])
    idx_ranges = gather_index(offsets, r_docs, r_first, r_count)
    out_docs, out_ranges, out_one = torch.empty_like(flat[: idx_docs.numel()]), torch.empty_like(flat[: idx_ranges.numel()]), torch.empty_like(flat[:4])
    one = torch.tensor([int(deep[0])], device="cuda")

    def decode_gather(idx):
        return decode(with_table, full)[0][idx]

    t = timed_alternating({
        "docs_select_table": lambda: select(with_table, docs, None, None, out_docs),
        "docs_select_plain": lambda: select(without_table, docs, None, None, out_docs),
        "docs_decode_gather": lambda: decode_gather(idx_docs),
        "ranges_select_table": lambda: select(with_table, r_docs, r_first, r_count, out_ranges),
        "ranges_select_plain": lambda: select(without_table, r_docs, r_first, r_count, out_ranges),
        "ranges_decode_gather": lambda: decode_gather(idx_ranges),
        "all_select_table": lambda: select(with_table, everyone, None, None, full),
        "all_decode_jump": lambda: decode(with_table, full),
        "fixed": lambda: select(with_table, one, one * 0, one * 0 + 1, out_one)})
    ok = True
    for batch in (with_table, without_table):
        for streams, first, count, idx in ((docs, None, None, idx_docs), (r_docs, r_first, r_count, idx_ranges)):
            got, _, status = select(batch, streams, first, count, None)
            ok = ok and bool(torch.equal(got, flat[idx])) and bool((status == 0).all())
    got, _, status = select(with_table, everyone, None, None, None)
    ok = ok and bool(torch.equal(got, flat)) and bool((status == 0).all())
    row = dict(queries=n_select, selected_symbols=int(idx_docs.numel()), range_symbols=int(idx_ranges.numel()), ok=ok)
    for name, (ms, spread) in t.items():
        row[name + "_ms"], row[name + "_spread_ms"] = ms, spread
    row["docs_gather_over_select"] = round(t["docs_decode_gather"][0] / t["docs_select_table"][0], 3)
    row["ranges_gather_over_select"] = round(t["ranges_decode_gather"][0] / t["ranges_select_table"][0], 3)
    row["all_select_over_decode"] = round(t["all_select_table"][0] / t["all_decode_jump"][0], 3)
    return row


def lengths_t(offsets):
    return offsets[1:] - offsets[:-1]
