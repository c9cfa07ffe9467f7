#!/usr/bin/env python3
"""Exponential-Golomb symbol codes on the C2 workload (65 536 streams x 4096 symbols): the quantized Gaussian's symbols of bench.py
folded to unsigned (zigzag: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...), as uint8 and as int32, both semantics, next to the Huffman calls
on the same matrix in the same run (the codebook of scripts/bench_huffman.py: the Gaussian's probabilities, in the folded order).
Then the ragged pair on the 100 000 documents of 20 .. 2000 symbols that scripts/bench_ragged.py draws.
Every time is the median of REPEATS event timings (each the median of 20 launches); `spread_ms` is their min .. max.
Prints one JSON line per measurement.
usage: bench_exp_golomb.py [n_streams] [n_per_stream]"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import batched as B

REPEATS = 5
n, k = (int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_STREAMS), (int(sys.argv[2]) if len(sys.argv) > 2 else bench.N_PER)
P = bench.P
m = B.Model.quantized_gaussian(bench.LO, bench.HI, bench.MEAN, bench.STD, P)
cdf = m.cdf().astype(np.int64)
sym = bench.synth_symbols_device(bench.SEED, 0, n, k, bench.LO, torch.from_numpy(cdf).cuda(), P)
folded32 = torch.where(sym >= 0, 2 * sym, -2 * sym - 1).to(torch.int32).contiguous()
folded8 = folded32.to(torch.uint8)
n_sym = n * k
values = np.arange(bench.LO, bench.HI + 1)
fold = np.where(values >= 0, 2 * values, -2 * values - 1)
probs = np.zeros(fold.max() + 1)
probs[fold] = np.diff(cdf).astype(np.float64) / (1 << P)
book = B.HuffmanCodebook.from_probabilities(probs)


def line(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    t = sorted(bench.event_ms(fn, 20) for _ in range(REPEATS))
    return round(t[len(t) // 2], 4), [round(t[0], 4), round(t[-1], 4)]


def name(dtype):
    return str(dtype).replace("torch.", "")


for s in (folded8, folded32):
    for semantics in ("stack", "queue"):
        # the two coders alternate, so that drift of the shared machine hits both
        eg = B.exp_golomb_encode(s, semantics)
        hf = B.huffman_encode(s, book, semantics)
        rows = {}
        for what, enc, dec, out in (("exp_golomb", lambda: B.exp_golomb_encode(s, semantics, out=eg),
                                     lambda: B.exp_golomb_decode(eg, k, dtype=s.dtype), eg),
                                    ("huffman", lambda: B.huffman_encode(s, book, semantics, out=hf),
                                     lambda: B.huffman_decode(hf, book, k, dtype=s.dtype), hf)):
            e, e_spread = timed(enc)
            ek = B.last_kernel()
            d, d_spread = timed(dec)
            dk = B.last_kernel()
            got, status = dec()
            ok = bool(torch.equal(got, s)) and bool((status == 0).all()) and bool((out.status == 0).all())
            rows[what] = dict(what=f"{what}_c2_folded", semantics=semantics, symbols=name(s.dtype), encode_ms=e, encode_spread_ms=e_spread,
                              decode_ms=d, decode_spread_ms=d_spread, encode_kernel=ek, decode_kernel=dk,
                              bits_per_symbol=round(int(out.n_bits.sum()) / n_sym, 4), stride_words=out.words.shape[1], ok=ok)
        c, c_spread = timed(lambda: B.exp_golomb_count_bits(s))
        rows["exp_golomb"].update(count_bits_ms=c, count_bits_spread_ms=c_spread)
        for r in rows.values():
            line(**r)
        del eg, hf

# the ragged pair: the documents of scripts/bench_ragged.py (same generator, same order of draws)
rng = np.random.default_rng(1)
n_docs, n_alphabet = 100_000, 64
doc_probs = rng.dirichlet(np.ones(n_alphabet) * 0.5)
lengths = np.exp(rng.uniform(np.log(20), np.log(2000), n_docs)).astype(np.int64)
offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).cuda()
flat32 = torch.from_numpy(rng.choice(n_alphabet, size=int(lengths.sum()), p=doc_probs).astype(np.int32)).cuda()
for flat in (flat32, flat32.to(torch.uint8)):
    for semantics in ("stack", "queue"):
        batch = B.exp_golomb_encode_ragged(flat, offsets, semantics)
        out = torch.empty_like(flat)
        e, e_spread = timed(lambda: B.exp_golomb_encode_ragged(flat, offsets, semantics))
        d, d_spread = timed(lambda: B.exp_golomb_decode_ragged(batch, offsets, out=out))
        got, status = B.exp_golomb_decode_ragged(batch, offsets, out=out)
        ok = bool(torch.equal(got, flat)) and bool((status == 0).all()) and bool((batch.status == 0).all())
        line(what="exp_golomb_ragged", semantics=semantics, symbols=name(flat.dtype), documents=n_docs, total_symbols=int(flat.numel()),
             encode_ms=e, encode_spread_ms=e_spread, decode_ms=d, decode_spread_ms=d_spread,
             bits_per_symbol=round(int(batch.n_bits.sum()) / flat.numel(), 4), words=int(batch.word_offsets[-1]), ok=ok,
             note="encode includes the count pass, the prefix sum of the slabs and its read-back")
