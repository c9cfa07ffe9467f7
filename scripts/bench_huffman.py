#!/usr/bin/env python3
"""Huffman symbol codes on the C2 workload (65 536 streams x 4096 symbols, the quantized Gaussian of bench.py turned into a
Huffman codebook over its 101 symbols) next to the ANS C2 pair in the same run: encode and decode for both semantics and for
int32 / uint8 symbols, the long-code kernels on a skewed codebook, bits per symbol.  Prints one JSON line per measurement.
usage: bench_huffman.py [n_streams] [n_per_stream]"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import batched as B

n, k = (int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_STREAMS), (int(sys.argv[2]) if len(sys.argv) > 2 else bench.N_PER)
P = bench.P
m = B.Model.quantized_gaussian(bench.LO, bench.HI, bench.MEAN, bench.STD, P)
cdf = m.cdf().astype(np.int64)
sym = bench.synth_symbols_device(bench.SEED, 0, n, k, bench.LO, torch.from_numpy(cdf).cuda(), P)
idx32 = (sym - bench.LO).contiguous()
idx8 = idx32.to(torch.uint8)
n_sym = n * k


def line(**kw):
    print(json.dumps(kw), flush=True)


# the ANS C2 pair, as bench.py runs it
enc = B.ans_encode(sym, m, (32, 64, P))
dec = torch.empty_like(sym)
e = bench.event_ms(lambda: B.ans_encode(sym, m, (32, 64, P), out=enc), 20)
d = bench.event_ms(lambda: B.ans_decode(enc, m, k, out=dec), 20)
B.ans_decode(enc, m, k, out=dec)
line(what="ans_c2", encode_ms=round(e, 4), decode_ms=round(d, 4), bits_per_symbol=round(32 * enc.total_words() / n_sym, 4),
     ok=bool(torch.equal(dec, sym)))

probs = np.diff(cdf).astype(np.float64) / (1 << P)
cb = B.HuffmanCodebook.from_probabilities(probs)
skewed = B.HuffmanCodebook.from_probabilities(np.array([2.0 ** -i for i in range(1, 61)] + [2.0 ** -60]))   # codewords 1 .. 60 bits
# symbols of the skewed codebook: the C2 indices folded onto 0..60 (most of them short, the tails up to 60 bits)
skew_sym = torch.clamp((idx32 - 50).abs(), max=60).to(torch.int32).contiguous()

for name, book, s in (("c2", cb, idx32), ("c2", cb, idx8), ("skewed", skewed, skew_sym)):
    for semantics in ("stack", "queue"):
        out = B.huffman_encode(s, book, semantics)
        e = bench.event_ms(lambda: B.huffman_encode(s, book, semantics, out=out), 20)
        ek = B.last_kernel()
        d = bench.event_ms(lambda: B.huffman_decode(out, book, k, dtype=s.dtype), 20)
        dk = B.last_kernel()
        got, status = B.huffman_decode(out, book, k, dtype=s.dtype)
        ok = bool(torch.equal(got, s)) and bool((status == 0).all()) and bool((out.status == 0).all())
        line(what=f"huffman_{name}", semantics=semantics, symbols=str(s.dtype).replace("torch.", ""), encode_ms=round(e, 4),
             decode_ms=round(d, 4), encode_kernel=ek, decode_kernel=dk,
             bits_per_symbol=round(int(out.n_bits.sum()) / n_sym, 4), stride_words=out.words.shape[1], ok=ok)
