#!/usr/bin/env python3
"""Huffman symbol codes on the C2 workload (65 536 streams x 4096 symbols, the quantized Gaussian of bench.py turned into a
Huffman codebook over its 101 symbols) next to the ANS C2 pair in the same run: encode and decode for both semantics and for
int32 / uint8 symbols, the long-code kernels on a skewed codebook, bits per symbol.  Prints one JSON line per measurement.
usage: bench_huffman.py [n_streams] [n_per_stream]

bench_huffman.py --ragged [n_documents]: the ragged calls instead, on the 100 000 documents of 20 .. 2000 symbols that
scripts/bench_ragged.py draws and on 100 000 documents of 200 symbols, int32 and uint8, both semantics, the codebook fitted to the
symbols' empirical distribution: huffman_encode_ragged plain and with jump_every=256, huffman_decode_ragged plain and through the
table, and the Exp-Golomb ragged pair on the same symbols.  The calls of one row alternate, so that drift of a shared machine hits
all of them; every time is the median of REPEATS event timings (each the median of 20 launches), `*_spread_ms` their min .. max.
The encode calls include their count pass, the prefix sum of the slabs and its read-back; `encode_kernel` / `encode_jump_kernel`
are the two encoder kernels alone, through the C ABI into buffers that exist.

bench_huffman.py --ragged --select N [n_documents]: on the same batches only scripts/bench_symbol_select.py's measurements (DESIGN.md
4.28): N whole documents and N ranges of 64 symbols through huffman_decode_ragged_select, with the table and without, against the
full jump decode and a gather."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import _native as N
from constriction_amd import batched as B



def line(**kw):
    print(json.dumps(kw), flush=True)


REPEATS = 5
JUMP_EVERY = 256


def timed_alternating(calls):
    """{name: fn} -> {name: (median ms, [min, max])}, the calls taking turns"""
    t = {name: [] for name in calls}
    for _ in range(REPEATS):
        for name, fn in calls.items():
            t[name].append(bench.event_ms(fn, 20))
    return {name: (round(sorted(v)[len(v) // 2], 4), [round(min(v), 4), round(max(v), 4)]) for name, v in t.items()}


def ragged(n_docs, n_select=0):
    rng = np.random.default_rng(1)          # the generator and the order of draws of scripts/bench_ragged.py
    n_alphabet = 64
    doc_probs = rng.dirichlet(np.ones(n_alphabet) * 0.5)
    lengths = np.exp(rng.uniform(np.log(20), np.log(2000), n_docs)).astype(np.int64)
    for batch_name, lens in (("20..2000", lengths), ("200", np.full(n_docs, 200, dtype=np.int64))):
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
        host = rng.choice(n_alphabet, size=int(lens.sum()), p=doc_probs).astype(np.int32)
        book = B.HuffmanCodebook.from_probabilities(np.bincount(host, minlength=n_alphabet) / host.size)
        flat32 = torch.from_numpy(host).cuda()
        for flat in (flat32, flat32.to(torch.uint8)):
            for semantics in ("stack", "queue"):
                plain = B.huffman_encode_ragged(flat, offsets, book, semantics)
                jump = B.huffman_encode_ragged(flat, offsets, book, semantics, jump_every=JUMP_EVERY)
                if n_select:
                    from bench_symbol_select import select_rows
                    line(what="huffman_ragged_select", batch=batch_name, semantics=semantics, symbols=str(flat.dtype).replace("torch.", ""),
                         documents=n_docs, jump_every=JUMP_EVERY,
                         **select_rows(flat, offsets, jump, plain, lambda b, o: B.huffman_decode_ragged(b, book, offsets, out=o),
                                       lambda b, s, f, c, o: B.huffman_decode_ragged_select(b, book, offsets, s, f, c, out=o), n_select))
                    del plain, jump
                    continue
                eg = B.exp_golomb_encode_ragged(flat, offsets, semantics)
                out = torch.empty_like(flat)
                # the two encoder kernels alone, into the batches' own buffers (no count pass, no prefix sums, no allocation)
                sem, sb, ptr = N.HUFFMAN_STACK if semantics == "stack" else N.HUFFMAN_QUEUE, flat.element_size(), B._ptr
                tab = jump.jump

                def encode_kernel():
                    N.check(N.lib().cst_huffman_encode_ragged(book._h, sem, ptr(flat), sb, ptr(offsets), n_docs, ptr(plain.words),
                                                              ptr(plain.word_offsets), 0, ptr(plain.n_words), ptr(plain.n_bits),
                                                              ptr(plain.status), B._stream_ptr()))

                def encode_jump_kernel():
                    N.check(N.lib().cst_huffman_encode_ragged_jump(book._h, sem, ptr(flat), sb, ptr(offsets), n_docs, ptr(jump.words),
                                                                   ptr(jump.word_offsets), 0, ptr(jump.n_words), ptr(jump.n_bits),
                                                                   tab.interval, ptr(tab.chunk_offsets), ptr(tab.bits), ptr(jump.status),
                                                                   B._stream_ptr()))

                t = timed_alternating({
                    "encode_kernel": encode_kernel, "encode_jump_kernel": encode_jump_kernel,
                    "encode": lambda: B.huffman_encode_ragged(flat, offsets, book, semantics),
                    "encode_jump": lambda: B.huffman_encode_ragged(flat, offsets, book, semantics, jump_every=JUMP_EVERY),
                    "exp_golomb_encode": lambda: B.exp_golomb_encode_ragged(flat, offsets, semantics),
                    "decode": lambda: B.huffman_decode_ragged(plain, book, offsets, out=out),
                    "decode_jump": lambda: B.huffman_decode_ragged(jump, book, offsets, out=out),
                    "exp_golomb_decode": lambda: B.exp_golomb_decode_ragged(eg, offsets, out=out)})
                ok = bool(torch.equal(plain.n_words, jump.n_words)) and bool(torch.equal(plain.n_bits, jump.n_bits))
                for batch, dec in ((plain, B.huffman_decode_ragged), (jump, B.huffman_decode_ragged)):
                    out.zero_()
                    got, status = dec(batch, book, offsets, out=out)
                    ok = ok and bool(torch.equal(got, flat)) and bool((status == 0).all()) and bool((batch.status == 0).all())
                row = dict(what="huffman_ragged", batch=batch_name, semantics=semantics, symbols=str(flat.dtype).replace("torch.", ""),
                           documents=n_docs, total_symbols=int(flat.numel()), jump_every=JUMP_EVERY,
                           chunks=int(jump.jump.chunk_offsets[-1]), ok=ok,
                           bits_per_symbol=round(int(plain.n_bits.sum()) / flat.numel(), 4),
                           exp_golomb_bits_per_symbol=round(int(eg.n_bits.sum()) / flat.numel(), 4))
                for name, (ms, spread) in t.items():
                    row[name + "_ms"], row[name + "_spread_ms"] = ms, spread
                row["decode_plain_over_jump"] = round(t["decode"][0] / t["decode_jump"][0], 3)
                row["encode_jump_over_plain"] = round(t["encode_jump"][0] / t["encode"][0], 3)
                row["encode_jump_kernel_over_plain"] = round(t["encode_jump_kernel"][0] / t["encode_kernel"][0], 3)
                line(**row)
                del plain, jump, eg, out


if "--ragged" in sys.argv:
    rest = [a for a in sys.argv[1:] if a != "--ragged"]
    n_select = 0
    if "--select" in rest:
        i = rest.index("--select")
        n_select = int(rest[i + 1])
        del rest[i: i + 2]
        sys.path.insert(0, str(Path(__file__).resolve().parent))
    ragged(int(rest[0]) if rest else 100_000, n_select)
    sys.exit(0)

n, k = (int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_STREAMS), (int(sys.argv[2]) if len(sys.argv) > 2 else bench.N_PER)
P = bench.P
m = B.Model.quantized_gaussian(bench.LO, bench.HI, bench.MEAN, bench.STD, P)
cdf = m.cdf().astype(np.int64)
sym = bench.synth_symbols_device(bench.SEED, 0, n, k, bench.LO, torch.from_numpy(cdf).cuda(), P)
idx32 = (sym - bench.LO).contiguous()
idx8 = idx32.to(torch.uint8)
n_sym = n * k

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
