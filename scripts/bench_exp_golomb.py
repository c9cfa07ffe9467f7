#!/usr/bin/env python3
"""Exponential-Golomb symbol codes on the C2 workload (65 536 streams x 4096 symbols): the quantized Gaussian's symbols of bench.py
folded to unsigned (zigzag: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...), as uint8 and as int32, both semantics, next to the Huffman calls
on the same matrix in the same run (the codebook of scripts/bench_huffman.py: the Gaussian's probabilities, in the folded order).
Then the ragged pair on the 100 000 documents of 20 .. 2000 symbols that scripts/bench_ragged.py draws.
Every time is the median of REPEATS event timings (each the median of 20 launches); `spread_ms` is their min .. max.
Prints one JSON line per measurement.
usage: bench_exp_golomb.py [n_streams] [n_per_stream]

bench_exp_golomb.py --jump-every I [--select N]: the ragged mode alone, with jump points, on those 100 000 documents
and on 100 000 documents of 200 symbols, int32 and uint8, both semantics: exp_golomb_encode_ragged plain and with jump_every=I (the
calls, and the two encoder kernels alone through the C ABI into buffers that exist), exp_golomb_decode_ragged plain and through
the table; the calls of a row take turns.  With --select N also scripts/bench_symbol_select.py's measurements on every batch: N
whole documents and N ranges of 64 symbols through exp_golomb_decode_ragged_select against the full jump decode and a gather."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import batched as B

REPEATS = 5


def flag(name):
    """--name VALUE out of sys.argv -> int, or None"""
    if name not in sys.argv:
        return None
    i = sys.argv.index(name)
    value = int(sys.argv[i + 1])
    del sys.argv[i: i + 2]
    return value


def ragged_jump(jump_every, n_select, n_docs=100_000):
    from constriction_amd import _native as N
    from bench_symbol_select import select_rows, timed_alternating
    rng = np.random.default_rng(1)          # the generator and the order of draws of scripts/bench_ragged.py
    n_alphabet = 64
    doc_probs = rng.dirichlet(np.ones(n_alphabet) * 0.5)
    lengths = np.exp(rng.uniform(np.log(20), np.log(2000), n_docs)).astype(np.int64)
    for batch_name, lens in (("20..2000", lengths), ("200", np.full(n_docs, 200, dtype=np.int64))):
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
        flat32 = torch.from_numpy(rng.choice(n_alphabet, size=int(lens.sum()), p=doc_probs).astype(np.int32)).cuda()
        for flat in (flat32, flat32.to(torch.uint8)):
            for semantics in ("stack", "queue"):
                plain = B.exp_golomb_encode_ragged(flat, offsets, semantics)
                jump = B.exp_golomb_encode_ragged(flat, offsets, semantics, jump_every=jump_every)
                out = torch.empty_like(flat)
                sem, sb, ptr = N.SYMBOL_STACK if semantics == "stack" else N.SYMBOL_QUEUE, flat.element_size(), B._ptr
                tab = jump.jump

                def encode_kernel():
                    N.check(N.lib().cst_exp_golomb_encode_ragged(sem, ptr(flat), sb, ptr(offsets), n_docs, ptr(plain.words),
                                                                 ptr(plain.word_offsets), 0, ptr(plain.n_words), ptr(plain.n_bits),
                                                                 ptr(plain.status), B._stream_ptr()))

                def encode_jump_kernel():
                    N.check(N.lib().cst_exp_golomb_encode_ragged_jump(sem, ptr(flat), sb, ptr(offsets), n_docs, ptr(jump.words),
                                                                      ptr(jump.word_offsets), 0, ptr(jump.n_words), ptr(jump.n_bits),
                                                                      tab.interval, ptr(tab.chunk_offsets), ptr(tab.bits), ptr(jump.status),
                                                                      B._stream_ptr()))

                t = timed_alternating({
                    "encode_kernel": encode_kernel, "encode_jump_kernel": encode_jump_kernel,
                    "encode": lambda: B.exp_golomb_encode_ragged(flat, offsets, semantics),
                    "encode_jump": lambda: B.exp_golomb_encode_ragged(flat, offsets, semantics, jump_every=jump_every),
                    "decode": lambda: B.exp_golomb_decode_ragged(plain, offsets, out=out),
                    "decode_jump": lambda: B.exp_golomb_decode_ragged(jump, offsets, out=out)})
                ok = bool(torch.equal(plain.n_words, jump.n_words)) and bool(torch.equal(plain.n_bits, jump.n_bits))
                for batch in (plain, jump):
                    out.zero_()
                    got, status = B.exp_golomb_decode_ragged(batch, offsets, out=out)
                    ok = ok and bool(torch.equal(got, flat)) and bool((status == 0).all()) and bool((batch.status == 0).all())
                row = dict(what="exp_golomb_ragged_jump", batch=batch_name, semantics=semantics, symbols=name(flat.dtype), documents=n_docs,
                           total_symbols=int(flat.numel()), jump_every=jump_every, chunks=int(tab.chunk_offsets[-1]), ok=ok,
                           bits_per_symbol=round(int(plain.n_bits.sum()) / flat.numel(), 4))
                for key, (ms, spread) in t.items():
                    row[key + "_ms"], row[key + "_spread_ms"] = ms, spread
                row["decode_plain_over_jump"] = round(t["decode"][0] / t["decode_jump"][0], 3)
                row["encode_jump_over_plain"] = round(t["encode_jump"][0] / t["encode"][0], 3)
                row["encode_jump_kernel_over_plain"] = round(t["encode_jump_kernel"][0] / t["encode_kernel"][0], 3)
                line(**row)
                if n_select:
                    line(what="exp_golomb_ragged_select", batch=batch_name, semantics=semantics, symbols=name(flat.dtype), documents=n_docs,
                         jump_every=jump_every,
                         **select_rows(flat, offsets, jump, plain, lambda b, o: B.exp_golomb_decode_ragged(b, offsets, out=o),
                                       lambda b, s, f, c, o: B.exp_golomb_decode_ragged_select(b, offsets, s, f, c, out=o), n_select))
                del plain, jump, out


def line(**kw):
    print(json.dumps(kw), flush=True)


def name(dtype):
    return str(dtype).replace("torch.", "")


JUMP_EVERY, SELECT = flag("--jump-every"), flag("--select")
if JUMP_EVERY is not None or SELECT is not None:
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    ragged_jump(JUMP_EVERY or B.RAGGED_JUMP_EVERY, SELECT or 0)
    sys.exit(0)

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


def timed(fn):
    t = sorted(bench.event_ms(fn, 20) for _ in range(REPEATS))
    return round(t[len(t) // 2], 4), [round(t[0], 4), round(t[-1], 4)]


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
