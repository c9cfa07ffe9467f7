#!/usr/bin/env python3
"""Many small coders (the reference's tests/issue52.rs pattern): 100 000 documents of 20 .. 2000 symbols with one categorical
model at P = 24 through `batched.ans_{encode,decode}_ragged` (one launch each), beside the same documents one
`stream.stack.AnsCoder` each through the drop-in (a device round trip per call; 200 documents, extrapolated).
`--coder range`: the same workloads through `batched.range_{encode,decode}_ragged` (one RangeEncoder / RangeDecoder per document), with
`ans_encode_ragged(..., jump_every=0)` / `ans_decode_ragged` on the same documents in the same run beside them.
`--coder range --jump-every N`: also `range_encode_ragged_jump(..., jump_every=N)` and the decode of its chunks side by side, beside the
plain pair on the same documents in the same run; every figure is measured twice (the second run shows the spread).
`--select N [--coder range] --jump-every I`: random access on the first batch (20 .. 2000 symbols, shuffled) with a jump point every I
symbols (default 256) -- N documents drawn at random through `batched.{ans,range}_decode_ragged_select` beside the full decode of the
batch followed by a device gather of those documents, and N ranges of 64 symbols at random depths with the table and without.
`--tables per-stream [--coder range] [--jump-every I]`: 16 384 streams of 256 .. 8192 symbols (support -127 .. 127, P = 12), ONE FITTED TABLE
PER STREAM (`Model.fit_per_stream(..., sym_offsets=)`) through the ragged pair of the coder, beside (a) the shared-table ragged pair on the
same symbols and (b), on the first `--loop-streams` streams, a loop of rectangular per-stream calls, one per distinct length -- the only
route to the same words without the ragged per-stream kernels; the words of (b) are compared with the batched call's.  Writes
profiles/ragged_per_stream.json (one entry per coder and interval, merged into the file)."""
import argparse, json, sys, time
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import batched as B
from constriction_amd.stream import model as M, stack

args = argparse.ArgumentParser(description=__doc__)
args.add_argument("--coder", choices=("ans", "range"), default="ans")
args.add_argument("--jump-every", type=int, default=0, help="range coder: also time the pair with a jump point every N symbols")
args.add_argument("--select", type=int, default=0, metavar="N", help="time random access to N documents / N ranges of 64 symbols, then stop")
args.add_argument("--tables", choices=("shared", "per-stream"), default="shared", help="per-stream: one fitted table per stream, then stop")
args.add_argument("--streams", type=int, default=16384, help="--tables per-stream: streams of the batch")
args.add_argument("--loop-streams", type=int, default=512, help="--tables per-stream: streams of the subset that route (b) loops over")
opts = args.parse_args()
coder, jump_every = opts.coder, opts.jump_every
best = lambda fn: min(bench.event_ms(fn, 5) for _ in range(3))      # best of three event timings of five calls


def bench_per_stream(n_streams, n_loop, every):
    lo, hi, P, cfg = -127, 127, 12, (32, 64, 12)
    gen = torch.Generator(device="cuda").manual_seed(7)
    lengths = torch.randint(256, 8193, (n_streams,), generator=gen, device="cuda")
    off_d = torch.zeros(n_streams + 1, dtype=torch.int64, device="cuda"); torch.cumsum(lengths, 0, out=off_d[1:])
    mean = torch.rand(n_streams, generator=gen, device="cuda") * 80 - 40
    std = torch.exp(torch.rand(n_streams, generator=gen, device="cuda") * (np.log(16) - np.log(0.5)) + np.log(0.5))
    total = int(off_d[-1])
    noise = torch.randn(total, generator=gen, device="cuda")
    flat = (noise * torch.repeat_interleave(std, lengths) + torch.repeat_interleave(mean, lengths)).round().clamp(lo, hi).to(torch.int32)
    del noise
    if coder == "range":
        encode = lambda sym, off, m, I: B.range_encode_ragged_jump(sym, off, m, cfg, jump_every=I) if I else B.range_encode_ragged(sym, off, m, cfg)
        decode, rect_encode, rect_decode = B.range_decode_ragged, B.range_encode, B.range_decode
    else:
        encode = lambda sym, off, m, I: B.ans_encode_ragged(sym, off, m, cfg, jump_every=I)
        decode, rect_encode, rect_decode = B.ans_decode_ragged, B.ans_encode, B.ans_decode
    t0 = time.perf_counter()
    model = B.Model.fit_per_stream(flat, lo, hi, P, sym_offsets=off_d)
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    shared = B.Model.fit(flat, lo, hi, P)

    def pair(m, sym, off):
        enc = encode(sym, off, m, every)
        enc_name = B.last_kernel()
        dec, st = decode(enc, m, off)
        dec_name = B.last_kernel()
        ok = bool(torch.equal(dec, sym)) and int(enc.status.abs().sum()) == 0 and int(st.abs().sum()) == 0
        e = best(lambda: encode(sym, off, m, every))
        d = best(lambda: decode(enc, m, off, out=dec))
        return enc, e, d, ok, int(enc.n_words.sum()), (enc_name, dec_name)

    enc, e, d, ok, words, names = pair(model, flat, off_d)
    _, se, sd, sok, swords, snames = pair(shared, flat, off_d)
    # route (b) on a subset: one rectangular per-stream call per distinct length, the models and matrices made outside the timed region
    n_loop = min(n_loop, n_streams)
    sub_off = off_d[: n_loop + 1].clone()
    sub_flat = flat[: int(sub_off[-1])]
    rows = model.cdfs_device(0, n_loop)
    sub_model = B.Model.from_cdf_rows_per_stream(rows, lo, P)
    sub_enc, be, bd, bok, _, _ = pair(sub_model, sub_flat, sub_off)
    len_h, off_h = lengths[:n_loop].cpu().numpy(), sub_off.cpu().numpy()
    groups = []
    for n in np.unique(len_h):
        idx = np.flatnonzero(len_h == n)
        sym = torch.stack([sub_flat[off_h[s]: off_h[s] + n] for s in idx]).contiguous()
        groups.append((int(n), idx, sym, B.Model.from_cdf_rows_per_stream(rows[torch.from_numpy(idx).cuda()].contiguous(), lo, P)))
    loop_encode = lambda: [rect_encode(sym, m, cfg, jump_points=0) for _, _, sym, m in groups]
    encs = loop_encode()
    loop_decode = lambda: [rect_decode(x, m, n) for x, (n, _, _, m) in zip(encs, groups)]
    same = True
    w, wo, nw = sub_enc.words.cpu().numpy(), sub_enc.word_offsets.cpu().numpy(), sub_enc.n_words.cpu().numpy()
    for x, (n, idx, sym, m), (back, st) in zip(encs, groups, loop_decode()):
        rw, rn = x.words.cpu().numpy(), x.n_words.cpu().numpy()
        same = same and bool(torch.equal(back, sym)) and int(st.abs().sum()) == 0
        for k, s in enumerate(idx):
            same = same and rn[k] == nw[s] and np.array_equal(rw[k, : rn[k]], w[wo[s]: wo[s] + nw[s]])
    le, ld = best(loop_encode), best(loop_decode)
    result = {"coder": coder, "jump_every": every, "n_streams": n_streams, "symbols": total, "config": list(cfg), "kernels": list(names),
              "fit_per_stream_ms": round(fit_ms, 3),
              "per_stream": {"encode_ms": round(e, 4), "decode_ms": round(d, 4), "words": words, "ok": ok},
              "shared_table": {"encode_ms": round(se, 4), "decode_ms": round(sd, 4), "words": swords, "ok": sok, "kernels": list(snames)},
              "per_stream_over_shared": {"encode": round(e / se, 3), "decode": round(d / sd, 3), "words": round(words / swords, 4)},
              "subset": {"n_streams": n_loop, "symbols": int(sub_off[-1]), "rectangular_calls": len(groups),
                         "batched": {"encode_ms": round(be, 4), "decode_ms": round(bd, 4), "ok": bok},
                         "rectangular_loop": {"encode_ms": round(le, 4), "decode_ms": round(ld, 4)},
                         "loop_over_batched": {"encode": round(le / be, 2), "decode": round(ld / bd, 2)}, "same_words": bool(same)}}
    print(json.dumps(result), flush=True)
    path = Path(__file__).resolve().parent.parent / "profiles" / "ragged_per_stream.json"
    runs = json.loads(path.read_text()) if path.exists() else {}
    runs[f"{coder}, jump_every={every}"] = result
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(runs, indent=1) + "\n")


if opts.tables == "per-stream":
    bench_per_stream(opts.streams, opts.loop_streams, jump_every)
    sys.exit(0)
rng = np.random.default_rng(1)
n_docs, n_sym, P = 100_000, 64, 24
probs = rng.dirichlet(np.ones(n_sym) * 0.5)
single = M.Categorical(probs, perfect=False)
from oracle import oracle as O      # (the table only: test infrastructure is not timed)
cdf = O.categorical_fast_cdf(probs, P)
model = B.Model.from_cdf(cdf, 0, P)


def bench_select(n_queries, every):
    """(a) N whole documents through the select call, (b) what a caller had before it: the full decode of the batch and a device gather
    of those documents, (c) N ranges of 64 symbols at random depths, (d) the same ranges on the batch encoded without jump points"""
    lengths = np.exp(rng.uniform(np.log(20), np.log(2000), n_docs)).astype(np.int64)
    offsets = np.zeros(n_docs + 1, dtype=np.int64); np.cumsum(lengths, out=offsets[1:])
    flat = torch.from_numpy(rng.choice(n_sym, size=int(offsets[-1]), p=probs).astype(np.int32)).cuda()
    off_d = torch.from_numpy(offsets).cuda()
    if coder == "range":
        with_table, without = B.range_encode_ragged_jump(flat, off_d, model, jump_every=every), B.range_encode_ragged(flat, off_d, model)
        decode, select = B.range_decode_ragged, B.range_decode_ragged_select
    else:
        with_table, without = B.ans_encode_ragged(flat, off_d, model, jump_every=every), B.ans_encode_ragged(flat, off_d, model, jump_every=0)
        decode, select = B.ans_decode_ragged, B.ans_decode_ragged_select
    picks = rng.choice(n_docs, size=n_queries, replace=False)
    streams = torch.from_numpy(picks).cuda()
    # the gather a caller writes: the flat positions of the picked documents' symbols
    sizes = off_d[streams + 1] - off_d[streams]
    starts = torch.zeros(n_queries + 1, dtype=torch.int64, device="cuda"); torch.cumsum(sizes, 0, out=starts[1:])
    index = torch.arange(int(starts[-1]), device="cuda") + torch.repeat_interleave(off_d[streams] - starts[:-1], sizes)
    want = flat[index]
    whole = torch.empty_like(flat)

    def full_then_gather():
        decode(with_table, model, off_d, out=whole)
        return whole[index]

    first_h = np.array([rng.integers(0, max(int(lengths[s]) - 64, 0) + 1) for s in picks], dtype=np.int64)
    count_h = np.minimum(64, lengths[picks] - first_h)
    first, count = torch.from_numpy(first_h).cuda(), torch.from_numpy(count_h).cuda()
    want_ranges = torch.cat([flat[offsets[s] + f: offsets[s] + f + c] for s, f, c in zip(picks, first_h, count_h)])
    got_a, _, st_a = select(with_table, model, off_d, streams)
    name = B.last_kernel()
    got_c, _, st_c = select(with_table, model, off_d, streams, first, count)
    got_d, _, st_d = select(without, model, off_d, streams, first, count)
    ok = (name.endswith("<select>") and bool(torch.equal(got_a, want)) and bool(torch.equal(full_then_gather(), want)) and bool(torch.equal(got_c, want_ranges))
          and bool(torch.equal(got_d, want_ranges)) and int(st_a.abs().sum() + st_c.abs().sum() + st_d.abs().sum()) == 0)
    a = best(lambda: select(with_table, model, off_d, streams, out=got_a))
    b = best(full_then_gather)
    c = best(lambda: select(with_table, model, off_d, streams, first, count, out=got_c))
    d = best(lambda: select(without, model, off_d, streams, first, count, out=got_d))
    print(f"{coder}: {n_docs} documents of 20 .. 2000 symbols ({int(offsets[-1]) / 1e6:.1f} M symbols), jump point every {every}; {n_queries} queries "
          f"({int(starts[-1])} symbols as whole documents, {int(count_h.sum())} as ranges of 64, mean depth {first_h.mean():.0f}):  "
          f"(a) select, whole documents {a:.3f} ms  (b) full decode + gather {b:.3f} ms  (c) select, ranges {c:.3f} ms  "
          f"(d) the ranges without jump points {d:.3f} ms  |  a / b {a / b:.2f}x  d / c {d / c:.1f}x  ok={ok}", flush=True)


if opts.select:
    bench_select(opts.select, jump_every or 256)
    sys.exit(0)
for label, lengths in (("20 .. 2000 symbols, shuffled", np.exp(rng.uniform(np.log(20), np.log(2000), n_docs)).astype(np.int64)),
                       ("the same, sorted by length", None), ("200 symbols each", np.full(n_docs, 200, dtype=np.int64))):
    if lengths is None:
        lengths = np.sort(prev)
    prev = lengths
    offsets = np.zeros(n_docs + 1, dtype=np.int64); np.cumsum(lengths, out=offsets[1:])
    flat = torch.from_numpy(rng.choice(n_sym, size=int(offsets[-1]), p=probs).astype(np.int32)).cuda()
    off_d = torch.from_numpy(offsets).cuda()
    if coder == "range":
        n = int(offsets[-1])
        enc = B.range_encode_ragged(flat, off_d, model)
        dec, st = B.range_decode_ragged(enc, model, off_d)
        ok = bool(torch.equal(dec, flat)) and int(enc.status.abs().sum()) == 0 and int(st.abs().sum()) == 0
        e = min(bench.event_ms(lambda: B.range_encode_ragged(flat, off_d, model), 5) for _ in range(3))
        d = min(bench.event_ms(lambda: B.range_decode_ragged(enc, model, off_d, out=dec), 5) for _ in range(3))
        # the comparison: the ANS coder without jump points (one chain per document, as the range coder's) on the same documents
        ans = B.ans_encode_ragged(flat, off_d, model, jump_every=0)
        adec, ast = B.ans_decode_ragged(ans, model, off_d)
        ok = ok and bool(torch.equal(adec, flat)) and int(ans.status.abs().sum()) == 0
        ae = min(bench.event_ms(lambda: B.ans_encode_ragged(flat, off_d, model, jump_every=0), 5) for _ in range(3))
        ad = min(bench.event_ms(lambda: B.ans_decode_ragged(ans, model, off_d, out=adec), 5) for _ in range(3))
        print(f"{n_docs} documents, {label} ({n / 1e6:.1f} M symbols): range encode {e:.3f} ms ({e * 1e3 / n_docs:.3f} us/doc, "
              f"{n / e / 1e6:.1f} Gsym/s)  decode {d:.3f} ms ({d * 1e3 / n_docs:.3f} us/doc, {n / d / 1e6:.1f} Gsym/s)  |  "
              f"ans, no jump points: encode {ae:.3f} ms  decode {ad:.3f} ms  |  range / ans: encode {e / ae:.2f}x  decode {d / ad:.2f}x  ok={ok}",
              flush=True)
        if jump_every:
            jenc = B.range_encode_ragged_jump(flat, off_d, model, jump_every=jump_every)
            jdec, jst = B.range_decode_ragged(jenc, model, off_d)
            jok = (B.last_kernel() == "range_decode_ragged_kernel<jump>" and bool(torch.equal(jdec, flat)) and bool(torch.equal(jenc.n_words, enc.n_words))
                   and int(jenc.status.abs().sum()) == 0 and int(jst.abs().sum()) == 0)
            runs = [(best(lambda: B.range_encode_ragged(flat, off_d, model)), best(lambda: B.range_decode_ragged(enc, model, off_d, out=dec)),
                     best(lambda: B.range_encode_ragged_jump(flat, off_d, model, jump_every=jump_every)),
                     best(lambda: B.range_decode_ragged(jenc, model, off_d, out=jdec))) for _ in range(2)]
            pair = lambda k: " / ".join(f"{r[k]:.3f}" for r in runs)
            print(f"    jump point every {jump_every} symbols ({int(jenc.jump.chunk_offsets[-1])} chunks), two runs: plain encode {pair(0)} ms  "
                  f"plain decode {pair(1)} ms  |  jump encode {pair(2)} ms  jump decode {pair(3)} ms  |  jump / plain: encode "
                  f"{min(r[2] for r in runs) / min(r[0] for r in runs):.2f}x  decode {min(r[3] for r in runs) / min(r[1] for r in runs):.2f}x  ok={jok}",
                  flush=True)
        continue
    enc = B.ans_encode_ragged(flat, off_d, model)
    dec, st = B.ans_decode_ragged(enc, model, off_d)
    ok = bool(torch.equal(dec, flat)) and int(enc.status.abs().sum()) == 0
    e = min(bench.event_ms(lambda: B.ans_encode_ragged(flat, off_d, model), 5) for _ in range(3))
    d = min(bench.event_ms(lambda: B.ans_decode_ragged(enc, model, off_d, out=dec), 5) for _ in range(3))
    n = int(offsets[-1])
    print(f"{n_docs} documents, {label} ({n / 1e6:.1f} M symbols): encode {e:.3f} ms ({e * 1e3 / n_docs:.3f} us/doc, {n / e / 1e6:.1f} Gsym/s)  "
          f"decode {d:.3f} ms ({d * 1e3 / n_docs:.3f} us/doc, {n / d / 1e6:.1f} Gsym/s)  ok={ok}")
docs = [flat[offsets[s]: offsets[s + 1]].cpu().numpy() for s in range(200)]
torch.cuda.synchronize()
if coder == "range":
    from constriction_amd.stream import queue
    t0 = time.perf_counter()
    words = []
    for doc in docs:
        c = queue.RangeEncoder(); c.encode(doc, single); words.append(c.get_compressed())
    t1 = time.perf_counter()
    for doc, w in zip(docs, words):
        assert np.array_equal(queue.RangeDecoder(w).decode(single, len(doc)), doc)
    t2 = time.perf_counter()
    print(f"drop-in, one RangeEncoder / RangeDecoder per document: encode {(t1 - t0) / 200 * 1e6:.0f} us/doc, decode {(t2 - t1) / 200 * 1e6:.0f} us/doc")
    sys.exit(0)
t0 = time.perf_counter()
words = []
for doc in docs:
    c = stack.AnsCoder(); c.encode_reverse(doc, single); words.append(c.get_compressed())
t1 = time.perf_counter()
for doc, w in zip(docs, words):
    assert np.array_equal(stack.AnsCoder(w).decode(single, len(doc)), doc)
t2 = time.perf_counter()
print(f"drop-in, one AnsCoder per document: encode {(t1 - t0) / 200 * 1e6:.0f} us/doc, decode {(t2 - t1) / 200 * 1e6:.0f} us/doc")
