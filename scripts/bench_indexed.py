#!/usr/bin/env python3
"""Indexed table coding against its neighbours, in one run with alternating calls.

Workload: 65 536 streams x 4096 symbols over -127..127, K = 64 Gaussian tables with log-spaced scales 0.11 .. 64, indices uniform,
every symbol drawn from the table its index names; P = 12 and P = 16, both coders, uint8 and int32 indices.  Neighbours:
  (a) batched.{ans,range}_{encode,decode}_gaussian on the same per-symbol (mean, std): what a caller uses today;
  (b) the per-stream-table (C3) ans_encode / ans_decode at P = 12 on the same shape: the same lookups with the row fixed per stream;
  (c) cst_{ans,range}_encode_cp_batch / _decode_rows_batch over explicit per-symbol rows at --explicit-streams streams (a cdf row per
      symbol is 1 KiB: the full batch would need 275 GB), with the gathers that feed them counted.
Times are medians of single launches between HIP events after a warm-up (bench.event_ms), the rounds of the candidates interleaved;
usage: bench_indexed.py [--streams N] [--symbols N] [--explicit-streams N] [--rounds R] [--out profiles/indexed.json]"""
import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import _native as N
from constriction_amd import batched as B

LO, HI, K = -127, 127, 64


def draw(idx, cdfs, P, seed):
    """symbols of idx's shape, each from the table its index names (the quantile function of a uniform P-bit draw)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sym = torch.empty(idx.shape, dtype=torch.int32, device="cuda")
    inner = torch.from_numpy(cdfs[:, 1:-1].astype(np.int64)).cuda()
    for a in range(0, idx.shape[0], 4096):
        part = idx[a:a + 4096].to(torch.int64)
        q = torch.randint(0, 1 << P, part.shape, generator=g, device="cuda")
        out = sym[a:a + 4096]
        for k in range(cdfs.shape[0]):
            m = part == k
            out[m] = (torch.searchsorted(inner[k], q[m], right=True) + LO).to(torch.int32)
    return sym


def interleaved(fns, rounds, reps=5):
    """{name: median ms}: `rounds` rounds over all candidates, each timed by bench.event_ms"""
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(bench.event_ms(fn, reps))
    return {name: float(np.median(t)) for name, t in times.items()}, {name: float(np.min(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--symbols", type=int, default=4096)
    ap.add_argument("--explicit-streams", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, per = a.streams, a.symbols
    stds = np.geomspace(0.11, 64.0, K)
    means = np.zeros(K)
    g = torch.Generator(device="cuda").manual_seed(1)
    idx32 = torch.randint(0, K, (n, per), generator=g, device="cuda", dtype=torch.int32)
    idx8 = idx32.to(torch.uint8)
    d_means = torch.from_numpy(means).cuda()[idx32.long()]
    d_stds = torch.from_numpy(stds).cuda()[idx32.long()]
    result = {"workload": {"streams": n, "symbols_per_stream": per, "support": [LO, HI], "tables": K, "stds": [0.11, 64.0]}, "rows": []}
    roofline_ms = lambda P: (n * per * 4 + n * per * P / 8 * 0.5) / 8e12 * 1e3        # (the symbol matrix alone bounds it; for orientation)

    for P in (12, 16):
        cfg = (32, 64, P)
        tables = B.TableSet.quantized_gaussians(LO, HI, means, stds, P)
        cdfs = tables.cdfs()
        sym = draw(idx32, cdfs, P, 100 + P)
        row = {"precision": P}
        for coder in ("ans", "range"):
            enc_ix, dec_ix = getattr(B, f"{coder}_encode_indexed"), getattr(B, f"{coder}_decode_indexed")
            enc_g, dec_g = getattr(B, f"{coder}_encode_gaussian"), getattr(B, f"{coder}_decode_gaussian")
            e8 = enc_ix(sym, idx8, tables, cfg)
            e32 = enc_ix(sym, idx32, tables, cfg)
            eg = enc_g(sym, LO, HI, d_means, d_stds, cfg)
            out = torch.empty_like(sym)
            assert torch.equal(dec_ix(e8, idx8, tables, per, out=out)[0], sym) and torch.equal(e8.n_words, e32.n_words)
            assert torch.equal(dec_g(eg, LO, HI, d_means, d_stds, out=out)[0], sym)
            assert torch.equal(eg.n_words, e8.n_words)      # (the same models, so the same words)
            fns = {
                f"{coder}_encode_indexed_u8": lambda: enc_ix(sym, idx8, tables, cfg, out=e8),
                f"{coder}_encode_indexed_i32": lambda: enc_ix(sym, idx32, tables, cfg, out=e32),
                f"{coder}_encode_gaussian": lambda: enc_g(sym, LO, HI, d_means, d_stds, cfg, out=eg),
                f"{coder}_decode_indexed_u8": lambda: dec_ix(e8, idx8, tables, per, out=out),
                f"{coder}_decode_indexed_i32": lambda: dec_ix(e32, idx32, tables, per, out=out),
                f"{coder}_decode_gaussian": lambda: dec_g(eg, LO, HI, d_means, d_stds, out=out),
            }
            if coder == "ans" and P == 12:      # (b) one table per stream: stream s has level s % K, its symbols drawn from that table
                idx_b = (torch.arange(n, device="cuda", dtype=torch.int32) % K)[:, None].expand(n, per).contiguous()
                sym_b = draw(idx_b, cdfs, P, 7)
                model_b = B.Model.quantized_gaussian_per_stream(LO, HI, torch.from_numpy(means).cuda()[idx_b[:, 0].long()],
                                                                torch.from_numpy(stds).cuda()[idx_b[:, 0].long()], P)
                eb = B.ans_encode(sym_b, model_b, cfg, jump_points=0)
                row["b_kernels"] = [B.last_kernel()]
                assert torch.equal(B.ans_decode(eb, model_b, per, out=out)[0], sym_b)
                row["b_kernels"].append(B.last_kernel())
                fns["ans_encode_per_stream_table"] = lambda: B.ans_encode(sym_b, model_b, cfg, out=eb, jump_points=0)
                fns["ans_decode_per_stream_table"] = lambda: B.ans_decode(eb, model_b, per, out=out)
            med, best = interleaved(fns, a.rounds)
            for name in fns:
                row[name] = {"median_ms": round(med[name], 4), "min_ms": round(best[name], 4)}
            if P == 16:         # the decoder's lookup: the bucket index capped at b bits (0: a binary search of the whole row)
                for bits in (0, 4, 8):
                    os.environ["CST_INDEXED_BUCKET_BITS"] = str(bits)
                    N.reload_knobs()
                    capped = B.TableSet.quantized_gaussians(LO, HI, means, stds, P)
                    assert torch.equal(dec_ix(e8, idx8, capped, per, out=out)[0], sym)
                    result.setdefault("lookup", []).append({"precision": P, "call": f"{coder}_decode_indexed_u8", "bucket_bits": bits,
                                                            "median_ms": round(bench.event_ms(lambda: dec_ix(e8, idx8, capped, per, out=out), 9), 4)})
                os.environ.pop("CST_INDEXED_BUCKET_BITS")
                N.reload_knobs()
            del fns, e8, e32, eg, out
        result["rows"].append(row)
        del sym, tables

        # (c) explicit per-symbol models at a size whose rows fit: the gathers are part of the route
        ns = a.explicit_streams
        tables = B.TableSet.quantized_gaussians(LO, HI, means, stds, P)
        d_cdfs = torch.from_numpy(tables.cdfs().astype(np.int32)).cuda()
        i32, i8 = idx32[:ns].contiguous(), idx8[:ns].contiguous()
        sym = draw(i32, tables.cdfs(), P, 200 + P)
        lib = N.lib()
        crow = {"precision": P, "streams": ns}
        for coder in ("ans", "range"):
            stride = (B.max_words if coder == "ans" else B.range_max_words)(per, cfg)
            enc = B._new_batch(ns, stride, sym.device, cfg)
            out = torch.empty_like(sym)
            status = torch.empty(ns, dtype=torch.int32, device="cuda")

            def encode_cp():
                at = (sym - LO).long()
                left = d_cdfs[i32.long(), at]
                prob = d_cdfs[i32.long(), at + 1] - left
                N.check(getattr(lib, f"cst_{coder}_encode_cp_batch")(B._cfg(*cfg), B._ptr(left), B._ptr(prob), ns, per, 0, B._ptr(enc.words), stride,
                                                                     B._ptr(enc.n_words), None, B._ptr(enc.status), 0, B._stream_ptr()))

            def decode_rows():
                rows = d_cdfs[i32.long().reshape(-1)]
                args = [B._cfg(*cfg), B._ptr(enc.words), None, stride, enc.words.numel(), B._ptr(enc.n_words), B._ptr(rows), HI - LO + 1, LO,
                        B._ptr(out), ns, per, 0, None]
                if coder == "ans":
                    args.append(None)
                N.check(getattr(lib, f"cst_{coder}_decode_rows_batch")(*args, B._ptr(status), 0, B._stream_ptr()))

            e8 = getattr(B, f"{coder}_encode_indexed")(sym, i8, tables, cfg)
            encode_cp()
            decode_rows()
            assert torch.equal(out, sym) and torch.equal(enc.words[:, :8], e8.words[:, :8]) and torch.equal(enc.n_words, e8.n_words)
            fns = {f"{coder}_encode_explicit": encode_cp, f"{coder}_decode_explicit": decode_rows,
                   f"{coder}_encode_indexed_u8": lambda: getattr(B, f"{coder}_encode_indexed")(sym, i8, tables, cfg, out=e8),
                   f"{coder}_decode_indexed_u8": lambda: getattr(B, f"{coder}_decode_indexed")(e8, i8, tables, per, out=out)}
            med, best = interleaved(fns, max(2, a.rounds // 2), reps=3)
            for name in fns:
                crow[name] = {"median_ms": round(med[name], 4), "min_ms": round(best[name], 4)}
            del fns, enc, out, e8
            torch.cuda.empty_cache()
        result.setdefault("explicit", []).append(crow)

    # the three ratios per coder and direction: indexed (uint8) time over the neighbour's time (below 1 = indexed is faster)
    ratios = []
    for row in result["rows"]:
        for coder in ("ans", "range"):
            for d in ("encode", "decode"):
                r = {"precision": row["precision"], "call": f"{coder}_{d}",
                     "indexed_u8_ms": row[f"{coder}_{d}_indexed_u8"]["median_ms"], "indexed_i32_ms": row[f"{coder}_{d}_indexed_i32"]["median_ms"],
                     "a_gaussian_ms": row[f"{coder}_{d}_gaussian"]["median_ms"]}
                r["over_a"] = round(r["indexed_u8_ms"] / r["a_gaussian_ms"], 3)
                if f"{coder}_{d}_per_stream_table" in row:
                    r["b_per_stream_table_ms"] = row[f"{coder}_{d}_per_stream_table"]["median_ms"]
                    r["over_b"] = round(r["indexed_u8_ms"] / r["b_per_stream_table_ms"], 3)
                c = next(x for x in result["explicit"] if x["precision"] == row["precision"])
                r["c_explicit_ms_at_%d_streams" % c["streams"]] = c[f"{coder}_{d}_explicit"]["median_ms"]
                r["over_c"] = round(c[f"{coder}_{d}_indexed_u8"]["median_ms"] / c[f"{coder}_{d}_explicit"]["median_ms"], 3)
                r["symbol_matrix_floor_ms"] = round(roofline_ms(row["precision"]), 4)
                ratios.append(r)
    result["ratios"] = ratios
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
