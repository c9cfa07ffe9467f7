#!/usr/bin/env python3
"""The counting kernels of csrc/cst_fit.hip and Model.fit_per_stream against their yardsticks, in one run.

  shared      cst_count_symbols over the bench's C2 matrix (65 536 x 4096 int32 over -50..50, 1 GiB) on uniform, C2-Gaussian and
              constant data (and a Gaussian of std 0.6: three bins), under CST_FIT_REPLICAS = 1 | 8 and CST_FIT_WAVE_UNIFORM = 0 | 1,
              next to a plain read of the same matrix (torch.max: one pass over 1 GiB), to the counting kernel over a support the data
              never meets (its own loads, no atomic: the floor of this kernel) and to the torch route (torch.bincount over symbol - min);
  per_stream  cst_count_symbols_per_stream over the C3 matrix (support -127..127, one Gaussian per stream), next to the torch route
              (torch.bincount over symbol - min + row * n);
  indexed     cst_count_symbols with K = 64 uint8 indices over the C3 matrix, next to the torch route;
  fit         Model.fit_per_stream (count + quantise + model, P = 12) end to end at the C3 shape, host clock around a synchronise.
Times are medians of single launches between HIP events after a warm-up (bench.event_ms), the candidates of a group interleaved over
`--rounds` rounds.  Every count is compared with the torch route's at the size that is timed.
usage: bench_fit.py [--streams N] [--symbols N] [--rounds R] [--out profiles/fit.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import _native as N
from constriction_amd import batched as B


def interleaved(fns, rounds, reps=5):
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(bench.event_ms(fn, reps))
    return {name: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4)} for name, t in times.items()}


def knobs(replicas=None, wave_uniform=None):
    for name, value in (("CST_FIT_REPLICAS", replicas), ("CST_FIT_WAVE_UNIFORM", wave_uniform)):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(value)
    N.reload_knobs()


def torch_counts(sym, lo, n, rows=None, n_rows=1):
    """the torch route: one bincount over symbol - min (+ row * n)"""
    key = sym.reshape(-1).to(torch.int64) - lo
    if rows is not None:
        key += rows.reshape(-1).to(torch.int64) * n
    return torch.bincount(key, minlength=n_rows * n).reshape(n_rows, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=bench.N_STREAMS)
    ap.add_argument("--symbols", type=int, default=bench.N_PER)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n_streams, n_per = a.streams, a.symbols
    gib = n_streams * n_per * 4 / 2**30
    result = {"device": torch.cuda.get_device_name(0), "workload": {"streams": n_streams, "symbols_per_stream": n_per, "symbol_GiB": round(gib, 3)}}

    # ---- shared counts over the C2 matrix ----
    lo, hi = bench.LO, bench.HI
    n = hi - lo + 1
    m12 = B.Model.quantized_gaussian(lo, hi, bench.MEAN, bench.STD, 12)
    cdf_dev = torch.from_numpy(m12.cdf().astype(np.int64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(7)
    data = {"uniform": torch.randint(lo, hi + 1, (n_streams, n_per), generator=g, device="cuda", dtype=torch.int32),
            "c2_gaussian": bench.synth_symbols_device(bench.SEED, 0, n_streams, n_per, lo, cdf_dev, 12),
            "peaked_gaussian": torch.clamp(torch.round(torch.randn((n_streams, n_per), generator=g, device="cuda") * 0.6 + bench.MEAN), lo, hi).to(torch.int32),
            "constant": torch.full((n_streams, n_per), 3, dtype=torch.int32, device="cuda")}
    result["shared"] = {"support": [lo, hi], "rows": []}
    for kind, sym in data.items():
        want = torch_counts(sym, lo, n)
        # (a support the data never meets: the counting kernel's own loads and compares, without a single LDS atomic)
        fns = {"plain_read_torch_max": lambda sym=sym: sym.max(), "read_only_same_kernel": lambda sym=sym: B.count_symbols(sym, hi + 1000, hi + 1000 + n - 1),
               "torch_bincount": lambda sym=sym: torch_counts(sym, lo, n)}
        for reps in (1, 8):
            for uniform in (0, 1):
                def call(sym=sym, reps=reps, uniform=uniform):
                    knobs(reps, uniform)
                    return B.count_symbols(sym, lo, hi)
                counts, outside = call()
                assert torch.equal(counts.to(torch.int64), want) and int(outside.item()) == 0, (kind, reps, uniform)
                fns[f"count_symbols_replicas{reps}_wave_uniform{uniform}"] = call
        row = {"data": kind, **interleaved(fns, a.rounds)}
        floor = row["plain_read_torch_max"]["median_ms"]
        for name in list(row):
            if name.startswith("count_symbols") or name in ("torch_bincount", "read_only_same_kernel"):
                row[name]["ratio_to_plain_read"] = round(row[name]["median_ms"] / floor, 3)
        row["plain_read_GBps"] = round(n_streams * n_per * 4 / floor / 1e6, 1)
        result["shared"]["rows"].append(row)
        print(json.dumps(row), flush=True)
        del want
    knobs()
    del data, sym

    # ---- per-stream and indexed counts over the C3 matrix ----
    lo, hi = -127, 127
    n = hi - lo + 1
    mu, sigma = bench.c3_parameters(bench.SEED, 0, n_streams, n_per, "cuda")
    m3 = B.Model.quantized_gaussian_per_stream(lo, hi, mu, sigma, 12)
    sym3 = bench.synth_symbols_per_stream(bench.SEED, 0, n_per, lo, m3.cdfs_device(), 12)
    del m3
    stream_of = torch.arange(n_streams, device="cuda", dtype=torch.int32)[:, None].expand(n_streams, n_per)
    want = torch_counts(sym3, lo, n, stream_of, n_streams)
    counts, outside = B.count_symbols(sym3, lo, hi, per_stream=True)
    assert torch.equal(counts.to(torch.int64), want) and int(outside.item()) == 0
    del want, counts
    row = interleaved({"plain_read_torch_max": lambda: sym3.max(),
                       "count_symbols_per_stream": lambda: B.count_symbols(sym3, lo, hi, per_stream=True),
                       "torch_bincount": lambda: torch_counts(sym3, lo, n, stream_of, n_streams)}, a.rounds)
    for name in ("count_symbols_per_stream", "torch_bincount"):
        row[name]["ratio_to_plain_read"] = round(row[name]["median_ms"] / row["plain_read_torch_max"]["median_ms"], 3)
    result["per_stream"] = {"support": [lo, hi], **row}
    print(json.dumps(result["per_stream"]), flush=True)

    K = 64
    idx = torch.randint(0, K, (n_streams, n_per), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    want = torch_counts(sym3, lo, n, idx, K)
    counts, outside = B.count_symbols(sym3, lo, hi, indices=idx, n_tables=K)
    assert torch.equal(counts.to(torch.int64), want) and int(outside.item()) == 0
    del want, counts
    row = interleaved({"plain_read_torch_max": lambda: (sym3.max(), idx.max()),
                       "count_symbols_indexed_u8": lambda: B.count_symbols(sym3, lo, hi, indices=idx, n_tables=K),
                       "torch_bincount": lambda: torch_counts(sym3, lo, n, idx, K)}, a.rounds)
    for name in ("count_symbols_indexed_u8", "torch_bincount"):
        row[name]["ratio_to_plain_read"] = round(row[name]["median_ms"] / row["plain_read_torch_max"]["median_ms"], 3)
    result["indexed"] = {"support": [lo, hi], "tables": K, "replicas": 1, **row}      # (64 x 255 bins leave LDS room for one copy)
    print(json.dumps(result["indexed"]), flush=True)
    del idx

    # ---- Model.fit_per_stream end to end ----
    def fit():
        return B.Model.fit_per_stream(sym3, lo, hi, 12)
    model = fit()
    assert model.n_tables == n_streams
    del model
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        model = fit()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del model
    parts = interleaved({"count": lambda: B.count_symbols(sym3, lo, hi, per_stream=True)}, 1)
    counts, _ = B.count_symbols(sym3, lo, hi, per_stream=True)
    parts.update(interleaved({"fit_cdf_rows": lambda: B.fit_cdf_rows(counts, 12)}, 1))
    result["fit_per_stream"] = {"precision": 12, "host_clock_median_ms": round(float(np.median(times)), 3), "host_clock_min_ms": round(min(times), 3),
                                "parts": parts}
    print(json.dumps(result["fit_per_stream"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
