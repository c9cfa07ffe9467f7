#!/usr/bin/env python3
"""The range coder with one table per stream (csrc/cst_range_ps.hip) next to its neighbours, in one run.

  batch    range_encode / range_decode over the C3 matrix (65 536 x 4096 int32, support -127..127, one Gaussian row per stream,
           P = 12), plain and with jump_points=2; the per-stream ANS default call on the same model and symbols (C3); the
           shared-table range call on the same symbols (C4: another model, the same bytes through the coder);
  loop256  at 256 streams: the batched per-stream call against a loop of 256 single-stream range_encode calls with shared models
           built from the same rows -- the only route to these words before the per-stream kernels.  The loop's words are compared
           with the batched call's.
Times are medians of single launches between HIP events after a warm-up (bench.event_ms), the candidates of a group interleaved over
`--rounds` rounds.  Every decode is compared with the symbols at the size that is timed.
usage: bench_range_per_stream.py [--streams N] [--symbols N] [--rounds R] [--out profiles/range_per_stream.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import batched as B


def interleaved(fns, rounds, reps=5):
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(bench.event_ms(fn, reps))
    return {name: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=bench.N_STREAMS)
    ap.add_argument("--symbols", type=int, default=bench.N_PER)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n_streams, n_per = a.streams, a.symbols
    lo, hi, P = -127, 127, 12
    cfg = (32, 64, P)
    result = {"device": torch.cuda.get_device_name(0), "preset": list(cfg), "support": [lo, hi],
              "workload": {"streams": n_streams, "symbols_per_stream": n_per, "symbol_GiB": round(n_streams * n_per * 4 / 2**30, 3)}}

    mu, sigma = bench.c3_parameters(bench.SEED, 0, n_streams, n_per, "cuda")
    model = B.Model.quantized_gaussian_per_stream(lo, hi, mu, sigma, P)
    rows = model.cdfs_device()
    sym = bench.synth_symbols_per_stream(bench.SEED, 0, n_per, lo, rows, P)
    shared = B.Model.quantized_gaussian(lo, hi, 0.0, 40.0, P)
    decoded = torch.empty_like(sym)

    def check(dec_status, what):
        dec, status = dec_status
        assert int(status.abs().sum()) == 0 and torch.equal(dec, sym), what

    # ---- the whole batch ----
    enc = B.range_encode(sym, model, cfg, jump_points=0)
    assert B.last_kernel() == "range_encode_ps_kernel" and int(enc.status.abs().sum()) == 0
    enc2 = B.range_encode(sym, model, cfg, jump_points=2)
    assert B.last_kernel() == "range_encode_ps_kernel<ckpt>" and torch.equal(enc2.n_words, enc.n_words)
    check(B.range_decode(enc, model, n_per, out=decoded), "plain")
    assert B.last_kernel() == "range_decode_ps_kernel"
    check(B.range_decode(enc2, model, n_per, out=decoded), "jump_points=2")
    assert B.last_kernel() == "range_decode_ps_kernel<chunks>"
    ans = B.ans_encode(sym, model, cfg)
    check(B.ans_decode(ans, model, n_per, out=decoded), "ans per stream")
    c4 = B.range_encode(sym, shared, cfg)
    check(B.range_decode(c4, shared, n_per, out=decoded), "range shared")
    fns = {"range_ps_encode": lambda: B.range_encode(sym, model, cfg, out=enc, jump_points=0),
           "range_ps_decode": lambda: B.range_decode(enc, model, n_per, out=decoded),
           "range_ps_encode_jump2": lambda: B.range_encode(sym, model, cfg, out=enc2, jump_points=2),
           "range_ps_decode_jump2": lambda: B.range_decode(enc2, model, n_per, out=decoded),
           "ans_ps_encode_default_C3": lambda: B.ans_encode(sym, model, cfg, out=ans),
           "ans_ps_decode_default_C3": lambda: B.ans_decode(ans, model, n_per, out=decoded),
           "range_shared_encode_default_C4": lambda: B.range_encode(sym, shared, cfg, out=c4),
           "range_shared_decode_default_C4": lambda: B.range_decode(c4, shared, n_per, out=decoded)}
    row = interleaved(fns, a.rounds)
    gsym = n_streams * n_per / 1e6
    for name in row:
        row[name]["Gsym_per_s"] = round(gsym / row[name]["median_ms"], 2)
    row["words_per_stream_mean"] = {"range_per_stream": round(float(enc.n_words.float().mean()), 2), "ans_per_stream": round(float(ans.n_words.float().mean()), 2),
                                    "range_shared": round(float(c4.n_words.float().mean()), 2)}
    row["jump2_decode_over_plain_decode"] = round(row["range_ps_decode_jump2"]["median_ms"] / row["range_ps_decode"]["median_ms"], 3)
    result["batch"] = row
    print(json.dumps(row), flush=True)
    del enc2, ans, c4, decoded

    # ---- 256 streams: one batched call against 256 single-stream calls ----
    k = min(256, n_streams)
    sym_k = sym[:k].contiguous()
    model_k = B.Model.from_cdf_rows_per_stream(rows[:k].contiguous(), lo, P)
    rows_host = rows[:k].cpu().numpy().view(np.uint32)
    singles = [B.Model.from_cdf(rows_host[s], lo, P) for s in range(k)]
    one = [sym_k[s:s + 1] for s in range(k)]
    enc_k = B.range_encode(sym_k, model_k, cfg, jump_points=0)
    outs = [B.range_encode(one[s], singles[s], cfg, jump_points=0) for s in range(k)]
    torch.cuda.synchronize()
    for s in range(k):
        n = int(enc_k.n_words[s])
        assert int(outs[s].n_words[0]) == n and torch.equal(outs[s].words[0, :n], enc_k.words[s, :n]), s

    def loop():
        for s in range(k):
            B.range_encode(one[s], singles[s], cfg, out=outs[s], jump_points=0)

    row = interleaved({"batched_per_stream_call": lambda: B.range_encode(sym_k, model_k, cfg, out=enc_k, jump_points=0),
                       "loop_of_single_stream_calls": loop}, a.rounds)
    row["streams"] = k
    row["loop_over_batched"] = round(row["loop_of_single_stream_calls"]["median_ms"] / row["batched_per_stream_call"]["median_ms"], 2)
    assert row["batched_per_stream_call"]["median_ms"] < row["loop_of_single_stream_calls"]["median_ms"], row
    result["loop256"] = row
    print(json.dumps(row), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
