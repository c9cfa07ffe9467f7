#!/usr/bin/env python3
"""Per-symbol quantized models (the reference's flagship call, src/pybindings/stream/stack.rs:567-588, 733-751) batched:
n_streams x n_per symbols, every symbol with its own two f64 parameters; both coders; round trip checked.

    bench_per_symbol.py [n_streams [n_per]] [--family gaussian laplace cauchy] [--support LO HI] [--rows] [--reps N] [--rounds K]
                        [--params f64|f32|both]
    bench_per_symbol.py [n_streams [n_per]] --categorical K [--f64] [--reps N] [--rounds K]
    bench_per_symbol.py [n_streams [n_per]] --categorical K --perfect [--f64] [--reps N] [--rounds K]

--family: one or more of gaussian (mean, std), laplace (mean, scale), cauchy (loc, scale); several families are timed in the
          same process on the same parameter matrices, alternating, `--rounds` times over: compare medians, look at the spread.
          Next to another family the Gaussian is also timed without jump points, which the other families do not have.
--params: the element type of the parameter matrices.  f64 (default): float64 tensors.  f32: float32 tensors, read by the kernels
          themselves (the _f32 entry points).  both: the SAME values (rounded to float32 first) through (a) the float64 call on tensors
          widened beforehand, (b) the float32 call, and (c) what a float32 caller paid before the _f32 entry points: `.double()` of both
          matrices inside the timed region plus the float64 call -- alternating like the families; the words of (a) and (b) and the
          symbols they decode to are compared at the timed size.
--rows:   also times what a caller of Laplace / Cauchy had before the family calls: one tabulated cdf row per symbol
          (family_cdf_rows) + cst_ans_encode_cp_batch / cst_ans_decode_rows_batch.  n_symbols + 1 words of row per symbol: keep
          the batch small (4096 x 256 at a 201-symbol support is 850 MB of rows).
--categorical K: per-symbol Categorical models instead, from a [n_streams, n_per, K] matrix of float32 (--f64: float64) probabilities
          (default 4096 x 256; at K = 256 that is 1 GiB of float32): encode and decode of both coders through the categorical calls
          (the decoder by both of its routes), the probability bytes per second of each against the 8 TB/s of HBM, and the same
          batch through the tabulated device route -- categorical_cdf_rows + cst_*_encode_cp_batch / cst_*_decode_rows_batch --
          in the same run.
--perfect: with --categorical K (K <= 1024), Categorical(perfect=True) instead: the rows kernel alone (rows per second, the maximum
          and the mean of its move counts), the four coder calls of `*_categorical(..., perfect=True)`, and -- in the same run --
          the host route they replace, Categorical(perfect=True).family_rows on a slice of at most 4096 rows, scaled to the
          batch and labelled as scaled."""
import argparse
import statistics
import sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from constriction_amd import batched as B
from constriction_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("n_streams", nargs="?", type=int, default=None)
ap.add_argument("n_per", nargs="?", type=int, default=None)
ap.add_argument("--categorical", type=int, default=0, metavar="K")
ap.add_argument("--f64", action="store_true")
ap.add_argument("--perfect", action="store_true")
ap.add_argument("--family", nargs="+", choices=["gaussian", "laplace", "cauchy"], default=["gaussian"])
ap.add_argument("--support", nargs=2, type=int, default=[-127, 127], metavar=("LO", "HI"))
ap.add_argument("--rows", action="store_true")
ap.add_argument("--params", choices=["f64", "f32", "both"], default="f64")
ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
ap.add_argument("--rounds", type=int, default=1, help="timed windows per entry (the median and the range are printed)")
args = ap.parse_args()
n_streams = args.n_streams or (4096 if args.categorical else 65536)
n_per = args.n_per or (256 if args.categorical else 4096)
lo, hi = args.support


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def categorical_bench(K):
    import os
    dtype = torch.float64 if args.f64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(1)
    probs = torch.softmax(torch.randn((n_streams, n_per, K), generator=g, device="cuda", dtype=torch.float32) * 3.0, dim=-1).to(dtype)
    sym = torch.randint(0, K, (n_streams, n_per), generator=g, device="cuda", dtype=torch.int32)
    prob_bytes = probs.numel() * probs.element_size()
    cfg = (32, 64, 24)
    L, p, sp = N.lib(), B._ptr, B._stream_ptr

    def route(name):
        os.environ["CST_CATEGORICAL_ROUTE"] = name
        N.reload_knobs()

    def tabulated(coder):
        """the tabulated device route, rows built inside the timed call (they are part of what the caller pays)"""
        flat = sym.reshape(-1).to(torch.int64)
        ar = torch.arange(n_streams * n_per, device="cuda")
        stride = (B.max_words if coder == "ans" else B.range_max_words)(n_per, cfg)
        out = B._new_batch(n_streams, stride, sym.device, cfg)
        dec = torch.empty_like(sym)
        status = torch.empty(n_streams, dtype=torch.int32, device="cuda")

        def encode():
            rows = B.categorical_cdf_rows(probs).reshape(-1, K + 1)
            left = rows[ar, flat].contiguous()
            prob = (rows[ar, flat + 1] - left).contiguous()
            N.check(getattr(L, f"cst_{coder}_encode_cp_batch")(B._cfg(*cfg), p(left), p(prob), n_streams, n_per, N.LAYOUT_STREAM_MAJOR, p(out.words), stride,
                                                               p(out.n_words), None, p(out.status), N.FLAG_NONE, sp()), "encode_cp")
            return out

        def decode(enc):
            rows = B.categorical_cdf_rows(probs)
            a = [B._cfg(*cfg), p(enc.words), None, stride, enc.words.numel(), p(enc.n_words), p(rows), K, 0, p(dec), n_streams, n_per,
                 N.LAYOUT_STREAM_MAJOR, None]
            if coder == "ans":
                a.append(None)
            N.check(getattr(L, f"cst_{coder}_decode_rows_batch")(*a, p(status), N.FLAG_NONE, sp()), "decode_rows")
            return dec, status
        return encode, decode

    entries = []
    for coder in ("ans", "range"):
        enc_f, dec_f = getattr(B, f"{coder}_encode_categorical"), getattr(B, f"{coder}_decode_categorical")
        entries.append((coder, "in-kernel, lane decoder", "fused", (lambda enc_f=enc_f: enc_f(sym, probs, cfg)), (lambda enc, dec_f=dec_f: dec_f(enc, probs))))
        entries.append((coder, "in-kernel, rows in pieces", "rows", (lambda enc_f=enc_f: enc_f(sym, probs, cfg)), (lambda enc, dec_f=dec_f: dec_f(enc, probs))))
        entries.append((coder, "tabulated device route", "", *tabulated(coder)))
    times = {i: ([], []) for i in range(len(entries))}
    ok = {}
    for i, (coder, how, r, enc_f, dec_f) in enumerate(entries):
        route(r)
        enc = enc_f()
        dec, st = dec_f(enc)
        torch.cuda.synchronize()
        ok[i] = bool(torch.equal(dec, sym)) and int(st.abs().sum()) == 0
    for _ in range(args.rounds):
        for i, (coder, how, r, enc_f, dec_f) in enumerate(entries):
            route(r)
            e, enc = timed(enc_f, args.reps)
            d, _ = timed(lambda: dec_f(enc), args.reps)
            times[i][0].append(e); times[i][1].append(d)
    route("")
    print(f"per-symbol Categorical, {n_streams} x {n_per} symbols, K = {K}, {str(dtype).split('.')[-1]}: {prob_bytes / 2**30:.2f} GiB of probabilities")
    for i, (coder, how, r, _, _) in enumerate(entries):
        e, d = statistics.median(times[i][0]), statistics.median(times[i][1])
        print(f"{coder:5s} {how:26s}: encode {e:9.3f} ms ({prob_bytes / e / 1e9:6.3f} TB/s of probabilities, {100 * prob_bytes / e / 1e9 / 8:5.1f} % of 8 TB/s)  "
              f"decode {d:9.3f} ms ({prob_bytes / d / 1e9:6.3f} TB/s, {100 * prob_bytes / d / 1e9 / 8:5.1f} %)  roundtrip_ok={ok[i]}")


def categorical_perfect_bench(K):
    import time
    import numpy as np
    from constriction_amd.stream import model as M
    dtype = torch.float64 if args.f64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(1)
    probs = torch.softmax(torch.randn((n_streams, n_per, K), generator=g, device="cuda", dtype=torch.float32) * 3.0, dim=-1).to(dtype)
    sym = torch.randint(0, K, (n_streams, n_per), generator=g, device="cuda", dtype=torch.int32)
    cfg, n_rows = (32, 64, 24), n_streams * n_per
    rows_ms, moves = [], None
    _, moves = B.categorical_cdf_rows(probs, cfg[2], perfect=True, return_moves=True)          # (warm-up; raises for a stopped row)
    for _ in range(args.rounds):
        t, _ = timed(lambda: B.categorical_cdf_rows(probs, cfg[2], perfect=True), args.reps)
        rows_ms.append(t)
    ok, times = {}, {}
    for coder in ("ans", "range"):
        enc_f, dec_f = getattr(B, f"{coder}_encode_categorical"), getattr(B, f"{coder}_decode_categorical")
        enc = enc_f(sym, probs, cfg, perfect=True)
        dec, st = dec_f(enc, probs, perfect=True)
        torch.cuda.synchronize()
        ok[coder] = bool(torch.equal(dec, sym)) and int(st.abs().sum()) == 0
        times[coder] = ([], [])
        for _ in range(args.rounds):
            e, enc = timed(lambda: enc_f(sym, probs, cfg, perfect=True), args.reps)
            d, _ = timed(lambda: dec_f(enc, probs, perfect=True), args.reps)
            times[coder][0].append(e); times[coder][1].append(d)
    # the host route: one sequential search per row in the library's host code, behind a Python loop
    n_host = min(n_rows, 4096)
    host_probs = probs.reshape(-1, K)[:n_host].cpu().numpy()
    t0 = time.perf_counter()
    host_rows = M.Categorical(perfect=True).family_rows((host_probs,))
    host_s = time.perf_counter() - t0
    same = np.array_equal(host_rows, B.categorical_cdf_rows(probs.reshape(-1, K)[:n_host], cfg[2], perfect=True).cpu().numpy().view(np.uint32))
    r = statistics.median(rows_ms)
    print(f"per-symbol Categorical(perfect=True), {n_streams} x {n_per} symbols, K = {K}, {str(dtype).split('.')[-1]}")
    print(f"rows kernel              : {r:9.3f} ms for {n_rows} rows ({n_rows / r / 1e3:8.3f} M rows/s)  moves: max {int(moves.max())}, "
          f"mean {float(moves.double().mean()):.2f} (cap {16 * K + 1024})")
    for coder in ("ans", "range"):
        e, d = statistics.median(times[coder][0]), statistics.median(times[coder][1])
        print(f"{coder:5s} device quantiser   : encode {e:9.3f} ms  decode {d:9.3f} ms  roundtrip_ok={ok[coder]}")
    print(f"host route (family_rows) : {host_s * 1e3:9.3f} ms for {n_host} rows = {host_s * 1e3 * n_rows / n_host:11.3f} ms SCALED to {n_rows} rows "
          f"({n_host / host_s / 1e6:8.5f} M rows/s; rows only, before any upload or coding)  same_rows={same}")


if args.perfect and not args.categorical:
    ap.error("--perfect needs --categorical K")
if args.categorical and args.perfect:
    categorical_perfect_bench(args.categorical)
    sys.exit(0)
if args.categorical:
    categorical_bench(args.categorical)
    sys.exit(0)

g = torch.Generator(device="cuda").manual_seed(1)
means = (torch.rand((n_streams, n_per), generator=g, device="cuda", dtype=torch.float64) * 20 - 10)
stds = torch.exp(torch.rand((n_streams, n_per), generator=g, device="cuda", dtype=torch.float64) * 3.4 - 0.7)
means32 = stds32 = None
if args.params != "f64":                     # float32-representable values: every form below codes the same models
    means32, stds32 = means.float(), stds.float()
    means, stds = means32.double(), stds32.double()
sym = torch.clamp(torch.round(torch.randn((n_streams, n_per), generator=g, device="cuda", dtype=torch.float64) * stds + means), lo, hi).to(torch.int32)
# (label, parameter matrices as the call gets them): "widen" = float32 matrices that the timed call itself widens first
PARAM_FORMS = {"f64": [("", "f64")], "f32": [(" f32", "f32")],
               "both": [(" (a) f64, widened beforehand", "f64"), (" (b) f32", "f32"), (" (c) f32 + .double() inside", "widen")]}[args.params]


def params_of(form):
    if form == "f64":
        return lambda: (means, stds)
    if form == "f32":
        return lambda: (means32, stds32)
    return lambda: (means32.double(), stds32.double())


def family_calls(family, coder, jump_points="auto", form="f64"):
    par = params_of(form)
    if family == "gaussian":
        enc_f, dec_f = getattr(B, f"{coder}_encode_gaussian"), getattr(B, f"{coder}_decode_gaussian")
        return (lambda: enc_f(sym, lo, hi, *par(), jump_points=jump_points)), (lambda enc: dec_f(enc, lo, hi, *par()))
    enc_f, dec_f = getattr(B, f"{coder}_encode_family"), getattr(B, f"{coder}_decode_family")
    return (lambda: enc_f(family, sym, lo, hi, *par())), (lambda enc: dec_f(family, enc, lo, hi, *par()))


def rows_calls(family, coder):
    """the tabulated route, rows built inside the timed call (they are part of what the caller pays)"""
    fam = B.FAMILIES[family]
    n = hi - lo + 1
    L, cfg = N.lib(), B._cfg(32, 64, 24)
    a, b = means.reshape(-1), stds.reshape(-1)
    rows = torch.empty((n_streams * n_per, n + 1), dtype=torch.int32, device="cuda")
    idx = (sym.reshape(-1).to(torch.int64) - lo)
    ar = torch.arange(n_streams * n_per, device="cuda")
    stride = (B.max_words if coder == "ans" else B.range_max_words)(n_per, (32, 64, 24))
    out = B._new_batch(n_streams, stride, sym.device, (32, 64, 24))
    dec = torch.empty_like(sym)
    status = torch.empty(n_streams, dtype=torch.int32, device="cuda")
    p, sp = B._ptr, B._stream_ptr

    def tabulate():
        N.check(L.cst_family_cdf_rows(fam, 24, lo, hi, p(a), p(b), None, a.numel(), p(rows), None, sp()), "cst_family_cdf_rows")

    def encode():
        tabulate()
        left = rows[ar, idx].contiguous()
        prob = (rows[ar, idx + 1] - left).contiguous()
        fn = getattr(L, f"cst_{coder}_encode_cp_batch")
        N.check(fn(cfg, p(left), p(prob), n_streams, n_per, N.LAYOUT_STREAM_MAJOR, p(out.words), stride, p(out.n_words), None, p(out.status),
                   N.FLAG_NONE, sp()), "encode_cp")
        return out

    def decode(enc):
        tabulate()
        args_ = [cfg, p(enc.words), None, stride, enc.words.numel(), p(enc.n_words), p(rows), n, lo, p(dec), n_streams, n_per, N.LAYOUT_STREAM_MAJOR, None]
        if coder == "ans":
            args_.append(None)
        N.check(getattr(L, f"cst_{coder}_decode_rows_batch")(*args_, p(status), N.FLAG_NONE, sp()), "decode_rows")
        return dec, status
    return encode, decode


entries = []
for coder in ("ans", "range"):
    for family in args.family:
        for label, form in PARAM_FORMS:
            entries.append((coder, family, label, *family_calls(family, coder, form=form)))
            if family == "gaussian" and len(args.family) > 1:      # the other families have no jump points: like for like
                entries.append((coder, family, label + " without jump points", *family_calls(family, coder, 0, form)))
        if args.rows and family != "gaussian":
            entries.append((coder, family, " by rows", *rows_calls(family, coder)))
results = {i: ([], []) for i in range(len(entries))}
encoded, checked = {}, {}
for i, (coder, family, how, enc_f, dec_f) in enumerate(entries):          # warm-up of every shape and route, and the check
    encoded[i] = enc_f()
    dec, st = dec_f(encoded[i])
    torch.cuda.synchronize()
    checked[i] = bool(torch.equal(dec, sym)) and int(st.abs().sum()) == 0
if args.params == "both":                                                   # (a) against (b): the same words, stream for stream
    for i, (coder, family, how, _, _) in enumerate(entries):
        if "(b)" not in how:
            continue
        j = next(k for k, e in enumerate(entries) if e[:2] == (coder, family) and e[2] == how.replace("(b) f32", "(a) f64, widened beforehand"))
        x, y = encoded[i], encoded[j]
        col = torch.arange(x.words.shape[1], device="cuda")[None, :] < x.n_words[:, None]
        same = bool(torch.equal(x.n_words, y.n_words)) and bool(torch.equal(x.status, y.status)) and bool(torch.equal(x.words * col, y.words * col))
        print(f"{coder:5s} per-symbol {family}{how}: words, counts and statuses equal to (a): {same}")
for _ in range(args.rounds):                                                # alternating: every entry once per round
    for i, (coder, family, how, enc_f, dec_f) in enumerate(entries):
        e, enc = timed(enc_f, args.reps)
        d, _ = timed(lambda: dec_f(enc), args.reps)
        results[i][0].append(e); results[i][1].append(d)
ns = n_streams * n_per
for i, (coder, family, how, _, _) in enumerate(entries):
    es, ds = results[i]
    e, d = statistics.median(es), statistics.median(ds)
    print(f"{coder:5s} per-symbol {family}{how} {n_streams} x {n_per} [{lo}, {hi}]: encode {e:8.3f} ms ({ns / e / 1e6:6.1f} Gsym/s, {min(es):.3f}..{max(es):.3f})  "
          f"decode {d:8.3f} ms ({ns / d / 1e6:6.1f} Gsym/s, {min(ds):.3f}..{max(ds):.3f})  roundtrip_ok={checked[i]}")
