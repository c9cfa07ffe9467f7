#!/usr/bin/env python3
"""Ragged indexed table coding against its neighbours, in one run with alternating calls.

Workload: 16 384 streams of 256 .. 8192 symbols (uniform; the batch of scripts/bench_per_symbol_ragged.py) over -127 .. 127, K = 64
Gaussian tables with log-spaced scales 0.11 .. 64, P = 16, indices uniform, every symbol drawn from the table its index names; uint8 and
int32 indices; lanes scheduled longest stream first (batched.ragged_order) for every candidate.  In the same run:
  (a) plain against jump points (--jump-every, default 256), encode and decode;
  (b) batched.*_gaussian_ragged[_jump] on the same per-symbol (mean, std): what a caller uses today;
  (c) the ragged kernels on a 16 384 x 4224 matrix against the rectangular *_indexed calls: the cost of raggedness.
The entry points are called directly on buffers made once (the Python calls size their slabs with a read-back).  Times are medians of
single launches between HIP events after a warm-up (bench.event_ms), the rounds of the candidates interleaved; `auto_rule` says whether
encode + decode with jump points was below plain in EVERY round.
--select N (default 0: not run): also (s) random access through batched.{coder}_decode_indexed_ragged_select on the
batch of (a) with --jump-every's table, in the same run, alternating single calls: N whole streams drawn at random through the select call
beside the route without it -- the full decode through the jump table (and by whole streams) plus a device gather of the same symbols;
N ranges of 64 symbols at random depths with the table and without it; and ALL streams in order through the select call beside the jump
decode of the same batch (what the SELECT form itself costs, call against call).  `*_prepared`: the entry point alone on queries
prepared once (no sizing read-back).  --only-select leaves (a) .. (c) out.
usage: bench_indexed_ragged.py [--coder ans|range|both] [--jump-every I] [--streams N] [--rounds R] [--select N [--only-select]]
                               [--out profiles/indexed_ragged.json]"""
import argparse
import dataclasses
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench
from constriction_amd import _native as N
from constriction_amd import batched as B

LO, HI, K, P = -127, 127, 64, 16
CFG = (32, 64, P)


def draw(idx, cdfs, seed):
    """flat symbols, each from the table its index names (the quantile function of a uniform P-bit draw)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    inner = torch.from_numpy(cdfs[:, 1:-1].astype(np.int64)).cuda()
    sym = torch.empty(idx.numel(), dtype=torch.int32, device="cuda")
    step = 1 << 24
    for a in range(0, idx.numel(), step):
        part = idx[a:a + step].to(torch.int64)
        q = torch.randint(0, 1 << P, part.shape, generator=g, device="cuda")
        out = sym[a:a + step]
        for k in range(cdfs.shape[0]):
            m = part == k
            out[m] = (torch.searchsorted(inner[k], q[m], right=True) + LO).to(torch.int32)
    return sym


def rounds_of(fns, rounds, reps=3):
    """{name: [ms per round]}: `rounds` rounds over all candidates in turn, each timed by bench.event_ms"""
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(bench.event_ms(fn, reps))
    return times


def summary(times):
    return {name: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4)} for name, t in times.items()}


def native_calls(coder, enc, model_enc, head, model_dec, off, order, out, every):
    """closures over the entry points `name`[_jump] for a batch the Python layer has made once: (encode, decode) of the plain form if
    `every` is 0, else of the jump form.  model_enc / head / model_dec: what _encode_ragged_slabs / _decode_ragged_slabs splice in"""
    lib, cfg, n = N.lib(), B._cfg(*CFG), off.numel() - 1
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    name_e, name_d = model_enc[0], model_dec[0]
    if not every:
        def encode():
            N.check(getattr(lib, name_e)(cfg, *model_enc[1], B._ptr(off), n, B._ptr(order), B._ptr(enc.words), B._ptr(enc.word_offsets), 0,
                                         B._ptr(enc.n_words), B._ptr(enc.status), B._stream_ptr()))

        def decode():
            N.check(getattr(lib, name_d)(cfg, *head, B._ptr(enc.words), B._ptr(enc.word_offsets), 0, enc.words.numel(), B._ptr(enc.n_words),
                                         *model_dec[1], B._ptr(out), B._ptr(off), n, B._ptr(order), B._ptr(status), B._stream_ptr()))
        return encode, decode
    jump = enc.jump
    arrays = (jump.pos, jump.state) if coder == "ans" else (jump.pos, jump.lower, jump.range)
    n_chunks = min(int(t.numel()) for t in arrays)
    scratch = torch.empty(lib.cst_persymbol_ragged_jump_scratch_bytes(n_chunks), dtype=torch.uint8, device="cuda")

    def encode():
        N.check(getattr(lib, name_e + "_jump")(cfg, *model_enc[1], B._ptr(off), n, B._ptr(order), B._ptr(enc.words), B._ptr(enc.word_offsets), 0,
                                               B._ptr(enc.n_words), every, B._ptr(jump.chunk_offsets), *(B._ptr(t) for t in arrays),
                                               B._ptr(enc.status), B._stream_ptr()))

    def decode():
        N.check(getattr(lib, name_d + "_jump")(cfg, *head, B._ptr(enc.words), B._ptr(enc.word_offsets), 0, enc.words.numel(), B._ptr(enc.n_words),
                                               *model_dec[1], B._ptr(out), B._ptr(off), n, every, B._ptr(jump.chunk_offsets), n_chunks,
                                               *(B._ptr(t) for t in arrays), B._ptr(scratch), B._ptr(status), B._stream_ptr()))
    return encode, decode


def timed(fn):
    """one run of fn() between two device events on the current stream: ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(candidates, n):
    """every candidate once for warm-up, then n rounds of all of them in turn, one call each: {name: [ms per round]}"""
    for fn in candidates.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in candidates}
    for _ in range(n):
        for k, fn in candidates.items():
            times[k].append(timed(fn))
    return times


def select_section(coder, tables, sym, idx, off, lengths, order, every, n_sel, rounds):
    """(s) of the module text for one coder and one index type: checked against the input, then timed"""
    n = off.numel() - 1
    dec_ix, sel = getattr(B, f"{coder}_decode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged_select")
    enc_t = getattr(B, f"{coder}_encode_indexed_ragged")(sym, idx, off, tables, CFG, order=order, jump_every=every)
    enc_0 = dataclasses.replace(enc_t, jump=None)
    assert int(enc_t.status.abs().sum().item()) == 0
    g = torch.Generator(device="cuda").manual_seed(7)
    q_streams = torch.randint(0, n, (n_sel,), generator=g, dtype=torch.int64, device="cuda")
    q_len = lengths[q_streams]
    q_count = torch.clamp(q_len, max=64)
    q_first = (torch.rand(n_sel, generator=g, dtype=torch.float64, device="cuda") * (q_len - q_count + 1).to(torch.float64)).to(torch.int64)
    q_first = torch.minimum(q_first, q_len - q_count)

    def gather_index(first, count):
        """the elements of `sym` that the queries (q_streams, first, count) ask for, in their order"""
        ends = torch.cumsum(count, 0)
        starts = ends - count
        k = torch.arange(int(ends[-1]), dtype=torch.int64, device="cuda")
        q = torch.searchsorted(ends, k, right=True)
        return off[q_streams[q]] + first[q] + (k - starts[q])

    idx_whole, idx_range = gather_index(torch.zeros_like(q_len), q_len), gather_index(q_first, q_count)
    every_stream = torch.arange(n, dtype=torch.int64, device="cuda")
    dec, out_all = torch.empty_like(sym), torch.empty_like(sym)
    checks = [(sel(enc_t, idx, off, tables, q_streams), sym[idx_whole]), (sel(enc_t, idx, off, tables, q_streams, q_first, q_count), sym[idx_range]),
              (sel(enc_0, idx, off, tables, q_streams, q_first, q_count), sym[idx_range]), (sel(enc_t, idx, off, tables, every_stream, out=out_all), sym)]
    torch.cuda.synchronize()
    kernel = B.last_kernel()
    ok = kernel == f"{coder}_decode_indexed_ragged_kernel<select>" and \
        all(bool(torch.equal(got, want)) and int(status.abs().sum()) == 0 for (got, _, status), want in checks)
    del checks
    # the entry point alone: the queries prepared once, as _decode_indexed_ragged_select prepares them
    name = f"cst_{coder}_decode_indexed_ragged_select"
    model = (B._ptr(idx), idx.element_size())
    prepared = {}
    for tag, e, (first, count), out in (("whole", enc_t, (None, None), None), ("ranges", enc_t, (q_first, q_count), None),
                                        ("ranges_no_table", enc_0, (q_first, q_count), None), ("all", enc_t, (None, None), out_all)):
        r = B._select_queries(e, e.jump, off, every_stream if tag == "all" else q_streams, first, count, out)
        prepared[tag] = (e, r)
    pieces = {tag: int(r.piece_offsets[-1].item()) for tag, (_, r) in prepared.items()}
    call = lambda tag: B._persymbol_select_call(name, coder, prepared[tag][0], prepared[tag][0].jump, prepared[tag][1], (tables._h,), model)
    candidates = {"select_whole": lambda: sel(enc_t, idx, off, tables, q_streams),
                  "full_jump_gather": lambda: dec_ix(enc_t, idx, off, tables, out=dec)[0][idx_whole],
                  "full_plain_gather": lambda: dec_ix(enc_0, idx, off, tables, out=dec, order=order)[0][idx_whole],
                  "select_ranges": lambda: sel(enc_t, idx, off, tables, q_streams, q_first, q_count),
                  "select_ranges_no_table": lambda: sel(enc_0, idx, off, tables, q_streams, q_first, q_count),
                  "select_all": lambda: sel(enc_t, idx, off, tables, every_stream, out=out_all),
                  "full_jump": lambda: dec_ix(enc_t, idx, off, tables, out=dec),
                  "select_whole_prepared": lambda: call("whole"), "select_ranges_prepared": lambda: call("ranges"),
                  "select_ranges_no_table_prepared": lambda: call("ranges_no_table"), "select_all_prepared": lambda: call("all")}
    times = alternate(candidates, rounds)
    med = summary(times)
    m = lambda k: med[k]["median_ms"]
    return {"ok": ok, "kernel": kernel, "queries": n_sel, "whole_symbols": int(idx_whole.numel()), "range_symbols": int(idx_range.numel()),
            "table_every": every, "launches": 4, "pieces": pieces, "times": med, "per_round_ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
            "ratios": {"select_whole_over_full_jump_gather": round(m("select_whole") / m("full_jump_gather"), 3),
                       "select_whole_prepared_over_full_jump_gather": round(m("select_whole_prepared") / m("full_jump_gather"), 3),
                       "select_ranges_over_full_jump_gather": round(m("select_ranges") / m("full_jump_gather"), 3),
                       "select_ranges_over_no_table": round(m("select_ranges") / m("select_ranges_no_table"), 3),
                       "select_ranges_prepared_over_no_table_prepared": round(m("select_ranges_prepared") / m("select_ranges_no_table_prepared"), 3),
                       "select_all_over_full_jump": round(m("select_all") / m("full_jump"), 3),
                       "select_all_prepared_over_full_jump": round(m("select_all_prepared") / m("full_jump"), 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coder", default="both", choices=["ans", "range", "both"])
    ap.add_argument("--jump-every", type=int, default=256)
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--min-len", type=int, default=256)
    ap.add_argument("--max-len", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--select", type=int, default=0, help="also time random access: N whole streams, and N ranges of 64 symbols")
    ap.add_argument("--only-select", action="store_true", help="with --select: leave (a), (b) and (c) out")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, every = a.streams, a.jump_every
    g = torch.Generator(device="cuda").manual_seed(1)
    lengths = torch.randint(a.min_len, a.max_len + 1, (n,), generator=g, device="cuda", dtype=torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lengths, 0, out=off[1:])
    total = int(off[-1].item())
    order = B.ragged_order(lengths)
    stds, means = np.geomspace(0.11, 64.0, K), np.zeros(K)
    tables = B.TableSet.quantized_gaussians(LO, HI, means, stds, P)
    idx32 = torch.randint(0, K, (total,), generator=g, device="cuda", dtype=torch.int32)
    idx8 = idx32.to(torch.uint8)
    sym = draw(idx32, tables.cdfs(), 116)
    d_means = torch.from_numpy(means).cuda()[idx32.long()]
    d_stds = torch.from_numpy(stds).cuda()[idx32.long()]
    out = torch.empty_like(sym)
    result = {"workload": {"streams": n, "lengths": [a.min_len, a.max_len], "symbols": total, "support": [LO, HI], "tables": K, "stds": [0.11, 64.0],
                           "precision": P, "jump_every": every, "order": "longest first"}, "coders": {}}

    if a.select and not every:
        ap.error("--select times the table's routes: give --jump-every")
    for coder in (("ans", "range") if a.coder == "both" else (a.coder,)):
        if a.select:
            result.setdefault("select", {})[coder] = {tag: select_section(coder, tables, sym, idx, off, lengths, order, every, a.select, a.rounds)
                                                      for tag, idx in (("u8", idx8), ("i32", idx32))}
            torch.cuda.empty_cache()
            if a.only_select:
                continue
        enc_ix, dec_ix = getattr(B, f"{coder}_encode_indexed_ragged"), getattr(B, f"{coder}_decode_indexed_ragged")
        enc_g, dec_g = getattr(B, f"{coder}_encode_gaussian_ragged"), getattr(B, f"{coder}_decode_gaussian_ragged")
        fns, kernels = {}, {}
        for tag, idx in (("u8", idx8), ("i32", idx32)):
            for form, I in (("plain", 0), ("jump", every)):
                enc = enc_ix(sym, idx, off, tables, CFG, order=order, jump_every=I)
                kernels[f"encode_{form}"] = B.last_kernel()
                got, status = dec_ix(enc, idx, off, tables, out=out)
                kernels[f"decode_{form}"] = B.last_kernel()
                assert torch.equal(got, sym) and int(status.abs().sum().item()) == 0 and int(enc.status.abs().sum().item()) == 0
                e, d = native_calls(coder, enc, (f"cst_{coder}_encode_indexed_ragged", (tables._h, B._ptr(sym), B._ptr(idx), idx.element_size())),
                                    (tables._h,), (f"cst_{coder}_decode_indexed_ragged", (B._ptr(idx), idx.element_size())), off, order, out, I)
                fns[f"encode_indexed_{tag}_{form}"], fns[f"decode_indexed_{tag}_{form}"] = e, d
        for form, I in (("plain", 0), ("jump", every)):
            enc = enc_g(sym, off, LO, HI, d_means, d_stds, CFG, order=order, jump_every=I)
            got, status = dec_g(enc, off, LO, HI, d_means, d_stds, out=out)
            assert torch.equal(got, sym) and int(status.abs().sum().item()) == 0
            e, d = native_calls(coder, enc, (f"cst_{coder}_encode_gaussian_ragged", (LO, HI, B._ptr(sym), B._ptr(d_means), B._ptr(d_stds))), (LO, HI),
                                (f"cst_{coder}_decode_gaussian_ragged", (B._ptr(d_means), B._ptr(d_stds))), off, order, out, I)
            fns[f"encode_gaussian_{form}"], fns[f"decode_gaussian_{form}"] = e, d
        times = rounds_of(fns, a.rounds)
        row = {"kernels": kernels, "times": summary(times)}
        # (a) the rule of jump_every="auto": encode + decode with jump points below plain in EVERY alternation, for either index type
        row["auto_rule"] = {}
        for tag in ("u8", "i32"):
            plain = np.add(times[f"encode_indexed_{tag}_plain"], times[f"decode_indexed_{tag}_plain"])
            jump = np.add(times[f"encode_indexed_{tag}_jump"], times[f"decode_indexed_{tag}_jump"])
            row["auto_rule"][tag] = {"plain_ms_per_round": [round(float(x), 4) for x in plain], "jump_ms_per_round": [round(float(x), 4) for x in jump],
                                     "jump_below_plain_in_every_round": bool((jump < plain).all())}
        med = row["times"]
        row["over_gaussian"] = {f"{d}_{form}": round(med[f"{d}_indexed_u8_{form}"]["median_ms"] / med[f"{d}_gaussian_{form}"]["median_ms"], 3)
                                for d in ("encode", "decode") for form in ("plain", "jump")}
        del fns, enc
        torch.cuda.empty_cache()

        # (c) equal lengths: the ragged kernels on a matrix against the rectangular calls
        per = min((a.min_len + a.max_len) // 2, total // n)
        m_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * per
        m_sym, m_idx8, m_idx32 = sym[: n * per].reshape(n, per), idx8[: n * per].reshape(n, per), idx32[: n * per].reshape(n, per)
        m_out = torch.empty_like(m_sym)
        fns = {}
        for tag, idx in (("u8", m_idx8), ("i32", m_idx32)):
            rect = getattr(B, f"{coder}_encode_indexed")(m_sym, idx, tables, CFG)
            rag = enc_ix(m_sym.reshape(-1), idx.reshape(-1), m_off, tables, CFG, order=None)
            assert torch.equal(rect.n_words, rag.n_words)
            assert torch.equal(getattr(B, f"{coder}_decode_indexed")(rect, idx, tables, per, out=m_out)[0], m_sym)
            assert torch.equal(dec_ix(rag, idx.reshape(-1), m_off, tables, out=m_out.reshape(-1))[0], m_sym.reshape(-1))
            e, d = native_calls(coder, rag, (f"cst_{coder}_encode_indexed_ragged", (tables._h, B._ptr(m_sym), B._ptr(idx), idx.element_size())),
                                (tables._h,), (f"cst_{coder}_decode_indexed_ragged", (B._ptr(idx), idx.element_size())), m_off, None, m_out, 0)
            fns[f"encode_ragged_{tag}"], fns[f"decode_ragged_{tag}"] = e, d
            fns[f"encode_rectangular_{tag}"] = lambda idx=idx, rect=rect: getattr(B, f"{coder}_encode_indexed")(m_sym, idx, tables, CFG, out=rect)
            fns[f"decode_rectangular_{tag}"] = lambda idx=idx, rect=rect: getattr(B, f"{coder}_decode_indexed")(rect, idx, tables, per, out=m_out)
        med = summary(rounds_of(fns, a.rounds))
        row["matrix"] = {"streams": n, "symbols_per_stream": per, "times": med,
                         "ragged_over_rectangular": {f"{d}_{tag}": round(med[f"{d}_ragged_{tag}"]["median_ms"] / med[f"{d}_rectangular_{tag}"]["median_ms"], 3)
                                                     for d in ("encode", "decode") for tag in ("u8", "i32")}}
        result["coders"][coder] = row
        del fns, rect, rag, m_out
        torch.cuda.empty_cache()

    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
