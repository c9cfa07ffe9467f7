#!/usr/bin/env python3
"""Per-symbol models for streams of different lengths: 16 384 streams of 256 .. 8192 symbols (uniform) at (32,64,24), support
-100 .. 100, parameters drawn as in tests/test_gpu_per_symbol_batch.py::workload, through
  (a) batched.{coder}_{encode,decode}_{family}_ragged: one launch each (as the streams come, and once more sorted by length);
  (b) the bit-exact alternative without them: the streams grouped by length, one {coder}_{encode,decode}_{family} call per distinct
      length (the groups' matrices are built beforehand and not timed);
  (c) the price of raggedness: the rectangular calls on a 16 384 x 4224 matrix (the same number of symbols) beside the ragged calls
      on that same matrix expressed with equal lengths.
--jump-every N (a multiple of 16; default 0: not run): also (j) the same batch with a jump point every N symbols of every stream --
`jump_every=N` of the encoder, and the decode of all chunks side by side -- timed beside the plain pair of (a) in the same run,
alternating; recorded per alternation, with the size of the table against the words.  No condition on it.
--select N (default 0: not run): also (s) random access through
batched.{coder}_decode_{family}[_perfect]_ragged_select on the batch of (a) -- with --jump-every's table where that is given -- timed in the same
run, alternating: N whole streams drawn at random through the select call; the full decode (whole streams, and through the jump table)
followed by a device gather of the same streams (the gather's index is built beforehand and not timed), which is all a caller had
before; N ranges of 64 symbols at random depths with the table and without it; and ALL streams in order through the select call beside
the jump decode of the same batch (what the SELECT form's second index and store predicate cost: call against call, the select call's
four launches, prefix sums and read-back included).  Recorded, no condition on it beyond the symbols being right.
--coder ans|range and --family gaussian|laplace|cauchy|categorical choose the form (default: ans, gaussian); --skip-grouped leaves (b)
out (it takes seconds per alternation and minutes to set up; its condition is then not judged).
--family categorical --k K: every symbol has its own row of K float32 probabilities (exp(3 z), z normal: not normalised; symbols drawn
from the rows) in place of (mean, std) -- symbols x K x 4 bytes for the ragged batch and as much again for (c), so K has to fit memory.
--perfect (with --family categorical): Categorical(perfect=True) -- the *_categorical_perfect_ragged calls beside *_categorical(...,
perfect=True).  A wave quantises ONE row (millions of rows a second, not billions): take a batch of minutes, not hours, with --streams,
--min-len and --max-len.
--params f64|f32|both (gaussian, laplace, cauchy; default f64): the element type of the parameter arrays.  f32: float32 arrays
everywhere, read by the kernels themselves (the _f32 entry points).  both: the values are rounded to float32 first, everything above
runs on them widened beforehand, and (p) times the ragged pair -- with --jump-every's table and --select's ranges where those are given --
through (a) the float64 call on the arrays widened beforehand, (b) the float32 call, and (c) what a float32 caller paid before:
`.double()` of both arrays inside the timed region plus the float64 call; alternating, medians and ranges; the words, tables and
decoded symbols of (a) and (b) are compared at the timed size.
Device events on the launch stream, warmed up, in one process, the candidates alternating, medians of the alternations.  Every
stream is checked by the decode round trip.  The one condition: (a) is faster than (b) in every alternation (exit status 1 otherwise);
(c) is a recorded ratio."""
import argparse, functools, json, statistics, sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from constriction_amd import batched as B

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=16384)
ap.add_argument("--min-len", type=int, default=256)
ap.add_argument("--max-len", type=int, default=8192)
ap.add_argument("--alternations", type=int, default=5)
ap.add_argument("--coder", choices=["ans", "range"], default="ans")
ap.add_argument("--family", choices=["gaussian", "laplace", "cauchy", "categorical"], default="gaussian")
ap.add_argument("--k", type=int, default=16, help="--family categorical: entries of a probability row")
ap.add_argument("--perfect", action="store_true", help="--family categorical: Categorical(perfect=True), quantised by the device quantiser")
ap.add_argument("--jump-every", type=int, default=0, help="also time the pair with a jump point every N symbols (a multiple of 16)")
ap.add_argument("--select", type=int, default=0, help="also time random access: N whole streams, and N ranges of 64 symbols")
ap.add_argument("--params", choices=["f64", "f32", "both"], default="f64", help="element type of the parameter arrays (see above)")
ap.add_argument("--skip-rectangular", action="store_true", help="leave (c), the rectangular matrix, out")
ap.add_argument("--skip-grouped", action="store_true", help="leave (b), one rectangular call per distinct length, out")
args = ap.parse_args()
assert args.alternations >= 5 or args.streams < 16384, "the recorded figures are medians of at least five alternations"
assert not args.perfect or args.family == "categorical", "--perfect goes with --family categorical"
assert args.params == "f64" or args.family != "categorical", "--params is about (mean, std) / (a, b) arrays"

CFG, LO, HI = (32, 64, 24), -100, 100
torch.manual_seed(1)
dev = "cuda"
FORM = args.family + ("_perfect" if args.perfect else "")
enc_ragged, dec_ragged = getattr(B, f"{args.coder}_encode_{FORM}_ragged"), getattr(B, f"{args.coder}_decode_{FORM}_ragged")
enc_rect, dec_rect = getattr(B, f"{args.coder}_encode_{args.family}"), getattr(B, f"{args.coder}_decode_{args.family}")
if args.perfect:
    enc_rect, dec_rect = functools.partial(enc_rect, perfect=True), functools.partial(dec_rect, perfect=True)
F32_TAG = ", f32" if args.params == "f32" else ""
JUMP_KERNEL = f"{args.coder}_decode_categorical_perfect_ragged_by_rows<jump>" if args.perfect else f"{args.coder}_decode_{args.family}_ragged_kernel<jump{F32_TAG}>"
SELECT_KERNEL = JUMP_KERNEL.replace("<jump", "<select")
NO_JUMP = {"jump_points": 0} if args.family == "gaussian" else {}      # (the family calls have no jump points to switch off)
CATEGORICAL = args.family == "categorical"
HEAD = () if CATEGORICAL else (LO, HI)                                  # what the calls take in front of the model's tensors


def draw(*shape):
    """mu uniform in 0.6 [lo, hi], sd log-uniform in 0.3 .. 40, symbols = clipped rounded draws from the family; returns (symbols, the
    model's tensors)"""
    if CATEGORICAL:
        probs = torch.randn(*shape, args.k, dtype=torch.float32, device=dev).mul_(3.0).exp_()      # (in place: the matrix is the memory)
        sym = torch.empty(shape, dtype=torch.int32, device=dev)
        flat_p, flat_s = probs.view(-1, args.k), sym.view(-1)
        for i in range(0, flat_s.numel(), 1 << 22):           # (multinomial takes at most 2^24 rows a call)
            flat_s[i: i + (1 << 22)] = torch.multinomial(flat_p[i: i + (1 << 22)], 1).view(-1).to(torch.int32)
        return sym, (probs,)
    mu = (torch.rand(*shape, dtype=torch.float64, device=dev) * 2 - 1) * (0.6 * HI)
    sd = torch.exp(torch.log(torch.tensor(0.3, dtype=torch.float64, device=dev))
                   + torch.rand(*shape, dtype=torch.float64, device=dev) * torch.log(torch.tensor(40.0 / 0.3, dtype=torch.float64, device=dev)))
    if args.params != "f64":                   # float32-representable values: every form codes the same models
        mu, sd = mu.float().double(), sd.float().double()
    if args.family == "gaussian":
        noise = torch.randn(*shape, dtype=torch.float64, device=dev)
    else:
        u = torch.rand(*shape, dtype=torch.float64, device=dev) - 0.5
        noise = -torch.sign(u) * torch.log1p(-2 * u.abs()) if args.family == "laplace" else torch.tan(torch.pi * u)
    sym = torch.clamp(torch.round(mu + sd * noise), LO, HI).to(torch.int32)
    return sym, ((mu.float(), sd.float()) if args.params == "f32" else (mu, sd))


def timed(fn):
    """one run of fn() between two device events on the current stream: ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(candidates, n):
    """candidates: {name: fn}; every fn once for warm-up, then n rounds of all of them in turn.  Returns {name: [ms per round]}"""
    for fn in candidates.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in candidates}
    for _ in range(n):
        for k, fn in candidates.items():
            times[k].append(timed(fn))
    return times


# ---- the ragged batch ----
n = args.streams
lengths = torch.randint(args.min_len, args.max_len + 1, (n,), dtype=torch.int64, device=dev)
offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
torch.cumsum(lengths, 0, out=offsets[1:])
total = int(offsets[-1])
sym, model = draw(total)

enc = enc_ragged(sym, offsets, *HEAD, *model, CFG)
dec, st = dec_ragged(enc, offsets, *HEAD, *model)
torch.cuda.synchronize()
ok_a = bool(torch.equal(dec, sym)) and int(enc.status.abs().sum()) == 0 and int(st.abs().sum()) == 0

# ---- (b): one rectangular batch per distinct length ----
order = torch.argsort(lengths, stable=True)
sorted_len = lengths[order].cpu().tolist() if not args.skip_grouped else []
order_h, off_h = order.cpu().tolist(), offsets.cpu().tolist()
groups = []          # (streams, symbols, the model's tensors) per distinct length
i = 0 if not args.skip_grouped else n
while i < n:
    j = i
    while j < n and sorted_len[j] == sorted_len[i]:
        j += 1
    L = sorted_len[i]
    rows = order_h[i:j]
    idx = torch.cat([torch.arange(off_h[s], off_h[s] + L, device=dev) for s in rows])
    groups.append((rows, sym[idx].reshape(len(rows), L), tuple(m[idx].reshape(len(rows), L, *m.shape[1:]) for m in model)))
    i = j
group_enc = [None] * len(groups)
group_dec = [None] * len(groups)


def b_encode():
    for g, (_, s_, m_) in enumerate(groups):
        group_enc[g] = enc_rect(s_, *HEAD, *m_, CFG, **NO_JUMP)


def b_decode():
    for g, (_, s_, m_) in enumerate(groups):
        group_dec[g] = dec_rect(group_enc[g], *HEAD, *m_)


b_encode(); b_decode()
torch.cuda.synchronize()
ok_b = all(bool(torch.equal(group_dec[g][0], groups[g][1])) and int(group_dec[g][1].abs().sum()) == 0 and int(group_enc[g].status.abs().sum()) == 0
           for g in range(len(groups)))
# (b) writes the words (a) writes: the word counts of every stream agree
n_words_b = torch.zeros(n, dtype=torch.int32, device=dev)
for g, (rows, *_rest) in enumerate(groups):
    n_words_b[torch.tensor(rows, device=dev)] = group_enc[g].n_words
ok_b = ok_b and (args.skip_grouped or bool(torch.equal(n_words_b, enc.n_words)))

# (a) once more with a schedule (streams of similar length side by side, the sort itself not timed): recorded, no condition on it
by_length = B.ragged_order(lengths)
enc_s = enc_ragged(sym, offsets, *HEAD, *model, CFG, order=by_length)
dec_s, st_s = dec_ragged(enc_s, offsets, *HEAD, *model)
torch.cuda.synchronize()
ok_a = ok_a and bool(torch.equal(dec_s, sym)) and int(st_s.abs().sum()) == 0 and bool(torch.equal(enc_s.n_words, enc.n_words))

t_ab = alternate({"a_encode": lambda: enc_ragged(sym, offsets, *HEAD, *model, CFG),
                  "b_encode": b_encode,
                  "a_sorted_encode": lambda: enc_ragged(sym, offsets, *HEAD, *model, CFG, order=by_length),
                  "a_decode": lambda: dec_ragged(enc, offsets, *HEAD, *model, out=dec),
                  "b_decode": b_decode,
                  "a_sorted_decode": lambda: dec_ragged(enc_s, offsets, *HEAD, *model, out=dec_s)}, args.alternations)
faster = args.skip_grouped or (all(a < b for a, b in zip(t_ab["a_encode"], t_ab["b_encode"]))
                               and all(a < b for a, b in zip(t_ab["a_decode"], t_ab["b_decode"])))
del groups, group_enc, group_dec

# ---- (j): jump points, beside the plain pair ----
ok_j, t_j, jump_info = True, {}, None
if args.jump_every:
    enc_j = enc_ragged(sym, offsets, *HEAD, *model, CFG, jump_every=args.jump_every)
    dec_j, st_j = dec_ragged(enc_j, offsets, *HEAD, *model)
    torch.cuda.synchronize()
    ok_j = (B.last_kernel() == JUMP_KERNEL and bool(torch.equal(dec_j, sym)) and int(st_j.abs().sum()) == 0
            and int(enc_j.status.abs().sum()) == 0 and bool(torch.equal(enc_j.n_words, enc.n_words)))
    t_j = alternate({"plain_encode": lambda: enc_ragged(sym, offsets, *HEAD, *model, CFG),
                     "jump_encode": lambda: enc_ragged(sym, offsets, *HEAD, *model, CFG, jump_every=args.jump_every),
                     "plain_decode": lambda: dec_ragged(enc, offsets, *HEAD, *model, out=dec),
                     "jump_decode": lambda: dec_ragged(enc_j, offsets, *HEAD, *model, out=dec_j)}, args.alternations)
    n_chunks = int(enc_j.jump.chunk_offsets[-1])
    jump_info = {"every": args.jump_every, "chunks": n_chunks, "table_bytes": n_chunks * (12 if args.coder == "ans" else 20),
                 "word_bytes": 4 * int(enc.n_words.sum()),
                 "pair_lower_in_every_alternation": all(je + jd < pe + pd for pe, pd, je, jd in zip(t_j["plain_encode"], t_j["plain_decode"],
                                                                                                    t_j["jump_encode"], t_j["jump_decode"]))}

# ---- (s): random access, beside the full decode and a gather ----
ok_s, t_s, select_info = True, {}, None
if args.select:
    sel_ragged = getattr(B, f"{args.coder}_decode_{FORM}_ragged_select")
    enc_t = enc_j if args.jump_every else enc                   # the batch with its table, where one was asked for
    enc_0 = enc                                                 # ... and the same words without one
    q_streams = torch.randint(0, n, (args.select,), dtype=torch.int64, device=dev)
    q_len = lengths[q_streams]
    q_count = torch.clamp(q_len, max=64)
    q_first = (torch.rand(args.select, dtype=torch.float64, device=dev) * (q_len - q_count + 1).to(torch.float64)).to(torch.int64)
    q_first = torch.minimum(q_first, q_len - q_count)

    def gather_index(first, count):
        """the elements of `sym` that the queries (q_streams, first, count) ask for, in their order"""
        ends = torch.cumsum(count, 0)
        starts = ends - count
        k = torch.arange(int(ends[-1]), dtype=torch.int64, device=dev)
        q = torch.searchsorted(ends, k, right=True)
        return offsets[q_streams[q]] + first[q] + (k - starts[q])

    idx_whole, idx_range = gather_index(torch.zeros_like(q_len), q_len), gather_index(q_first, q_count)
    want_whole, want_range = sym[idx_whole], sym[idx_range]
    every_stream = torch.arange(n, dtype=torch.int64, device=dev)
    out_all = torch.empty_like(sym)
    checks = [(sel_ragged(enc_t, offsets, *HEAD, *model, q_streams), want_whole),
              (sel_ragged(enc_t, offsets, *HEAD, *model, q_streams, q_first, q_count), want_range),
              (sel_ragged(enc_0, offsets, *HEAD, *model, q_streams, q_first, q_count), want_range),
              (sel_ragged(enc_t, offsets, *HEAD, *model, every_stream, out=out_all), sym)]
    torch.cuda.synchronize()
    ok_s = B.last_kernel() == SELECT_KERNEL and \
        all(bool(torch.equal(got, want)) and int(status.abs().sum()) == 0 for (got, _, status), want in checks)
    del checks
    candidates = {"select_whole": lambda: sel_ragged(enc_t, offsets, *HEAD, *model, q_streams),
                  "full_plain_gather": lambda: dec_ragged(enc_0, offsets, *HEAD, *model, out=dec)[0][idx_whole],
                  "select_ranges": lambda: sel_ragged(enc_t, offsets, *HEAD, *model, q_streams, q_first, q_count),
                  "select_ranges_no_table": lambda: sel_ragged(enc_0, offsets, *HEAD, *model, q_streams, q_first, q_count),
                  "select_all": lambda: sel_ragged(enc_t, offsets, *HEAD, *model, every_stream, out=out_all)}
    if args.jump_every:
        candidates["full_jump_gather"] = lambda: dec_ragged(enc_t, offsets, *HEAD, *model, out=dec_j)[0][idx_whole]
        candidates["full_jump"] = lambda: dec_ragged(enc_t, offsets, *HEAD, *model, out=dec_j)
    t_s = alternate(candidates, args.alternations)
    select_info = {"queries": args.select, "whole_symbols": int(idx_whole.numel()), "range_symbols": int(idx_range.numel()),
                   "table_every": args.jump_every}
    del out_all, idx_whole, idx_range, want_whole, want_range
# ---- (p): float32 parameters, beside the float64 call and the conversion a float32 caller paid before ----
ok_p, t_p, params_info = True, {}, None
if args.params == "both":
    m32 = tuple(m.float() for m in model)
    widened = lambda: tuple(m.double() for m in m32)
    je = {"jump_every": args.jump_every} if args.jump_every else {}
    enc_a = enc_j if args.jump_every else enc
    enc_b = enc_ragged(sym, offsets, *HEAD, *m32, CFG, **je)
    name_b = B.last_kernel()
    dec_b, st_b = dec_ragged(enc_b, offsets, *HEAD, *m32)
    name_b = (name_b, B.last_kernel())
    torch.cuda.synchronize()
    same = bool(torch.equal(enc_b.n_words, enc_a.n_words)) and bool(torch.equal(enc_b.status, enc_a.status)) and \
        bool(torch.equal(enc_b.word_offsets, enc_a.word_offsets))
    if same:                                   # every stream's words (what lies behind them in a slab was never written)
        pos = torch.arange(enc_a.words.numel(), dtype=torch.int64, device=dev)
        owner = torch.searchsorted(enc_a.word_offsets[1:].contiguous(), pos, right=True).clamp(max=n - 1)
        written = pos < enc_a.word_offsets[owner] + enc_a.n_words[owner]
        same = bool(torch.equal(enc_b.words[written], enc_a.words[written]))
        del pos, owner, written
    if args.jump_every:
        k = int(enc_a.jump.chunk_offsets[-1])
        fields = ("pos", "state") if args.coder == "ans" else ("pos", "lower", "range")
        same = same and all(bool(torch.equal(getattr(enc_b.jump, f)[:k], getattr(enc_a.jump, f)[:k])) for f in fields)
    ok_p = same and all("f32" in x for x in name_b) and bool(torch.equal(dec_b, sym)) and int(st_b.abs().sum()) == 0
    dec_p = torch.empty_like(sym)
    cands = {"a_encode": lambda: enc_ragged(sym, offsets, *HEAD, *model, CFG, **je),
             "b_encode": lambda: enc_ragged(sym, offsets, *HEAD, *m32, CFG, **je),
             "c_encode": lambda: enc_ragged(sym, offsets, *HEAD, *widened(), CFG, **je),
             "a_decode": lambda: dec_ragged(enc_a, offsets, *HEAD, *model, out=dec_p),
             "b_decode": lambda: dec_ragged(enc_a, offsets, *HEAD, *m32, out=dec_p),
             "c_decode": lambda: dec_ragged(enc_a, offsets, *HEAD, *widened(), out=dec_p),
             "conversion_alone": widened}
    if args.select:
        got_b = sel_ragged(enc_a, offsets, *HEAD, *m32, q_streams, q_first, q_count)
        ok_p = ok_p and "f32" in B.last_kernel() and bool(torch.equal(got_b[0], sym[gather_index(q_first, q_count)])) and int(got_b[2].abs().sum()) == 0
        cands.update({"a_select_ranges": lambda: sel_ragged(enc_a, offsets, *HEAD, *model, q_streams, q_first, q_count),
                      "b_select_ranges": lambda: sel_ragged(enc_a, offsets, *HEAD, *m32, q_streams, q_first, q_count),
                      "c_select_ranges": lambda: sel_ragged(enc_a, offsets, *HEAD, *widened(), q_streams, q_first, q_count)})
    t_p = alternate(cands, args.alternations)
    params_info = {"kernels": list(name_b), "same_words_tables_symbols": ok_p, "jump_every": args.jump_every}
    del m32, dec_p, enc_b, dec_b
if args.jump_every:
    del enc_j, dec_j

# ---- (c): a rectangular matrix of the same size, both ways ----
ok_c, t_c = True, {}
if not args.skip_rectangular:
    n_per = (args.min_len + args.max_len) // 2
    del model
    sym_r, model_r = draw(n, n_per)
    off_r = torch.arange(n + 1, dtype=torch.int64, device=dev) * n_per
    flat_r, model_f = sym_r.reshape(-1), tuple(m.reshape(n * n_per, *m.shape[2:]) for m in model_r)
    enc_r = enc_rect(sym_r, *HEAD, *model_r, CFG, **NO_JUMP)
    dec_r, st_r = dec_rect(enc_r, *HEAD, *model_r)
    enc_e = enc_ragged(flat_r, off_r, *HEAD, *model_f, CFG)
    dec_e, st_e = dec_ragged(enc_e, off_r, *HEAD, *model_f)
    torch.cuda.synchronize()
    ok_c = bool(torch.equal(dec_r, sym_r)) and bool(torch.equal(dec_e, flat_r)) and int(st_r.abs().sum()) == 0 and int(st_e.abs().sum()) == 0 \
        and bool(torch.equal(enc_r.n_words, enc_e.n_words))
    t_c = alternate({"rect_encode": lambda: enc_rect(sym_r, *HEAD, *model_r, CFG, out=enc_r, **NO_JUMP),
                     "ragged_encode": lambda: enc_ragged(flat_r, off_r, *HEAD, *model_f, CFG),
                     "rect_decode": lambda: dec_rect(enc_r, *HEAD, *model_r, out=dec_r),
                     "ragged_decode": lambda: dec_ragged(enc_e, off_r, *HEAD, *model_f, out=dec_e)}, args.alternations)

med = lambda xs: statistics.median(xs)
m_ab = {k: med(v) for k, v in t_ab.items()}
m_c = {k: med(v) for k, v in t_c.items()}
print(f"{args.coder} x {FORM}{f' (K = {args.k}, float32)' if CATEGORICAL else ''}: {n} streams of {args.min_len} .. {args.max_len} symbols ({total / 1e6:.1f} M symbols), (32,64,24), "
      f"medians of {args.alternations}:")
print(f"  (a) ragged calls:               encode {m_ab['a_encode']:9.3f} ms ({total / m_ab['a_encode'] / 1e6:.2f} Gsym/s)  "
      f"decode {m_ab['a_decode']:9.3f} ms ({total / m_ab['a_decode'] / 1e6:.2f} Gsym/s)  round trip ok={ok_a}")
print(f"      ... sorted by length:       encode {m_ab['a_sorted_encode']:9.3f} ms ({total / m_ab['a_sorted_encode'] / 1e6:.2f} Gsym/s)  "
      f"decode {m_ab['a_sorted_decode']:9.3f} ms ({total / m_ab['a_sorted_decode'] / 1e6:.2f} Gsym/s)")
if args.skip_grouped:
    print("  (b) one call per length:       left out (--skip-grouped)")
else:
    print(f"  (b) one call per length:       encode {m_ab['b_encode']:9.3f} ms  decode {m_ab['b_decode']:9.3f} ms  round trip ok={ok_b}")
    print(f"      (a) faster than (b) in every alternation: {faster}")
if args.jump_every:
    m_j = {k: med(v) for k, v in t_j.items()}
    spread = lambda k: f"{min(t_j[k]):.3f} - {max(t_j[k]):.3f}"
    print(f"  (j) a jump point every {args.jump_every} symbols ({jump_info['chunks']} chunks, table {jump_info['table_bytes'] / 1e6:.2f} MB against "
          f"{jump_info['word_bytes'] / 1e6:.1f} MB of words = {100 * jump_info['table_bytes'] / jump_info['word_bytes']:.2f} %), plain beside it:")
    print(f"      plain: encode {m_j['plain_encode']:9.3f} ms ({spread('plain_encode')})  decode {m_j['plain_decode']:9.3f} ms ({spread('plain_decode')})")
    print(f"      jump:  encode {m_j['jump_encode']:9.3f} ms ({spread('jump_encode')}, {m_j['jump_encode'] / m_j['plain_encode']:.3f}x)  "
          f"decode {m_j['jump_decode']:9.3f} ms ({spread('jump_decode')}, {m_j['jump_decode'] / m_j['plain_decode']:.3f}x)  round trip ok={ok_j}")
    print(f"      encode + decode lower with jump points in every alternation: {jump_info['pair_lower_in_every_alternation']}")
if args.select:
    m_s = {k: med(v) for k, v in t_s.items()}
    table = f"a jump point every {args.jump_every} symbols" if args.jump_every else "NO table"
    print(f"  (s) random access, {args.select} queries, {table}:")
    print(f"      {args.select} whole streams ({select_info['whole_symbols'] / 1e6:.2f} M symbols) through the select call: {m_s['select_whole']:9.3f} ms")
    print(f"      full decode + gather of the same streams: whole streams {m_s['full_plain_gather']:9.3f} ms"
          + (f", through the jump table {m_s['full_jump_gather']:9.3f} ms" if args.jump_every else ""))
    print(f"      {args.select} ranges of 64 symbols at random depths: {m_s['select_ranges']:9.3f} ms with the table, "
          f"{m_s['select_ranges_no_table']:9.3f} ms without ({m_s['select_ranges'] / m_s['select_ranges_no_table']:.3f}x)")
    print(f"      all {n} streams in order through the select call: {m_s['select_all']:9.3f} ms"
          + (f" against {m_s['full_jump']:9.3f} ms of the jump decode ({m_s['select_all'] / m_s['full_jump']:.2f}x)" if args.jump_every else "")
          + f"  symbols ok={ok_s}")
if args.params == "both":
    spread_p = lambda k: f"{statistics.median(t_p[k]):9.3f} ms ({min(t_p[k]):.3f} - {max(t_p[k]):.3f})"
    print(f"  (p) float32 parameters{f', a jump point every {args.jump_every} symbols' if args.jump_every else ''}: {params_info['kernels']}, "
          f"words, tables and symbols equal to the float64 call's: {ok_p}")
    for what in ["encode", "decode"] + (["select_ranges"] if args.select else []):
        print(f"      {what:14s} (a) f64, widened beforehand {spread_p('a_' + what)}  (b) f32 {spread_p('b_' + what)}  "
              f"(c) f32 + .double() inside {spread_p('c_' + what)}")
    print(f"      the conversion alone (two .double()): {spread_p('conversion_alone')}")
if args.skip_rectangular:
    print("  (c) rectangular matrix:        left out (--skip-rectangular)")
else:
    print(f"  (c) {n} x {n_per} rectangular:  encode {m_c['rect_encode']:9.3f} ms  decode {m_c['rect_decode']:9.3f} ms")
    print(f"      the same through the ragged calls: encode {m_c['ragged_encode']:9.3f} ms ({m_c['ragged_encode'] / m_c['rect_encode']:.2f}x)  "
          f"decode {m_c['ragged_decode']:9.3f} ms ({m_c['ragged_decode'] / m_c['rect_decode']:.2f}x)  round trips ok={ok_c}")
print(json.dumps({"coder": args.coder, "family": args.family, "perfect": args.perfect, "k": args.k if CATEGORICAL else None, "grouped": not args.skip_grouped, "streams": n, "symbols": total, "alternations": args.alternations, "ms": {**m_ab, **m_c}, "all_ms": {**t_ab, **t_c},
                  "jump": jump_info, "jump_ms": {k: med(v) for k, v in t_j.items()}, "jump_all_ms": t_j,
                  "select": select_info, "select_ms": {k: med(v) for k, v in t_s.items()}, "select_all_ms": t_s,
                  "params": args.params, "params_info": params_info, "params_ms": {k: med(v) for k, v in t_p.items()}, "params_all_ms": t_p,
                  "a_faster_than_b": faster, "round_trips_ok": ok_a and ok_b and ok_c and ok_j and ok_s and ok_p}))
sys.exit(0 if faster and ok_a and ok_b and ok_c and ok_j and ok_s and ok_p else 1)
