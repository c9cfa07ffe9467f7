#!/usr/bin/env python3
"""Randomised parity stress of jump points for RAGGED per-symbol batches against the CPU oracle (not part of the test suite: GPU time
by the minute).  Random batches -- both coders, Gaussian / Laplace / Cauchy, the three presets of the Python API, with or without a
schedule -- with a random `jump_every` in {16, 32, 48, 256}: words and jump table of every stream against one oracle coder coded chunk
by chunk (tests/persymbol_jump_oracle.py), the decode of the chunks side by side, and the plain call's words.
usage: python tests/stress/stress_persymbol_ragged_jump.py [seconds] [seed]"""
import sys, time
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from constriction_amd import batched as B
from oracle import oracle as O
from persymbol_jump_oracle import ans_table, range_table

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
t_end = time.time() + budget
n_cases = 0
while time.time() < t_end:
    coder, family = str(rng.choice(["ans", "range"])), str(rng.choice(["gaussian", "laplace", "cauchy"]))
    cfg = [(32, 64, 24), (32, 64, 12), (16, 32, 12)][int(rng.integers(0, 3))]
    W, S, P = cfg
    lo, hi = (-100, 100) if P == 24 else (-60, 60)
    every = int(rng.choice([16, 32, 48, 256]))
    n_streams = int(rng.choice([1, 5, 31, 33, 64, 65, 130]))
    lengths = rng.choice([0, 1, every - 1, every, every + 1, 2 * every, 3 * every + 5] + rng.integers(0, 400, 8).tolist(), n_streams)
    syms, locs, scales = [], [], []
    for n in lengths:
        a, b = rng.uniform(lo * 0.6, hi * 0.6, n), np.exp(rng.uniform(np.log(1e-3 if rng.random() < 0.2 else 0.3), np.log(40.0), n))
        noise = rng.standard_normal(n) if family == "gaussian" else rng.laplace(0, 1, n) if family == "laplace" else rng.standard_cauchy(n)
        syms.append(np.clip(np.rint(a + b * noise), lo, hi).astype(np.int32)); locs.append(a); scales.append(b)
    flat, offsets = B.ragged(syms)
    a_d, b_d = dev(np.concatenate(locs)), dev(np.concatenate(scales))
    order = None if rng.random() < 0.5 else "sorted"
    tag = f"{coder} x {family} {cfg} every={every} streams={n_streams} order={order}"
    encode, decode = getattr(B, f"{coder}_encode_{family}_ragged"), getattr(B, f"{coder}_decode_{family}_ragged")
    enc = encode(flat, offsets, lo, hi, a_d, b_d, cfg, order=order, jump_every=every)
    plain = encode(flat, offsets, lo, hi, a_d, b_d, cfg, order=order)
    dec, st = decode(enc, offsets, lo, hi, a_d, b_d)
    torch.cuda.synchronize()
    assert B.last_kernel() == f"{coder}_decode_{family}_ragged_kernel<jump>", tag
    assert int(enc.status.abs().sum()) == 0 and int(st.abs().sum()) == 0 and torch.equal(dec, flat), tag
    assert torch.equal(enc.n_words, plain.n_words) and plain.jump is None, tag
    words, woff, nw = enc.words.cpu().numpy().view(np.uint32), enc.word_offsets.cpu().numpy(), enc.n_words.cpu().numpy()
    pwords = plain.words.cpu().numpy().view(np.uint32)
    coff, pos = enc.jump.chunk_offsets.cpu().numpy(), enc.jump.pos.cpu().numpy().view(np.uint32)
    cols = [pos] + [x.cpu().numpy().view(np.uint64) for x in ([enc.jump.state] if coder == "ans" else [enc.jump.lower, enc.jump.range])]
    for s in range(n_streams):
        if family == "gaussian":
            models = [O.GaussianModel(lo, hi, float(x), float(y), P) for x, y in zip(locs[s], scales[s])]
        else:
            fam = O.FAMILY_LAPLACE if family == "laplace" else O.FAMILY_CAUCHY
            models = [O.TableModel(O.leaky_family_cdf(fam, lo, hi, float(x), float(y), P), lo, P) for x, y in zip(locs[s], scales[s])]
        want, table = (ans_table if coder == "ans" else range_table)(O, cfg, syms[s], models, every)
        assert words[woff[s]: woff[s] + nw[s]].tolist() == want.tolist() == pwords[woff[s]: woff[s] + nw[s]].tolist(), (tag, s, "words")
        assert [tuple(int(c[k]) for c in cols) for k in range(coff[s], coff[s + 1])] == table, (tag, s, "table")
    n_cases += 1
print(f"{n_cases} random ragged per-symbol batches with jump points agree with the oracle")
