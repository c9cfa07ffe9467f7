"""The expected jump table of one stream of a ragged per-symbol batch, from the CPU oracle alone (no GPU result enters): what the
reference's Pos / Seek give when a stream is coded chunk by chunk.  Shared by tests/test_persymbol_ragged_jump_cpu.py, which checks
the recipe itself, and tests/test_gpu_persymbol_ragged_jump.py, which compares the device's tables with it."""
import numpy as np


def ans_table(O, cfg, sym, models, every):
    """(words, [(pos, state) per chunk]): AnsCoder.encode_reverse per chunk, LAST chunk first (a stack), pos() after each --
    AnsCoder::pos() in front of chunk j is taken once the symbols from j * every on are encoded"""
    W, S, P = cfg
    n = len(sym)
    if n == 0:
        return np.zeros(0, np.uint32), []
    c = O.AnsCoder(W=W, S=S)
    table = [None] * (-(-n // every))
    for j in range(len(table) - 1, -1, -1):
        c.encode_reverse(sym[j * every: (j + 1) * every], models[j * every: (j + 1) * every], P)
        pos, state = c.pos()
        table[j] = (int(pos), int(state))
    return np.asarray(c.get_compressed()), table


def range_table(O, cfg, sym, models, every):
    """(words, [(pos, lower, range) per chunk]): RangeEncoder.pos() BEFORE each encode(chunk), first chunk first (a queue)"""
    W, S, P = cfg
    n = len(sym)
    c = O.RangeEncoder(W=W, S=S)
    table = []
    for j in range(-(-n // every)):
        pos, (lower, rng) = c.pos()
        table.append((int(pos), int(lower), int(rng)))
        c.encode(sym[j * every: (j + 1) * every], models[j * every: (j + 1) * every], P)
    return np.asarray(c.get_compressed()), table
