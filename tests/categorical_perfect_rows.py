"""Shared by tests/test_categorical_perfect_cpu.py and tests/test_gpu_categorical_perfect.py: the seeded probability rows both
files run through `perfectly_quantized_probabilities`, the host restatements they compare with, and a line-by-line Python
restatement of the reference's formulation (a vector of slots that is stable-sorted and scanned) that counts the unit moves."""
import ctypes

import numpy as np

KINDS = ("uniform", "lognormal6", "all_equal", "half_zero", "repeated", "softmax_tail")
# (K, n_rows, P, dtype): every K of {2, 3, 63, 64, 65, 128, 257, 1024} (the lane boundary, more than one slot per lane, the
# maximum), every n_rows of {1, 63, 65, 1000}, P = 24 and 12, and P = 12 with K = 1000 (nearly every weight is 1: loss = inf)
ROW_CASES = [(2, 1000, 24, "f64"), (2, 65, 12, "f32"), (3, 65, 24, "f32"), (63, 63, 24, "f64"), (64, 65, 12, "f32"), (64, 63, 24, "f64"),
             (65, 63, 24, "f32"), (128, 65, 12, "f64"), (128, 1, 24, "f32"), (257, 63, 24, "f32"), (257, 65, 12, "f64"), (1024, 63, 24, "f32"),
             (1024, 1, 12, "f64"), (1000, 65, 12, "f64"), (1000, 63, 12, "f32")]
DTYPES = {"f32": np.float32, "f64": np.float64}


def case_id(case):
    return "K%d_n%d_P%d_%s" % case


def move_cap(k):
    """the kernel's safety stop (perfect_move_cap of csrc/cst_categorical_perfect.hip)"""
    return 16 * k + 1024


def make_rows(n_rows, k, dtype, seed):
    """[n_rows, k] in `dtype`: row r is of kind KINDS[r % 6]
         uniform       uniform random entries
         lognormal6    exp(N(0, 6^2)): entries over many orders of magnitude
         all_equal     one value k times: every tie rule decides
         half_zero     uniform entries, half of them exactly 0
         repeated      three values, each many times
         softmax_tail  exp(-x), x spread over [0, 100] in random order: in f32 the tail is subnormal (from e^-87.4 on) and, at
                       the very end, a few exact zeros"""
    rng = np.random.default_rng(seed)
    out = np.empty((n_rows, k), dtype=np.float64)
    for r in range(n_rows):
        kind = KINDS[r % len(KINDS)]
        if kind == "uniform":
            row = rng.random(k)
        elif kind == "lognormal6":
            row = np.exp(rng.normal(0.0, 6.0, k))
        elif kind == "all_equal":
            row = np.full(k, (1.0, 0.1, 3.0, 1e-3)[(r // len(KINDS)) % 4])
        elif kind == "half_zero":
            row = rng.random(k) + 1e-3
            row[rng.permutation(k)[: k // 2]] = 0.0
        elif kind == "repeated":
            row = rng.choice(np.array([0.5, 0.25, 1e-4]), size=k)
        else:
            row = np.exp(-rng.permutation(np.linspace(0.0, 100.0, k)))
        out[r] = row
    return np.ascontiguousarray(out.astype(dtype))


def case_rows(case):
    k, n_rows, P, dtype = case
    return make_rows(n_rows, k, DTYPES[dtype], 7919 * k + 31 * n_rows + P)


def host_perfect(lib, probs, P):
    """cst_categorical_perfect_cdf_host: (rows [n, K + 1], codes [n], moves [n])"""
    probs = np.ascontiguousarray(probs)
    n, k = probs.shape
    rows, bad, moves = np.zeros((n, k + 1), np.uint32), np.full(n, -1, np.int32), np.full(n, 0xFFFFFFFF, np.uint32)
    rc = lib.cst_categorical_perfect_cdf_host(P, ctypes.c_void_p(probs.ctypes.data), probs.itemsize, n, k, ctypes.c_void_p(rows.ctypes.data),
                                              ctypes.c_void_p(bad.ctypes.data), ctypes.c_void_p(moves.ctypes.data))
    assert rc == 0
    return rows, bad, moves


def sorted_vector_perfect(lib, row, P):
    """cst_categorical_perfect_cdf (the reference's formulation in the library's host code): (rc, cdf)"""
    p = np.ascontiguousarray(row, dtype=np.float64)              # F: Into<f64>
    cdf = np.zeros(len(p) + 1, dtype=np.uint32)
    rc = lib.cst_categorical_perfect_cdf(ctypes.c_void_p(p.ctypes.data), len(p), P, ctypes.c_void_p(cdf.ctypes.data))
    return rc, cdf


def python_perfect(lib, row, P):
    """categorical.rs:56-177 line by line over the library's host log1p (musl's, as the reference's libm crate): a list of slots,
    `sort_by` (stable) on win descending, max_by / min_by scans that keep the last maximum and the first minimum.  Returns
    (cdf, moves), or (None, 0) where the reference returns Err."""
    log1p = lib.cst_debug_host_log1p
    probs = [float(x) for x in np.asarray(row, dtype=np.float64)]
    k, total, inf = len(probs), 1 << P, float("inf")
    norm = 0.0
    for p in probs:
        norm += p
    if not (np.isfinite(norm) and norm >= np.finfo(np.float64).tiny):
        return None, 0
    left = total - k
    scale = np.float64(left) / np.float64(norm)

    def gain(p, w):
        return p * log1p(1.0 / w)

    def cost(p, w):
        return inf if w == 1 else -p * log1p(-1.0 / w)

    slots = []
    for i, p in enumerate(probs):
        if p < 0.0:
            return None, 0
        share = float(np.float64(p) * scale)
        extra = 0 if not share > 0.0 else min(int(share), 0xFFFFFFFF)
        if extra > left:
            return None, 0
        left -= extra
        slots.append({"i": i, "p": p, "w": extra + 1, "win": gain(p, extra + 1), "loss": cost(p, extra + 1)})
    while left:
        slots.sort(key=lambda s: -s["win"])                      # (stable; -0.0 and 0.0 compare equal)
        batch = min(left, k)
        for s in slots[:batch]:
            s["w"] += 1
            s["win"], s["loss"] = gain(s["p"], s["w"]), cost(s["p"], s["w"])
        left -= batch
    moves = 0
    while True:
        buyer, seller = slots[0], slots[0]
        for s in slots[1:]:
            if not s["win"] < buyer["win"]:
                buyer = s
            if s["loss"] < seller["loss"]:
                seller = s
        if buyer is seller or buyer["win"] <= seller["loss"]:
            break
        seller["w"] -= 1
        seller["win"], seller["loss"] = -inf, cost(seller["p"], seller["w"])
        buyer["w"] += 1
        buyer["loss"], buyer["win"] = inf, gain(buyer["p"], buyer["w"])
        moves += 1
    weights = np.zeros(k, dtype=np.uint64)
    for s in slots:
        weights[s["i"]] = s["w"]
    return np.concatenate([[0], np.cumsum(weights)]).astype(np.uint32), moves
