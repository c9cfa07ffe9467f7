"""CPU-only: every entry point of the per-symbol coders (csrc/cst_persymbol*.hip) judges its arguments before it touches the device,
and the answers are part of the interface: which code, and which of two failing checks speaks first.  Every call here has HOST
buffers behind its pointers and is one that returns before the device is touched -- a refusal, or a batch of no streams.

EXPECTED was recorded from the library as it was before the per-symbol source file was split (one row per entry point, one
entry per case of `_cases`, in order); the table is data, not derived from the code under test."""
import ctypes

import numpy as np
import pytest

from constriction_amd import _native as N

OK, BAD, MODEL = N.CST_OK, N.CST_ERR_INVALID_ARGUMENT, N.CST_ERR_MODEL

# One (name, kind) per parameter, in the order of include/constriction_amd.h.  Kinds:
#   cfg   the coder config, and its unsupported values      cfgw  ... where only the word size is looked at before the device
#   lo hi the support of a quantised family                 fam   the family id
#   P     a pointer the call requires                       o     a pointer or number it does not judge before the device
#   S     the raw state (required with CST_FLAG_RAW_STATE)  fl    the flags
#   ns np n_streams, n_per_stream                           lay   the layout
#   K     n_symbols of explicit rows (up to 2^P)            Kf Kp n_symbols of Categorical (fast: below 2^P - 1; perfect: 1024 and 2^P)
#   pb    prob_bytes                                        ci    the jump-point interval
_ENC_TAIL = "words:P stride:o n_words:P state:S status:P flags:fl stream:o"
_GAUSS = "cfg:cfg lo:lo hi:hi "
_CHAIN_TAIL = "push_words:P push_stride:o n_push:P heads:P status:P stream:o"
_RAGGED_ENC = "symbols:P a:P b:P sym_offsets:P ns:ns order:o words:P word_offsets:o stride:o n_words:P status:P stream:o"
_RAGGED_DEC = "words:P word_offsets:o stride:o cap:o n_words:P a:P b:P symbols:P sym_offsets:P ns:ns order:o status:P stream:o"
_CAT_ENC = "cfg:cfg symbols:P probs:P pb:pb K:%s ns:ns np:np lay:lay " + _ENC_TAIL
_CAT_DEC = "cfg:cfg words:P offsets:o stride:o cap:o n_words:P probs:P pb:pb K:%s symbols:P ns:ns np:np lay:lay state:S %sstatus:P flags:fl stream:o"
SPECS = {
    "cst_ans_encode_cp_batch": "cfg:cfg left:P prob:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_range_encode_cp_batch": "cfg:cfg left:P prob:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_ans_encode_gaussian_batch": _GAUSS + "symbols:P a:P b:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_range_encode_gaussian_batch": _GAUSS + "symbols:P a:P b:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_ans_decode_gaussian_batch": _GAUSS + "words:o offsets:o stride:o cap:o n_words:P a:P b:P symbols:P ns:ns np:np lay:lay state:S "
                                              "n_words_out:o status:P flags:fl stream:o",
    "cst_range_decode_gaussian_batch": _GAUSS + "words:o offsets:o stride:o cap:o n_words:P a:P b:P symbols:P ns:ns np:np lay:lay state:S "
                                                "status:P flags:fl stream:o",
    "cst_ans_decode_rows_batch": "cfg:cfg words:o offsets:o stride:o cap:o n_words:P rows:P K:K min:o symbols:P ns:ns np:np lay:lay state:S "
                                 "n_words_out:o status:P flags:fl stream:o",
    "cst_range_decode_rows_batch": "cfg:cfg words:o offsets:o stride:o cap:o n_words:P rows:P K:K min:o symbols:P ns:ns np:np lay:lay state:S "
                                   "status:P flags:fl stream:o",
    "cst_chain_encode_cp_batch": "cfg:cfg left:P prob:P ns:ns np:np lay:lay pop_words:P pop_offsets:o pop_stride:o n_pop:P " + _CHAIN_TAIL,
    "cst_chain_encode_gaussian_batch": _GAUSS + "symbols:P a:P b:P ns:ns np:np lay:lay pop_words:P pop_offsets:o pop_stride:o n_pop:P " + _CHAIN_TAIL,
    "cst_chain_decode_gaussian_batch": _GAUSS + "pop_words:P pop_offsets:o pop_stride:o n_pop:P a:P b:P symbols:P ns:ns np:np lay:lay " + _CHAIN_TAIL,
    "cst_chain_decode_rows_batch": "cfg:cfg pop_words:P pop_offsets:o pop_stride:o n_pop:P rows:P row_stride:rs K:K min:o symbols:P ns:ns np:np lay:lay "
                                   + _CHAIN_TAIL,
    "cst_ans_encode_gaussian_batch_ckpt": _GAUSS + "symbols:P a:P b:P ns:ns np:np lay:lay words:P stride:o n_words:P ci:ci ckpt_pos:P ckpt_state:P "
                                                   "status:P stream:o",
    "cst_range_encode_gaussian_batch_ckpt": _GAUSS + "symbols:P a:P b:P ns:ns np:np lay:lay words:P stride:o n_words:P ci:ci ckpt_pos:P ckpt_lower:P "
                                                     "ckpt_range:P status:P stream:o",
    # (the jump-point decoders launch their first kernel before the rest is judged: only what comes before it is asked here)
    "cst_ans_decode_gaussian_batch_ckpt": "cfg:o lo:o hi:o words:o offsets:o stride:o cap:o ci:cid ckpt_pos:P ckpt_state:P a:o b:o symbols:o ns:ns np:np "
                                          "scratch:P status:P stream:o",
    "cst_range_decode_gaussian_batch_ckpt": "cfg:cfgw lo:o hi:o words:P offsets:o stride:o cap:o n_words:P ci:cid ckpt_pos:P ckpt_lower:P ckpt_range:P "
                                            "a:o b:o symbols:o ns:ns np:np scratch:P status:P stream:o",
    "cst_ans_encode_gaussian_ragged": _GAUSS + _RAGGED_ENC,
    "cst_range_encode_gaussian_ragged": _GAUSS + _RAGGED_ENC,
    "cst_ans_decode_gaussian_ragged": _GAUSS + _RAGGED_DEC,
    "cst_range_decode_gaussian_ragged": _GAUSS + _RAGGED_DEC,
    "cst_ans_encode_family_ragged": "cfg:cfg fam:fam lo:lo hi:hi " + _RAGGED_ENC,
    "cst_range_encode_family_ragged": "cfg:cfg fam:fam lo:lo hi:hi " + _RAGGED_ENC,
    "cst_ans_decode_family_ragged": "cfg:cfg fam:fam lo:lo hi:hi " + _RAGGED_DEC,
    "cst_range_decode_family_ragged": "cfg:cfg fam:fam lo:lo hi:hi " + _RAGGED_DEC,
    "cst_ans_encode_family_batch": "cfg:cfg fam:fam lo:lo hi:hi symbols:P a:P b:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_range_encode_family_batch": "cfg:cfg fam:fam lo:lo hi:hi symbols:P a:P b:P ns:ns np:np lay:lay " + _ENC_TAIL,
    "cst_ans_decode_family_batch": "cfg:cfg fam:fam lo:lo hi:hi words:P offsets:o stride:o cap:o n_words:P a:P b:P symbols:P ns:ns np:np lay:lay "
                                   "state:S n_words_out:o status:P flags:fl stream:o",
    "cst_range_decode_family_batch": "cfg:cfg fam:fam lo:lo hi:hi words:P offsets:o stride:o cap:o n_words:P a:P b:P symbols:P ns:ns np:np lay:lay "
                                     "state:S status:P flags:fl stream:o",
    "cst_ans_encode_categorical_batch": _CAT_ENC % "Kf",
    "cst_range_encode_categorical_batch": _CAT_ENC % "Kf",
    "cst_ans_decode_categorical_batch": _CAT_DEC % ("Kf", "n_words_out:o "),
    "cst_range_decode_categorical_batch": _CAT_DEC % ("Kf", ""),
    "cst_ans_encode_categorical_perfect_batch": _CAT_ENC % "Kp",
    "cst_range_encode_categorical_perfect_batch": _CAT_ENC % "Kp",
    "cst_ans_decode_categorical_perfect_batch": _CAT_DEC % ("Kp", "n_words_out:o "),
    "cst_range_decode_categorical_perfect_batch": _CAT_DEC % ("Kp", ""),
    "cst_categorical_fast_cdf_rows": "precision:prec probs:P pb:pb ns:ns K:Kr rows:P bad:o stream:o",
    "cst_categorical_fast_cdf_host": "precision:prec probs:P pb:pb ns:ns K:Kr rows:P bad:o",
}

_DEFAULTS = {"lo": -100, "hi": 100, "fam": N.FAMILY_LAPLACE, "ns": 1, "np": 32, "lay": N.LAYOUT_STREAM_MAJOR, "fl": N.FLAG_NONE, "K": 8, "Kf": 8,
             "Kp": 8, "Kr": 8, "pb": 4, "ci": 16, "cid": 16, "rs": 0, "prec": 12}
_NUMBERS = {"stride": 64, "cap": 64, "pop_stride": 64, "push_stride": 64, "min": 0, "lo": -100, "hi": 100}
_OPTIONAL_BUFFERS = ("words", "a", "b", "symbols", "status", "n_words", "n_words_out", "bad")     # kind o, but pointers a valid call gives
_NULL = ("offsets", "word_offsets", "pop_offsets", "order", "stream")                                # ... and pointers it may leave out
_BUFFER = object()
_P8 = (32, 64, 8)


def _spec(name):
    return [tuple(item.split(":")) for item in SPECS[name].split()]


def _cases(name):
    """(label, {parameter: value}) for every case of one entry point, in a fixed order"""
    spec = _spec(name)
    kinds = {kind for _, kind in spec}
    kind_of = dict(spec)
    required = [p for p, kind in spec if kind == "P"]
    out = [("null " + p, {p: None}) for p in required]
    if "hi" in kinds:
        out += [("max == min", {"hi": -100}), ("max < min", {"hi": -101})]
        out += [("max == min, null " + p, {"hi": -100, p: None}) for p in required]
        out += [("support 2^P + 1", {"cfg": _P8, "lo": 0, "hi": 256}), ("support 2^P + 1, null " + required[0], {"cfg": _P8, "lo": 0, "hi": 256, required[0]: None})]
    if "fam" in kinds:
        out += [("family 0", {"fam": 0}), ("family binomial", {"fam": N.FAMILY_BINOMIAL}), ("family binomial, max == min", {"fam": N.FAMILY_BINOMIAL, "hi": -100})]
    if "K" in kinds:
        out += [("n_symbols 1", {"K": 1}), ("n_symbols 2^P + 1", {"cfg": _P8, "K": 257}), ("n_symbols 1, null " + required[0], {"K": 1, required[0]: None})]
    if "Kf" in kinds:
        out += [("n_symbols 1", {"K": 1}), ("n_symbols 2^P - 1", {"cfg": _P8, "K": 255}), ("n_symbols 2^P", {"cfg": _P8, "K": 256}),
                ("n_symbols 1, null " + required[0], {"K": 1, required[0]: None}), ("n_symbols 1, layout 7", {"K": 1, "lay": 7})]
    if "Kp" in kinds:
        out += [("n_symbols 1", {"K": 1}), ("n_symbols 1025", {"K": N.CATEGORICAL_PERFECT_MAX_K + 1}), ("n_symbols 2^P + 1", {"cfg": _P8, "K": 257}),
                ("n_symbols 1, null " + required[0], {"K": 1, required[0]: None}), ("n_symbols 1, layout 7", {"K": 1, "lay": 7})]
    if "Kr" in kinds:
        out += [("n_symbols 1", {"K": 1}), ("n_symbols 2^P - 1", {"precision": 8, "K": 255}), ("n_symbols 1, null " + required[0], {"K": 1, required[0]: None})]
    if "prec" in kinds:
        out += [("precision 0", {"precision": 0}), ("precision 32", {"precision": 32})]
    if "lay" in kinds:
        out += [("layout 7", {"lay": 7}), ("layout 7, null " + required[0], {"lay": 7, required[0]: None})]
    if "cfg" in kinds:
        out += [("config 32/64/25", {"cfg": (32, 64, 25)}), ("config 16/32/17", {"cfg": (16, 32, 17)}), ("config 8/16/4", {"cfg": (8, 16, 4)}),
                ("config 32/32/8", {"cfg": (32, 32, 8)}), ("config 8/16/4, null " + required[0], {"cfg": (8, 16, 4), required[0]: None})]
    if "cfgw" in kinds:
        out += [("config 8/16/4", {"cfg": (8, 16, 4)})]
    if "S" in kinds:
        out += [("raw state, null state", {"flags": N.FLAG_RAW_STATE, "state": None})]
        if "hi" in kinds:
            out += [("raw state, null state, max == min", {"flags": N.FLAG_RAW_STATE, "state": None, "hi": -100})]
    if "pb" in kinds:
        out += [("prob_bytes 2", {"pb": 2}), ("prob_bytes 2, null " + required[0], {"pb": 2, required[0]: None})]
    if "ci" in kinds or "cid" in kinds:
        out += [("interval 0", {"ci": 0}), ("interval 48 of 32", {"ci": 48})]
    if "ci" in kinds:
        out += [("interval 24", {"ci": 24, "np": 48}), ("interval 0, max == min", {"ci": 0, "hi": -100})]
    if "rs" in kinds:
        out += [("row_stride 5 for 8 symbols", {"row_stride": 5})]
    if name.endswith("_ragged"):
        out += [("no word_offsets, stride 0", {"stride": 0}), ("order, 2^32 + 1 streams", {"order": _BUFFER, "ns": (1 << 32) + 1})]
    if name == "cst_range_decode_gaussian_batch_ckpt":
        out += [("2^31 virtual streams", {"ns": 1 << 31, "np": 16})]
    out += [("no streams", {"ns": 0})]
    assert all(k in kind_of for _, o in out for k in o), name
    return out


def _call(lib, name, overrides):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = N.SIGNATURES[name]
    keep, args = [], []
    for p, kind in _spec(name):
        v = overrides.get(p, _BUFFER if kind in ("P", "S") or p in _OPTIONAL_BUFFERS else None)
        if v is _BUFFER:
            buf = np.zeros(512, dtype=np.uint64)
            keep.append(buf)
            v = ctypes.c_void_p(buf.ctypes.data)
        elif p in overrides or p in _NULL:
            pass
        elif p == "cfg":
            v = (32, 64, 24)
        else:
            v = _NUMBERS[p] if p in _NUMBERS else _DEFAULTS[kind]
        if p == "cfg":
            v = N.CoderConfig(*v)
        args.append(v)
    return int(fn(*args))


@pytest.fixture(scope="module")
def lib():
    from constriction_amd import build
    build.build_library()
    return N.load_library()


EXPECTED = {
    "cst_ans_encode_cp_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_encode_cp_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_encode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD,
        BAD, MODEL, OK],
    "cst_range_encode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD,
        BAD, MODEL, OK],
    "cst_ans_decode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL,
        OK],
    "cst_range_decode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL,
        OK],
    "cst_ans_decode_rows_batch": [
        BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_decode_rows_batch": [
        BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_chain_encode_cp_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_chain_encode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, BAD, BAD,
        BAD, BAD, BAD, MODEL, BAD, BAD, OK],
    "cst_chain_decode_gaussian_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL, MODEL,
        MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_chain_decode_rows_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_encode_gaussian_batch_ckpt": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD,
        MODEL, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_encode_gaussian_batch_ckpt": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, MODEL, MODEL, BAD, BAD, BAD,
        BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_decode_gaussian_batch_ckpt": [
        BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_decode_gaussian_batch_ckpt": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_encode_gaussian_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_encode_gaussian_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_decode_gaussian_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_decode_gaussian_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_encode_family_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_range_encode_family_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_ans_decode_family_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_range_decode_family_ragged": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_ans_encode_family_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_range_encode_family_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_ans_decode_family_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_range_decode_family_batch": [
        BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
        BAD, BAD, OK],
    "cst_ans_encode_categorical_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_encode_categorical_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_decode_categorical_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_decode_categorical_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_encode_categorical_perfect_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_encode_categorical_perfect_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_ans_decode_categorical_perfect_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_range_decode_categorical_perfect_batch": [
        BAD, BAD, BAD, BAD, BAD, MODEL, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_categorical_fast_cdf_rows": [
        BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, OK],
    "cst_categorical_fast_cdf_host": [
        BAD, BAD, MODEL, MODEL, BAD, BAD, BAD, BAD, BAD, OK],
}


def test_the_table_covers_every_entry_point_and_case():
    assert sorted(EXPECTED) == sorted(SPECS)
    for name in SPECS:
        assert len(EXPECTED[name]) == len(_cases(name)), name
        # nothing in the table is a call that reached the device, and every call but "no streams" is a refusal
        assert set(EXPECTED[name][:-1]) <= {BAD, MODEL} and EXPECTED[name][-1] == OK, name


@pytest.mark.parametrize("name", sorted(SPECS))
def test_arguments_are_judged_as_before(lib, name):
    got = [_call(lib, name, overrides) for _, overrides in _cases(name)]
    wrong = [(label, g, e) for (label, _), g, e in zip(_cases(name), got, EXPECTED[name]) if g != e]
    assert not wrong, f"{name}: (case, returned, expected) {wrong}"


def test_range_ckpt_scratch_bytes(lib):
    fn = lib.cst_range_gaussian_ckpt_scratch_bytes
    fn.restype, fn.argtypes = N.SIGNATURES["cst_range_gaussian_ckpt_scratch_bytes"]
    assert fn(3, 64, 0) == 0
    # (sizeof(cst_range_state) + 16) bytes per (stream, chunk), chunks rounded up, and 64 for alignment
    assert fn(3, 64, 16) == (40 + 16) * 3 * 4 + 64 and fn(3, 65, 16) == (40 + 16) * 3 * 5 + 64
