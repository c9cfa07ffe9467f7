"""Batched, device-resident front end: thousands of independent coders per call.

This is the extension the reference has no counterpart for (it codes one stream per `AnsCoder`
object, src/stream/stack.rs); every stream's compressed words are bit-identical to what one
reference coder would produce for that stream alone.  PyTorch is used for device memory and
streams only; all computation happens in the HIP library behind include/constriction_amd.h.
"""
from __future__ import annotations

import ctypes as C
import inspect
import json
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N

PRESETS = {"default": (32, 64, 24), "lookup": (32, 64, 12), "small": (16, 32, 12)}


_SYMBOL_BYTES = {torch.int8: 1, torch.int16: 2, torch.int32: 4}


def _cfg(W, S, P):
    return N.CoderConfig(W, S, P)


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _require_cuda(t: torch.Tensor, dtype, name):
    if not t.is_cuda:
        raise ValueError(f"{name} must live in device memory (HBM)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}")
    return t.contiguous()


class Model:
    """Device image of an entropy model with contiguous support (include/constriction_amd.h, cst_model)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.load_library().cst_model_destroy(h)
            except Exception:
                pass

    @classmethod
    def from_cdf(cls, cdf, min_symbol: int, precision: int) -> "Model":
        """Any tabulated model: cdf[n+1] with cdf[0]=0 < ... < cdf[n]=2^P."""
        cdf = np.ascontiguousarray(cdf, dtype=np.uint32)
        h = C.c_void_p()
        N.check(N.lib().cst_model_create_table(precision, int(min_symbol), len(cdf) - 1, cdf.ctypes.data, C.byref(h)),
                "cst_model_create_table")
        return cls(h)

    @classmethod
    def from_cdf_noncontiguous(cls, symbols, cdf, precision: int) -> "Model":
        """A tabulated model over arbitrary distinct int32 symbols (symbols[i] has left cumulative cdf[i]):
        NonContiguousCategorical{Encoder,Decoder}Model / NonContiguousLookupDecoderModel of the reference."""
        cdf = np.ascontiguousarray(cdf, dtype=np.uint32)
        symbols = np.ascontiguousarray(symbols, dtype=np.int32)
        if len(symbols) != len(cdf) - 1:
            raise ValueError("one symbol per table entry")
        h = C.c_void_p()
        N.check(N.lib().cst_model_create_table_noncontiguous(precision, len(symbols), symbols.ctypes.data, cdf.ctypes.data, C.byref(h)),
                "cst_model_create_table_noncontiguous")
        m = cls(h)
        m.noncontiguous = True
        return m

    def symbols_to_indices(self, symbols: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        symbols = _require_cuda(symbols, torch.int32, "symbols")
        out = torch.empty_like(symbols) if out is None else out
        N.check(N.lib().cst_symbols_to_indices(self._h, _ptr(symbols), symbols.numel(), _ptr(out), _stream_ptr()), "cst_symbols_to_indices")
        return out

    def indices_to_symbols(self, indices: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = torch.empty_like(indices) if out is None else out
        N.check(N.lib().cst_indices_to_symbols(self._h, _ptr(indices), indices.numel(), _ptr(out), _stream_ptr()), "cst_indices_to_symbols")
        return out

    noncontiguous = False
    per_stream = False            # True: table s belongs to stream s (the *_per_stream constructors), whatever the number of tables

    @classmethod
    def quantized_gaussian(cls, min_symbol: int, max_symbol: int, mean: float, std: float, precision: int) -> "Model":
        """LeakyQuantizer(min..=max) x Gaussian(mean, std), tabulated on the GPU in bit-exact f64."""
        h = C.c_void_p()
        N.check(N.lib().cst_model_create_gaussian(precision, int(min_symbol), int(max_symbol), float(mean), float(std),
                                                  _stream_ptr(), C.byref(h)), "cst_model_create_gaussian")
        return cls(h)

    @classmethod
    def quantized_gaussian_per_stream(cls, min_symbol, max_symbol, means: torch.Tensor, stds: torch.Tensor,
                                      precision: int) -> "Model":
        means = _require_cuda(means, torch.float64, "means")
        stds = _require_cuda(stds, torch.float64, "stds")
        if means.shape != stds.shape or means.dim() != 1:
            raise ValueError("means and stds must be 1-d and of equal length (one entry per stream)")
        h = C.c_void_p()
        N.check(N.lib().cst_model_create_gaussian_per_stream(precision, int(min_symbol), int(max_symbol), _ptr(means),
                                                             _ptr(stds), means.numel(), _stream_ptr(), C.byref(h)),
                "cst_model_create_gaussian_per_stream")
        m = cls(h)
        m.per_stream = True
        return m

    @classmethod
    def from_cdf_rows_per_stream(cls, rows, min_symbol: int, precision: int) -> "Model":
        """One table per stream from cdf rows [n_streams, n + 1] (a device tensor, int32-typed like cdfs_device() gives them, or a
        numpy array): the inverse of cdfs_device() -- a decoder rebuilds the encoder's per-stream model from the rows alone.  Every
        row is validated on the device (cdf[0] = 0 < ... < cdf[n] = 2^P); a bad row raises ValueError."""
        if isinstance(rows, np.ndarray):
            if rows.ndim != 2 or rows.dtype.kind not in "iu":
                raise ValueError("rows must be a 2-d integer array [n_streams, n_symbols + 1]")
            host = np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32)
            _fit_rows_shape(host.shape, precision)
            rows = torch.from_numpy(host).to(torch.device("cuda", torch.cuda.current_device()))
        elif not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.int32:
            raise ValueError("rows must be a 2-d torch.int32 tensor (or numpy array) [n_streams, n_symbols + 1]")
        _fit_rows_shape(tuple(rows.shape), precision)
        if not rows.is_cuda:
            raise ValueError("rows must live in device memory (HBM)")
        rows = rows.contiguous()
        h = C.c_void_p()
        N.check(N.lib().cst_model_create_tables_per_stream(int(precision), int(min_symbol), rows.shape[1] - 1, _ptr(rows), rows.shape[0],
                                                           _stream_ptr(), C.byref(h)), "cst_model_create_tables_per_stream")
        m = cls(h)
        m.per_stream = True
        return m

    @classmethod
    def fit(cls, symbols, min_symbol: int, max_symbol: int, precision: int, perfect: bool = False) -> "Model":
        """One shared table fitted to `symbols` (any shape) on the device: count, quantise like Categorical(counts, perfect=...),
        build.  ValueError if a symbol lies outside [min_symbol, max_symbol]: such a model could not encode its own data."""
        _fit_precision(precision, 24)
        counts, outside = count_symbols(symbols.reshape(-1) if isinstance(symbols, torch.Tensor) else symbols, min_symbol, max_symbol)
        _fit_refuse_outside(outside)
        rows = fit_cdf_rows(counts, precision, perfect)
        return cls.from_cdf(rows[0].cpu().numpy().view(np.uint32), min_symbol, precision)

    @classmethod
    def fit_per_stream(cls, symbols, min_symbol: int, max_symbol: int, precision: int, perfect: bool = False,
                       sym_offsets: Optional[torch.Tensor] = None) -> "Model":
        """One table per stream, each fitted to its own stream on the device: `symbols` [n_streams, n_per_stream], or flat with
        `sym_offsets` [n_streams + 1] (ragged).  An empty stream gets the uniform table.  ValueError as for fit()."""
        _fit_precision(precision, 16)
        counts, outside = count_symbols(symbols, min_symbol, max_symbol, per_stream=True, sym_offsets=sym_offsets)
        _fit_refuse_outside(outside)
        return cls.from_cdf_rows_per_stream(fit_cdf_rows(counts, precision, perfect), min_symbol, precision)

    @property
    def precision(self):
        return N.load_library().cst_model_precision(self._h)

    @property
    def min_symbol(self):
        return N.load_library().cst_model_min_symbol(self._h)

    @property
    def n_symbols(self):
        return N.load_library().cst_model_n_symbols(self._h)

    @property
    def n_tables(self):
        return N.load_library().cst_model_n_tables(self._h)

    def cdfs_device(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """The cdfs of tables [first, first + count) as an int32-typed tensor [count, n_symbols + 1] in HBM (values < 2^31
        for every precision <= 24 ... 30), copied on the current stream."""
        count = self.n_tables - first if count is None else count
        out = torch.empty((count, self.n_symbols + 1), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        N.check(N.lib().cst_model_copy_cdfs(self._h, int(first), int(count), _ptr(out), _stream_ptr()), "cst_model_copy_cdfs")
        return out

    def cdf(self, index: int = 0) -> np.ndarray:
        out = np.zeros(self.n_symbols + 1, dtype=np.uint32)
        N.check(N.lib().cst_model_get_cdf(self._h, index, out.ctypes.data, _stream_ptr()), "cst_model_get_cdf")
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Fitting table models on the device (csrc/cst_fit.hip): count -> quantise -> model, nothing leaves HBM but
# the one row of a shared model and the K rows of a table set
# ---------------------------------------------------------------------------------------------------------------------

def _fit_precision(precision, most):
    if not 1 <= int(precision) <= most:
        raise ValueError(f"precision must be 1 .. {most}")


def _fit_rows_shape(shape, precision):
    _fit_precision(precision, 16)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 3:
        raise ValueError("rows must be 2-d: one row of n_symbols + 1 >= 3 cumulatives per stream")


def _fit_refuse_outside(outside):
    n = int(outside.item())
    if n:
        raise ValueError(f"{n} symbols lie outside the support (or name no table): a model fitted to the rest could not encode them")


def count_symbols(symbols, min_symbol: int, max_symbol: int, *, indices=None, n_tables=None, per_stream: bool = False, sym_offsets=None):
    """Histograms of int32 `symbols` over the support [min_symbol, max_symbol], counted on the device.  Returns (counts, outside):
    `counts` a torch.int32 tensor in HBM, `outside` a 1-element tensor with the number of symbols that fell into no bin.
      default                  one histogram of the whole tensor (any shape): counts [1, n]
      indices=, n_tables=K     symbol i counts into row indices[i] (torch.uint8 or torch.int32, the symbols' shape): counts [K, n];
                               an index outside [0, K) counts as outside.  K <= 256, n <= 65536
      per_stream=True          one histogram per row of `symbols` [n_streams, n_per_stream], or with sym_offsets= [n_streams + 1]
                               (torch.int64) per stream of the flat `symbols`: counts [n_streams, n].  n <= 1024"""
    if not isinstance(symbols, torch.Tensor) or symbols.dtype != torch.int32:
        raise ValueError("symbols must be a torch.int32 tensor")
    n = int(max_symbol) - int(min_symbol) + 1
    if not -2**31 <= int(min_symbol) <= int(max_symbol) < 2**31:
        raise ValueError("the support [min_symbol, max_symbol] must lie inside int32")
    if not 2 <= n <= (1024 if per_stream else 65536):
        raise ValueError(f"the support must hold 2 .. {1024 if per_stream else 65536} symbols")
    if symbols.numel() >= 2**31:
        raise ValueError("fewer than 2^31 symbols per call")
    if per_stream:
        if indices is not None or n_tables is not None:
            raise ValueError("per_stream counts take no indices")
        if sym_offsets is None:
            if symbols.dim() != 2 or symbols.shape[0] < 1:
                raise ValueError("per_stream counts need symbols [n_streams, n_per_stream] or flat symbols with sym_offsets")
            rows = symbols.shape[0]
        else:
            if not isinstance(sym_offsets, torch.Tensor) or sym_offsets.dtype != torch.int64 or sym_offsets.dim() != 1 or sym_offsets.numel() < 2:
                raise ValueError("sym_offsets must be a 1-d torch.int64 tensor of n_streams + 1 entries")
            if symbols.dim() != 1:
                raise ValueError("with sym_offsets the symbols are flat")
            rows = sym_offsets.numel() - 1
    else:
        if sym_offsets is not None:
            raise ValueError("sym_offsets go with per_stream=True")
        if (indices is None) != (n_tables is None):
            raise ValueError("indices and n_tables come together")
        rows = 1 if n_tables is None else int(n_tables)
        if not 1 <= rows <= 256:
            raise ValueError("n_tables must be 1 .. 256")
        if indices is not None:
            if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.uint8, torch.int32):
                raise ValueError("indices must be a torch.uint8 or torch.int32 tensor")
            if tuple(indices.shape) != tuple(symbols.shape):
                raise ValueError("indices must have the shape of the symbols")
    if not symbols.is_cuda:
        raise ValueError("symbols must live in device memory (HBM)")
    for name, t in (("indices", indices), ("sym_offsets", sym_offsets)):
        if t is not None and (not t.is_cuda or t.device != symbols.device):
            raise ValueError(f"{name} must live in device memory (HBM), on the device of the symbols")
    symbols = symbols.contiguous()
    counts = torch.empty((rows, n), dtype=torch.int32, device=symbols.device)
    outside = torch.empty(1, dtype=torch.int32, device=symbols.device)
    if per_stream:
        if sym_offsets is not None:
            sym_offsets = sym_offsets.contiguous()
            first, last = int(sym_offsets[0].item()), int(sym_offsets[-1].item())
            if not 0 <= first <= last <= symbols.numel():
                raise ValueError("sym_offsets must ascend within the symbols")
        n_per = 0 if sym_offsets is not None else symbols.shape[1]
        N.check(N.lib().cst_count_symbols_per_stream(_ptr(symbols), _ptr(sym_offsets), rows, n_per, int(min_symbol), n, _ptr(counts),
                                                     _ptr(outside), _stream_ptr()), "cst_count_symbols_per_stream")
    else:
        index_bytes = 0
        if indices is not None:
            indices, index_bytes = indices.contiguous(), (1 if indices.dtype == torch.uint8 else 4)
        N.check(N.lib().cst_count_symbols(_ptr(symbols), symbols.numel(), int(min_symbol), n, _ptr(indices), index_bytes, rows, _ptr(counts),
                                          _ptr(outside), _stream_ptr()), "cst_count_symbols")
    return counts, outside


def fit_cdf_rows(counts, precision: int, perfect: bool = False, return_empty: bool = False):
    """The cdf rows of count rows [n_rows, n] (count_symbols), quantised on the device as Categorical(counts[r], perfect=...) does:
    an int32-typed tensor [n_rows, n + 1] in HBM in the format of categorical_cdf_rows.  A row without any count is quantised as if
    every count were 1 (the reference refuses it; here an empty stream does not void a batch); return_empty=True returns
    (rows, empty) with empty[r] = 1 for such rows."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 2:
        raise ValueError("counts must be a 2-d torch.int32 tensor [n_rows, n_symbols]")
    n_rows, n = counts.shape
    if not 1 <= int(precision) <= 31:
        raise ValueError("precision must be 1 .. 31")
    if perfect:
        if n < 2 or n > min(N.CATEGORICAL_PERFECT_MAX_K, 1 << int(precision)):
            raise ValueError(f"perfect=True needs 2 <= n_symbols <= min({N.CATEGORICAL_PERFECT_MAX_K}, 2**precision)")
    elif n < 2 or n >= (1 << int(precision)) - 1:
        raise ValueError("the fast quantisation needs 2 <= n_symbols < 2**precision - 1")
    if not counts.is_cuda:
        raise ValueError("counts must live in device memory (HBM)")
    counts = counts.contiguous()
    rows = torch.empty((n_rows, n + 1), dtype=torch.int32, device=counts.device)
    empty = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=counts.device)
    if n_rows:
        N.check(N.lib().cst_fit_cdf_rows(int(precision), int(bool(perfect)), _ptr(counts), n_rows, n, _ptr(rows), _ptr(empty), _stream_ptr()),
                "cst_fit_cdf_rows")
    return (rows, empty[:n_rows]) if return_empty else rows


def family_cdf_rows(family: int, min_symbol: int, max_symbol: int, a, b=None, n_per_row=None, precision: int = 24,
                    to_numpy: bool = True):
    """LeakyQuantizer(min..=max) x Laplace / Cauchy / Binomial tabulated on the GPU, one cdf row per parameter pair
    (cst_family_cdf_rows; family = 1 Laplace(mean, scale), 2 Cauchy(loc, scale), 3 Binomial(p) over 0..=max or, with
    `n_per_row`, over 0..=n_per_row[r]).  Returns uint32 rows [n_rows, max - min + 2] (numpy, or a torch.int32 view of
    them in HBM with to_numpy=False); raises ValueError where the reference panics (a probability of zero)."""
    dev = torch.device("cuda", torch.cuda.current_device())

    def dev_f64(x):
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            return _require_cuda(x, torch.float64, "model parameter")
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)

    da, db = dev_f64(a), dev_f64(b)
    dn = None if n_per_row is None else torch.from_numpy(np.ascontiguousarray(n_per_row, dtype=np.int32)).to(dev)
    n_rows = da.numel()
    width = int(max_symbol) - int(min_symbol) + 2
    rows = torch.empty((n_rows, width), dtype=torch.int32, device=dev)
    bad = torch.empty(n_rows, dtype=torch.int32, device=dev)
    N.check(N.lib().cst_family_cdf_rows(int(family), int(precision), int(min_symbol), int(max_symbol), _ptr(da), _ptr(db), _ptr(dn),
                                        n_rows, _ptr(rows), _ptr(bad), _stream_ptr()), "cst_family_cdf_rows")
    if n_rows and bool(bad.any().item()):
        raise ValueError("Invalid model: a symbol of the support gets probability zero under the leaky quantizer "
                         "(quantize.rs:560-566).")
    return rows.cpu().numpy().view(np.uint32) if to_numpy else rows


def _to_indices(model: "Model", symbols: torch.Tensor) -> torch.Tensor:
    """Every table-model entry point codes INDICES into the model's alphabet; for a non-contiguous alphabet
    (Model.from_cdf_noncontiguous) the symbols are translated first (a symbol outside the alphabet becomes index n, which the
    coders report as CST_STREAM_IMPOSSIBLE_SYMBOL), for a contiguous one the kernels subtract min_symbol themselves."""
    return model.symbols_to_indices(symbols) if model.noncontiguous else symbols


def _to_symbols(model: "Model", decoded: torch.Tensor) -> torch.Tensor:
    if model.noncontiguous:
        model.indices_to_symbols(decoded, out=decoded)
    return decoded


@dataclass
class EncodedBatch:
    """Per-stream compressed words in fixed-stride slabs (stream s: words[s, :n_words[s]]).

    jump: the jump points the encode call noted for its own words (Checkpoints / RangeCheckpoints, `jump_points=` of the encode
    calls; None = none) -- side information the matching decode call uses to decode every stream on several lanes.  They describe
    the words the encoder wrote: replacing `words` or `n_words` drops them, and whoever edits those tensors IN PLACE sets
    `jump = None` (the plain decoders read the words alone)."""
    words: torch.Tensor      # uint32 as int32 storage? -> torch.int32 view of uint32 words [n_streams, stride]
    n_words: torch.Tensor    # int32 [n_streams] (values are counts)
    status: torch.Tensor     # int32 [n_streams]
    config: tuple
    jump: Optional[object] = None

    def __setattr__(self, name, value):
        if name in ("words", "n_words") and "jump" in self.__dict__:
            object.__setattr__(self, "jump", None)
        object.__setattr__(self, name, value)

    @property
    def stride(self):
        return self.words.shape[1]

    def total_words(self) -> int:
        return int(self.n_words.to(torch.int64).sum().item())

    @property
    def packed16(self) -> bool:
        """(16,32) words two per 32-bit slot, as the reference's Vec<u16> (CST_FLAG_PACKED_W16): `words` is an int16 tensor and
        every count, stride and offset is in 16-bit words"""
        return self.words.dtype == torch.int16

    def stream(self, s: int) -> np.ndarray:
        n = int(self.n_words[s].item())
        return self.words[s, :n].cpu().numpy().view(np.uint16 if self.packed16 else np.uint32)

    def to_numpy(self):
        return (self.words.cpu().numpy().view(np.uint16 if self.packed16 else np.uint32), self.n_words.cpu().numpy().view(np.uint32),
                self.status.cpu().numpy())


# Provenance of compressed words (round 5).  The (32,64), P <= 12 decoder has two ways of reading its words: 16-byte chunks per
# lane (fastest on words that sit in the GPU's caches: what an encode call on the same HIP stream has just left there) and
# whole 64-byte segments by lane quads (CST_FLAG_COLD_WORDS, cst_ans_dq.hip: 11 - 17 % faster on words that come from HBM -- by
# DMA from the host, from a peer, from a file, or simply written long ago).  The C ABI takes a flag; this layer KNOWS where its
# words come from: ans_encode stamps the EncodedBatch it fills, any later encode on that stream takes the stamp's currency away,
# and words that arrive as plain tensors (packed + offsets, scatter results, container files) never had one.  Batches whose words
# alone exceed the chip's 256-MiB memory-side cache are cold whatever their history.
_INFINITY_CACHE_BYTES = 256 << 20
_launch_serial = [0]
_last_encode = {}        # HIP stream -> serial of the last encode launched on it


def _stamp_fresh(out) -> None:
    _launch_serial[0] += 1
    out._fresh = (torch.cuda.current_stream().cuda_stream, _launch_serial[0])
    _last_encode[out._fresh[0]] = _launch_serial[0]


def _words_are_cold(encoded) -> bool:
    fresh = getattr(encoded, "_fresh", None)
    if fresh is None or fresh[0] != torch.cuda.current_stream().cuda_stream or _last_encode.get(fresh[0]) != fresh[1]:
        return True
    return int(encoded.n_words.numel()) * int(encoded.words.shape[1]) * encoded.words.element_size() > 3 * _INFINITY_CACHE_BYTES   # (slabs are ~1/3 used)


def last_kernel() -> str:
    """the kernel family this thread's last batched coder call launched (cst_last_kernel_name)"""
    return N.lib().cst_last_kernel_name().decode()


def max_words(n_per_stream: int, config=(32, 64, 12)) -> int:
    return N.load_library().cst_ans_max_words(n_per_stream, _cfg(*config))


_TUNED_STRIDES = {}


def tuned_stride(symbols: torch.Tensor, model: "Model", config=(32, 64, 12), layout="stream_major", span=640, step=32,
                 coder="ans", report=None) -> int:
    """The slab stride (words per stream, >= max_words) at which THIS batch shape codes fastest on this device, by measurement.

    How far apart the slabs lie is the caller's choice (`stride_words` of the C ABI), and the P <= 12 ANS decoder is sensitive to
    it: at 65 536 x 4096 it takes 0.25 ms at some strides and 0.35 ms at others, reproducibly, with nothing in the stride's
    residues to go by ("Slab stride": the vector-memory unit takes longer over a load whose 64 lanes
    address 64 lines `stride` apart).  So: encode and decode the given batch at every multiple of `step` words in
    [max_words, max_words + span] (one encode, three decodes each, HIP events), keep the stride with the smallest
    encode + decode time, remember it per (device, shape, preset, layout).  Costs about 30 ms and a few hundred MB of scratch
    the first time; small batches (< 2^26 symbols) get max_words at once.  coder="range": the same for range_encode /
    range_decode.  report: a list that receives (stride, encode_ms, decode_ms) per candidate.  With the environment variable
    CST_STRIDE_CACHE=<file.json> the choice is kept across processes (one file per kind of device)."""
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    n_streams, n_per, _ = _layout_shape(symbols, layout)
    if coder not in ("ans", "range"):
        raise ValueError("coder must be 'ans' or 'range'")
    enc_fn, dec_fn, base = (ans_encode, ans_decode, max_words(n_per, config)) if coder == "ans" else \
                           (range_encode, range_decode, range_max_words(n_per, config))
    # (what picks the kernel: the batch shape, the preset, the layout, the coder, one table or one per stream, the alphabet size)
    kind = ("shared" if model.n_tables == 1 else "per_stream", model.n_symbols)
    key = (symbols.device.index, n_streams, n_per, tuple(config), layout, coder, *kind)
    if key in _TUNED_STRIDES and report is None:
        return _TUNED_STRIDES[key]
    # CST_STRIDE_CACHE=<file.json>: strides measured by earlier processes on this kind of device (a service does not measure at
    # every start; a profiler run of a command that has run before sees the command's own launches only)
    cache_path = os.environ.get("CST_STRIDE_CACHE")
    cache_key = "|".join(map(str, (n_streams, n_per, *config, layout, coder, *kind)))      # (one file per kind of device)
    if cache_path and report is None and os.path.exists(cache_path):
        try:
            with open(cache_path) as f:
                cached = int(json.load(f).get(cache_key, 0))
        except (OSError, ValueError, TypeError, AttributeError):
            cached = 0
        if cached >= base:
            _TUNED_STRIDES[key] = cached
            return cached
    best = base
    if n_streams * n_per >= (1 << 26):
        first = (base + step - 1) // step * step
        cands = [base] + [c for c in range(first, base + span + 1, step) if c != base]
        flat = torch.empty(n_streams * max(cands), dtype=torch.int32, device=symbols.device)
        n_words = torch.empty(n_streams, dtype=torch.int32, device=symbols.device)
        status = torch.empty(n_streams, dtype=torch.int32, device=symbols.device)
        decoded = torch.empty_like(symbols)

        def ms(fn, reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            ev[0].record()
            for k in range(reps):
                fn()
                ev[k + 1].record()
            torch.cuda.synchronize()
            return min(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))

        best_ms = None
        for c in cands:
            enc = EncodedBatch(flat[: n_streams * c].view(n_streams, c), n_words, status, tuple(config))
            enc_fn(symbols, model, config, layout, out=enc)
            te, td = ms(lambda: enc_fn(symbols, model, config, layout, out=enc), 2), ms(lambda: dec_fn(enc, model, n_per, layout, out=decoded), 3)
            if report is not None:
                report.append((c, te, td))
            if best_ms is None or te + td < best_ms:
                best, best_ms = c, te + td
        del flat, decoded
    _TUNED_STRIDES[key] = best
    if cache_path and report is None:
        try:
            known = {}
            if os.path.exists(cache_path):
                with open(cache_path) as f:
                    known = json.load(f)
            known[cache_key] = best
            with open(cache_path, "w") as f:
                json.dump(known, f, indent=1, sort_keys=True)
        except (OSError, ValueError, TypeError):
            pass                                    # (a cache that cannot be written is only a cache)
    return best


def _layout_shape(symbols: torch.Tensor, layout: str):
    if symbols.dim() != 2:
        raise ValueError("symbols must be 2-d")
    if layout == "stream_major":
        return symbols.shape[0], symbols.shape[1], N.LAYOUT_STREAM_MAJOR
    if layout == "symbol_major":
        return symbols.shape[1], symbols.shape[0], N.LAYOUT_SYMBOL_MAJOR
    raise ValueError("layout must be 'stream_major' or 'symbol_major'")


def _new_batch(n_streams, stride, dev, config, packed16=False) -> EncodedBatch:
    return EncodedBatch(torch.empty((n_streams, stride), dtype=torch.int16 if packed16 else torch.int32, device=dev),
                        torch.empty(n_streams, dtype=torch.int32, device=dev),
                        torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config))


def _jump_interval(jump_points, n_per: int, auto) -> int:
    """`jump_points` of an encode call -> symbols between jump points (0 = none).  "auto": the library's own choice for this batch
    (`auto()` asks cst_jump_points_auto); an integer k: k jump points per stream (must divide the row length)."""
    if isinstance(jump_points, str):
        if jump_points != "auto":
            raise ValueError("jump_points must be 'auto' or a number of jump points per stream")
        return int(auto())
    k = int(jump_points or 0)
    if k == 0:
        return 0
    if k < 0 or n_per % k != 0:
        raise ValueError("jump_points must divide the number of symbols per stream")
    return n_per // k


def _jump_table(out: EncodedBatch, kind, interval: int, n_streams: int, n_per: int, dev):
    """the jump table of `out` for this shape: the batch's own one if it has the right form (coding again into the same buffers
    allocates nothing), else a new one"""
    n_chunks = (n_per + interval - 1) // interval
    ck = out.jump
    if isinstance(ck, kind) and ck.interval == interval and tuple(ck.pos.shape) == (n_streams, n_chunks) and ck.pos.device == dev:
        return ck
    if kind is Checkpoints:
        return Checkpoints(interval, torch.zeros((n_streams, n_chunks), dtype=torch.int32, device=dev),
                           torch.zeros((n_streams, n_chunks), dtype=torch.int64, device=dev))
    return RangeCheckpoints(interval, *(torch.zeros((n_streams, n_chunks), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64)))


def ans_encode(symbols: torch.Tensor, model: Model, config=(32, 64, 12), layout="stream_major",
               stride=None, out: Optional[EncodedBatch] = None, packed16: bool = False, jump_points="auto") -> EncodedBatch:
    """One AnsCoder per stream: encode_iid_symbols_reverse + into_compressed (stack.rs:835-849, 891-895).
    jump_points: the encoder can also note `AnsCoder.pos()` (stack.rs:1107-1139) in front of every k-th part of a stream -- the
    words are unchanged, the batch carries the points as `.jump`, and ans_decode then decodes every part on a lane of its own (two
    or more waves per SIMD where a 65 536-stream batch has one).  "auto" (default): where that pays and costs the encoder nothing
    (cst_jump_points_auto: int8 / int16 matrices, tables per stream, P > 12, fewer streams than the chip has lanes; none for
    int32 symbols with one table of P <= 12 at 65 536 streams or more); an integer k: k points per stream (k divides the rows);
    0: none.
    stride: words per slab (default max_words), or "tuned" for the stride measured fastest for this shape (tuned_stride).
    On packed 16-bit words and symbol-major matrices "auto" notes none; an explicit k does (the generic checkpointing encoder supplies the
    table -- slower -- and ans_decode decodes the chunks through the plain decoder with raw states: random access, not speed).
    packed16 (the (16,32) preset only): the words two per 32-bit slot, as the reference's Vec<u16> (CST_FLAG_PACKED_W16) -- the
    batch's `words` is then an int16 tensor; ans_decode and compact recognise it.
    out: an EncodedBatch of an earlier call with the same shapes, to code into the same buffers (its jump table is reused,
    replaced or dropped as this call's jump_points say)."""
    if isinstance(stride, str):
        if stride != "tuned":
            raise ValueError("stride must be a number of words or 'tuned'")
        stride = tuned_stride(symbols, model, config, layout) if out is None else None
    given = symbols
    narrow = _SYMBOL_BYTES.get(symbols.dtype, 4) if symbols.dtype in _SYMBOL_BYTES else 4
    if narrow != 4:
        # int8 / int16 symbol matrices (the reference's Symbol is generic, quantize.rs:229-255; cst_ans_encode_batch_sym): rows of whole
        # 128-byte lines at (32, 64, P <= 12) are read by the encoder loops themselves (round 5: a quarter / half of the symbol bytes in
        # HBM and on the link); every other shape is widened on the device next to the int32 call
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only (map the symbols to indices first)")
        symbols = _require_cuda(symbols, symbols.dtype, "symbols")
    else:
        symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    if out is None:
        out = _new_batch(n_streams, stride or max_words(n_per, config), symbols.device, config, packed16)
    L = N.lib()
    # (packed 16-bit words: "auto" notes none -- the packed decoder's LDS image leaves one workgroup per CU, more lanes would only
    #  queue; an explicit k is honoured for what the reference's Pos / Seek is FOR, random access, see below)
    interval = _jump_interval(0 if out.packed16 and isinstance(jump_points, str) else jump_points, n_per, lambda: L.cst_jump_points_auto(
        model._h, _cfg(*config), N.CODER_ANS, narrow, _ptr(symbols), n_streams, n_per, lay, _ptr(out.words), out.words.shape[1]))
    packed_jump = None
    if interval and out.packed16:
        # AnsCoder::pos() does not depend on how the words are stored (stack.rs:1107-1139: words in the bulk + state).  Chunks of whole
        # tiles: the packed encoder notes them itself.  Other intervals: the WORDS come from the packed encoder below, the TABLE from
        # the checkpointing encoder of the unpacked preset run beside it into a scratch slab (same recurrence, same counts)
        if narrow != 4:
            raise ValueError("packed16 with jump points: int32 symbols")
        packed_jump = _jump_table(out, Checkpoints, interval, n_streams, n_per, symbols.device)
        if interval % 32 == 0 and layout == "stream_major" and 8 <= config[2] <= 12 and not model.noncontiguous:
            # chunks of whole tiles: the packed encoder notes the points on its way (cst_ans_encode_batch_ckpt_packed16)
            N.check(L.cst_ans_encode_batch_ckpt_packed16(model._h, _cfg(*config), _ptr(symbols), n_streams, n_per, _ptr(out.words), out.words.shape[1],
                                                         _ptr(out.n_words), interval, _ptr(packed_jump.pos), _ptr(packed_jump.state), _ptr(out.status),
                                                         _stream_ptr()), "cst_ans_encode_batch_ckpt_packed16")
            out.jump = packed_jump
            _stamp_fresh(out)
            return out
        tmp = _new_batch(n_streams, max_words(n_per, config), symbols.device, config, False)
        ans_encode_checkpointed(given, model, interval, config, layout, out=(tmp, packed_jump))
        del tmp
        interval = 0
    if interval:
        ck = _jump_table(out, Checkpoints, interval, n_streams, n_per, symbols.device)
        ans_encode_checkpointed(given, model, interval, config, layout, out=(out, ck))
        out.jump = ck
        _stamp_fresh(out)
        return out
    out.jump = None              # (an earlier call's jump points describe an earlier call's words)
    flags = N.FLAG_PACKED_W16 if out.packed16 else N.FLAG_NONE
    if narrow != 4:
        scratch = _ckpt_scratch("widen", symbols.device, L.cst_symbols_scratch_bytes(n_streams, n_per, narrow))
        N.check(L.cst_ans_encode_batch_sym(model._h, _cfg(*config), _ptr(symbols), narrow, n_streams, n_per, lay, _ptr(out.words),
                                           out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status), flags, _ptr(scratch),
                                           _stream_ptr()), "cst_ans_encode_batch_sym")
    else:
        N.check(L.cst_ans_encode_batch(model._h, _cfg(*config), _ptr(symbols), n_streams, n_per, lay, _ptr(out.words),
                                       out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status), flags,
                                       _stream_ptr()), "cst_ans_encode_batch")
    out.jump = packed_jump
    _stamp_fresh(out)
    return out


def ans_roundtrip_launcher(symbols: torch.Tensor, model: Model, encoded: EncodedBatch, decoded: torch.Tensor, layout="stream_major"):
    """Returns step(): one cst_ans_encode_batch + one cst_ans_decode_batch over fixed buffers, with every argument converted
    once.  For loops that launch the same pair many times (bench.py's timed steps, a server coding batch after batch into the
    same buffers): ~5 us of host time per launch instead of ~40 us through ans_encode / ans_decode, so that a busy host
    core does not show up as gaps between 0.3-ms kernels.  The launches go to the stream that is current when step() runs."""
    symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    if model.noncontiguous:
        raise ValueError("ans_roundtrip_launcher: contiguous alphabets only")
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    cfg = _cfg(*encoded.config)
    lib = N.lib()
    enc_fn, dec_fn = lib.cst_ans_encode_batch, lib.cst_ans_decode_batch
    words, n_words, status = encoded.words, encoded.n_words, encoded.status
    dstatus = torch.empty(n_streams, dtype=torch.int32, device=symbols.device)
    enc_args = (model._h, cfg, _ptr(symbols), n_streams, n_per, lay, _ptr(words), words.shape[1], _ptr(n_words), None, _ptr(status), N.FLAG_NONE)
    dec_args = (model._h, cfg, _ptr(words), None, words.shape[1], words.numel(), _ptr(n_words), _ptr(decoded), n_streams, n_per, lay, None, None,
                _ptr(dstatus), N.FLAG_NONE)
    keep = (symbols, words, n_words, status, decoded, dstatus, model)      # (the pointers above stay valid as long as step does)

    def step():
        sp = _stream_ptr()
        rc = enc_fn(*enc_args, sp) or dec_fn(*dec_args, sp)
        if rc:
            N.check(rc, "ans_roundtrip_launcher")
    step.keep = keep
    step.decode_status = dstatus
    return step


def ans_decode(encoded, model: Model, n_per_stream: int, layout="stream_major", offsets: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, config=None, cold: Optional[bool] = None, dtype=torch.int32):
    """One AnsCoder per stream: from_compressed + decode_iid_symbols (stack.rs:299-318, mod.rs:1016-1031).
    dtype (or the dtype of `out`): torch.int32, or int16 / int8 for a narrow symbol matrix (cst_ans_decode_batch_sym: written by the
    decoder loops themselves where the rows are whole 128-byte lines at (32, 64, P <= 12), narrowed on the device next to the int32
    call otherwise; the model's support must fit the type).

    `encoded` is an EncodedBatch, or (words, n_words) with `offsets` for the packed layout.  `cold` (CST_FLAG_COLD_WORDS, a hint
    that never changes results): are the words NOT expected in the GPU's caches?  Default None = decided by provenance: hot only
    if `encoded` is the EncodedBatch that the last ans_encode on this HIP stream filled (and small enough to have stayed in the
    caches); words that came from the host, a peer or a file -- plain tensors, packed + offsets -- are cold."""
    jump = encoded.jump if isinstance(encoded, EncodedBatch) else None
    if isinstance(jump, Checkpoints) and offsets is None and \
            n_per_stream == jump.interval * jump.pos.shape[1] and jump.pos.shape[0] == encoded.n_words.numel():
        # the batch carries jump points for exactly this decode (ans_encode, jump_points): every part of a stream on a lane of its
        # own.  (A prefix of the streams, n_per_stream < what was encoded, is a plain decode: the table's rows have another stride.)
        dec, part_status = ans_decode_checkpointed(encoded, jump, model, n_per_stream, out=out, dtype=dtype if out is None else out.dtype,
                                                   layout=layout)
        return dec, _status_per_stream(part_status)
    if isinstance(encoded, EncodedBatch):
        words, n_words, config = encoded.words, encoded.n_words, config or encoded.config
        stride = words.shape[1]
    else:
        words, n_words = encoded
        stride = words.shape[1] if words.dim() == 2 else 0
        config = config or (32, 64, 12)
    if cold is None:
        cold = _words_are_cold(encoded) if isinstance(encoded, EncodedBatch) else True
    n_streams = n_words.numel()
    dev = words.device
    if out is None:
        shape = (n_streams, n_per_stream) if layout == "stream_major" else (n_per_stream, n_streams)
        out = torch.empty(shape, dtype=dtype, device=dev)
    lay = N.LAYOUT_STREAM_MAJOR if layout == "stream_major" else N.LAYOUT_SYMBOL_MAJOR
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    narrow = _SYMBOL_BYTES.get(out.dtype)
    if narrow is None:
        raise TypeError("decoded symbols are int32, int16 or int8")
    flags = (N.FLAG_COLD_WORDS if cold else N.FLAG_NONE) | (N.FLAG_PACKED_W16 if words.dtype == torch.int16 else N.FLAG_NONE)
    if narrow != 4:
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only")
        L = N.lib()
        scratch = _ckpt_scratch("narrow", dev, L.cst_symbols_scratch_bytes(n_streams, n_per_stream, narrow))
        N.check(L.cst_ans_decode_batch_sym(model._h, _cfg(*config), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words),
                                           _ptr(out), narrow, n_streams, n_per_stream, lay, None, None, _ptr(status),
                                           flags, _ptr(scratch), _stream_ptr()), "cst_ans_decode_batch_sym")
        return out, status
    N.check(N.lib().cst_ans_decode_batch(model._h, _cfg(*config), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words),
                                         _ptr(out), n_streams, n_per_stream, lay, None, None, _ptr(status),
                                         flags, _stream_ptr()), "cst_ans_decode_batch")
    return _to_symbols(model, out), status


_scratch = {}


# ---------------------------------------------------------------------------------------------------------------------
# streams of different lengths: thousands of small coders with one model in one launch (the reference's "compressed index"
# pattern, tests/issue52.rs: one AnsCoder per document)
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class RaggedBatch:
    """Compressed words of streams of different lengths: stream s owns words[word_offsets[s] : word_offsets[s] + n_words[s]]."""
    words: torch.Tensor          # int32, flat
    word_offsets: torch.Tensor   # int64 [n_streams + 1]: the slabs (a slab is at least as long as its stream can get)
    n_words: torch.Tensor        # int32 [n_streams]
    status: torch.Tensor         # int32 [n_streams]
    config: tuple
    order: Optional[torch.Tensor] = None   # int32 [n_streams]: the schedule the encoder ran with (the decoders reuse it)
    jump: Optional["RaggedJump"] = None    # jump points the encoder noted (ans_encode_ragged, jump_every): ans_decode_ragged decodes the chunks side by side
    #                                        (a range batch carries a RangeRaggedJump here: range_encode_ragged_jump / range_decode_ragged)
    coder: str = "ans"                     # "ans" (a stack) or "range" (a queue): which coder wrote the words -- the other one's decoders refuse them
    #                                        ("exp_golomb": exp_golomb_encode_ragged, "huffman": huffman_encode_ragged; config is then
    #                                        (semantics, symbol dtype), and a Huffman batch's `jump` is a BitJump)
    n_bits = None                          # (no field: set by the symbol codes) int64 [n_streams], the written bits of every stream

    def stream(self, s: int) -> np.ndarray:
        """get_compressed() of stream s (uint32, host)."""
        lo, n = int(self.word_offsets[s].item()), int(self.n_words[s].item())
        return self.words[lo: lo + n].cpu().numpy().view(np.uint32)


@dataclass
class RaggedJump:
    """AnsCoder.pos() in front of every `interval` symbols of every stream of a RaggedBatch (stack.rs:1107-1139): chunk j of stream s is
    entry chunk_offsets[s] + j of pos (words in the bulk) / state (the coder state there)."""
    interval: int
    chunk_offsets: torch.Tensor   # int64 [n_streams + 1]: exclusive prefix sum of ceil(length / interval)
    pos: torch.Tensor             # int32 [>= total chunks]
    state: torch.Tensor           # int64 [>= total chunks]


@dataclass
class RangeRaggedJump:
    """RangeEncoder.pos() in front of every `interval` symbols of every stream of a range RaggedBatch (queue.rs:172-196): chunk j of
    stream s is entry chunk_offsets[s] + j of pos (words emitted so far, held-back ones included) / lower / range (the coder state there)."""
    interval: int
    chunk_offsets: torch.Tensor   # int64 [n_streams + 1]: exclusive prefix sum of ceil(length / interval)
    pos: torch.Tensor             # int32 [>= total chunks]
    lower: torch.Tensor           # int64 [>= total chunks]
    range: torch.Tensor           # int64 [>= total chunks]


RAGGED_JUMP_EVERY = 256            # jump_every="auto": symbols between the jump points of a ragged batch


def ragged(sequences, device="cuda"):
    """list of 1-d integer arrays -> (flat int32 device tensor, int64 offsets [n + 1]) as the ragged entry points take them."""
    lengths = np.fromiter((len(x) for x in sequences), dtype=np.int64, count=len(sequences))
    offsets = np.zeros(len(sequences) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in sequences]) if len(sequences) else np.zeros(0, np.int32)
    return torch.from_numpy(flat).to(device), torch.from_numpy(offsets).to(device)


RAGGED_BALANCE_FROM = 250_000      # streams from which `order="auto"` sorts: below, the launch is bound by its longest stream anyway


def ragged_order(keys: torch.Tensor) -> torch.Tensor:
    """The schedule of the `*_ragged_ordered` entry points for streams whose cost grows with `keys` (lengths for the encoder,
    word counts for the decoders): stream indices, longest first, so that the 64 streams of a wave are about equally long."""
    return torch.sort(keys.to(torch.int32), descending=True).indices.to(torch.int32)


def _ragged_order(order, n_streams, keys):
    """`order` argument of the ragged calls: None (slot i = stream i), "auto" (sorted from RAGGED_BALANCE_FROM streams on),
    "sorted", or an int32 permutation on the device."""
    if order is None or (isinstance(order, str) and order == "auto" and n_streams < RAGGED_BALANCE_FROM):
        return None
    if isinstance(order, str):
        if order not in ("auto", "sorted"):
            raise ValueError('order: None, "auto", "sorted" or an int32 tensor of stream indices')
        return ragged_order(keys)
    order = _require_cuda(order, torch.int32, "order")
    if order.numel() != n_streams:
        raise ValueError("order must hold one stream index per stream")
    return order


def _ragged_per_stream(model: Model, n_streams: int, config) -> bool:
    """What the ragged calls ask of a model with one table per stream (quantized_gaussian_per_stream, from_cdf_rows_per_stream,
    fit_per_stream with sym_offsets), said before any launch.  False: a shared table, of which nothing is asked here."""
    if not (model.per_stream or model.n_tables != 1):
        return False
    if model.noncontiguous:
        raise ValueError("tables per stream: contiguous alphabets only")
    if model.n_tables != n_streams:
        raise ValueError(f"the model has {model.n_tables} tables, the batch {n_streams} streams: one table per stream")
    W, S, P = (int(x) for x in config)
    if P != model.precision:
        raise ValueError(f"the config's precision is {P}, the model's {model.precision}")
    if (W, S) not in ((32, 64), (16, 32)):
        raise ValueError("tables per stream: presets (32, 64) and (16, 32) only")
    return True


def _refuse_per_stream(model: Model, what: str) -> None:
    if model.per_stream or model.n_tables != 1:
        raise ValueError(f"{what}: shared tables only (a model with one table per stream decodes whole batches: ans_decode_ragged / "
                         f"range_decode_ragged)")


def _require_coder(encoded: RaggedBatch, coder: str) -> None:
    if encoded.coder != coder:
        raise ValueError(f"the batch holds the words of the {encoded.coder!r} coder: a {coder!r} decoder cannot read them")


def ans_encode_ragged(symbols: torch.Tensor, sym_offsets: torch.Tensor, model: Model, config=(32, 64, 24), order="auto",
                      jump_every="auto") -> RaggedBatch:
    """One AnsCoder per stream, streams of different lengths (`symbols` flat, stream s = symbols[sym_offsets[s]:sym_offsets[s+1]]):
    encode_iid_symbols_reverse + into_compressed per stream (stack.rs:835-849, 891-895) in ONE launch.  `order`: see
    _ragged_order (big batches of very different lengths run 1.5 - 3x faster with their streams sorted by length; the
    results do not depend on it).
    jump_every: the encoder also notes AnsCoder.pos() in front of every jump_every symbols of every stream (a multiple of 8; the words
    are unchanged) and the batch carries the table as `.jump`: ans_decode_ragged then decodes all chunks side by side -- a launch
    lasts as long as its longest CHAIN, and a 2000-symbol document among short ones is 2000 dependent steps without jump points.
    "auto" (default): every RAGGED_JUMP_EVERY symbols if the streams average more than a quarter of that; 0: none.
    model: one shared table, or ONE TABLE PER STREAM (Model.fit_per_stream(..., sym_offsets=), from_cdf_rows_per_stream,
    quantized_gaussian_per_stream): as many tables as streams, contiguous alphabets, presets (32, 64) and (16, 32), the config's precision
    the model's (<= 16) -- anything else raises ValueError before a launch.  Stream s is coded with table s; its words are those of
    ans_encode for that stream alone.  With tables per stream "auto" notes NO jump points (every chunk lane of the decoder stages its own
    copy of its stream's row, and nothing has measured where that pays); an explicit jump_every is honoured."""
    symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if symbols.dim() != 1 or n_streams < 0:
        raise ValueError("symbols must be flat and sym_offsets hold n_streams + 1 entries")
    per_stream = _ragged_per_stream(model, n_streams, config)
    W, S, P = config
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    # a stream of n symbols fills at most min(n, ceil(n P / W)) + S / W words (cst_ans_max_words without its rounding to 64 bytes:
    # thousands of short streams; 16-byte slabs keep the chunk stores aligned)
    bound = torch.minimum(lengths, (lengths * P + (W - 1)) // W) + S // W
    slabs = (bound + 3) // 4 * 4
    word_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=symbols.device)
    torch.cumsum(slabs, 0, out=word_offsets[1:])
    total = int(word_offsets[-1].item()) if n_streams else 0
    dev = symbols.device
    order = _ragged_order(order, n_streams, lengths)
    out = RaggedBatch(torch.empty(max(total, 4), dtype=torch.int32, device=dev), word_offsets,
                      torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config),
                      order)
    if isinstance(jump_every, str):
        if jump_every != "auto":
            raise ValueError("jump_every: 'auto', 0 or a multiple of 8")
        jump_every = RAGGED_JUMP_EVERY if n_streams > 0 and symbols.numel() * 4 > n_streams * RAGGED_JUMP_EVERY and not per_stream else 0
    jump_every = int(jump_every or 0)
    if jump_every < 0 or jump_every % 8 != 0:
        raise ValueError("jump_every: 'auto', 0 or a multiple of 8")
    if jump_every and n_streams > 0:
        chunk_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        torch.cumsum((lengths + (jump_every - 1)) // jump_every, 0, out=chunk_offsets[1:])
        # (no read-back of the total: sum(ceil(len / I)) <= total / I + n_streams bounds it, entries behind the last chunk stay unused)
        n_chunks = symbols.numel() // jump_every + n_streams
        jump = RaggedJump(jump_every, chunk_offsets, torch.empty(max(n_chunks, 1), dtype=torch.int32, device=dev),
                          torch.empty(max(n_chunks, 1), dtype=torch.int64, device=dev))
        N.check(N.lib().cst_ans_encode_ragged_jump(model._h, _cfg(*config), _ptr(symbols), _ptr(sym_offsets), n_streams,
                                                   _ptr(order) if order is not None else None, _ptr(out.words), _ptr(word_offsets), 0,
                                                   _ptr(out.n_words), jump_every, _ptr(chunk_offsets), _ptr(jump.pos), _ptr(jump.state),
                                                   _ptr(out.status), _stream_ptr()), "cst_ans_encode_ragged_jump")
        out.jump = jump
        return out
    N.check(N.lib().cst_ans_encode_ragged_ordered(model._h, _cfg(*config), _ptr(symbols), _ptr(sym_offsets), n_streams,
                                                  _ptr(order) if order is not None else None, _ptr(out.words), _ptr(word_offsets), 0,
                                                  _ptr(out.n_words), _ptr(out.status), _stream_ptr()), "cst_ans_encode_ragged_ordered")
    return out


def ans_decode_ragged(encoded: RaggedBatch, model: Model, sym_offsets: torch.Tensor, out: Optional[torch.Tensor] = None, order="auto"):
    """from_compressed + decode_iid_symbols per stream (stack.rs:299-318, 1070-1100): stream s yields
    sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:].  Returns (symbols flat, status per stream).
    `order`: the schedule (see _ragged_order); "auto" reuses the encoder's, or sorts by word count from RAGGED_BALANCE_FROM
    streams on.
    model: the shared table, or the per-stream model the batch was encoded with (as many tables as streams; ValueError otherwise, or if
    the batch's precision is not the model's); a table of jump points is followed for either."""
    _require_coder(encoded, "ans")
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    _ragged_per_stream(model, n_streams, encoded.config)
    # a batch with jump points decodes its chunks side by side (they are all at most `interval` symbols long: no schedule needed) --
    # unless the caller hands in a schedule of their own, which is then honoured on the whole streams
    take_jump = encoded.jump is not None and (order is None or (isinstance(order, str) and order == "auto"))
    if isinstance(order, str) and order == "auto" and encoded.order is not None and encoded.order.numel() == n_streams:
        order = encoded.order
    order = _ragged_order(order, n_streams, encoded.n_words)
    dev = encoded.words.device
    total = int(sym_offsets[-1].item()) if n_streams > 0 else 0
    if out is None:
        out = torch.empty(total, dtype=torch.int32, device=dev)
    status = torch.empty(max(n_streams, 0), dtype=torch.int32, device=dev)
    jump = encoded.jump
    if take_jump and n_streams > 0 and jump.chunk_offsets.numel() == n_streams + 1:
        # the batch carries jump points: every chunk of every stream on a lane of its own (the table is checked against the lengths on
        # the device: a stream it does not describe reports INVALID_DATA)
        L = N.lib()
        n_chunks = int(jump.pos.numel())              # (an upper bound of the chunks is enough: entries behind the last chunk are empty streams)
        scratch = _ckpt_scratch("ragged_jump", dev, L.cst_ragged_jump_scratch_bytes(n_chunks))
        N.check(L.cst_ans_decode_ragged_jump(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0, encoded.words.numel(),
                                             _ptr(encoded.n_words), _ptr(out), _ptr(sym_offsets), n_streams, jump.interval, _ptr(jump.chunk_offsets),
                                             n_chunks, _ptr(jump.pos), _ptr(jump.state), _ptr(scratch), _ptr(status), _stream_ptr()),
                "cst_ans_decode_ragged_jump")
        return _to_symbols(model, out), status
    N.check(N.lib().cst_ans_decode_ragged_ordered(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                  encoded.words.numel(), _ptr(encoded.n_words), _ptr(out), _ptr(sym_offsets), n_streams,
                                                  _ptr(order) if order is not None else None, _ptr(status), _stream_ptr()),
            "cst_ans_decode_ragged_ordered")
    return _to_symbols(model, out), status


def ans_decode_until(encoded: RaggedBatch, model: Model, eof_symbol: int, max_symbols: Optional[int] = None):
    """Streams whose length is not stored: every stream is decoded until `eof_symbol` (tests/issue52.rs:63-80).  Two launches
    -- count, prefix sum, decode.  Returns (symbols flat, sym_offsets [n + 1], status); the terminator is the last symbol of
    every stream; status CAPACITY (2): no terminator among the first max_symbols symbols -- such a stream (corrupt data, a wrong
    eof_symbol) decodes to NO symbols: its length is 0 in sym_offsets, so that a batch of bad documents cannot ask for
    n_streams x max_symbols symbols of output.  max_symbols defaults to 2^20.  Shared tables only: a model with one table per stream
    raises ValueError."""
    _refuse_per_stream(model, "ans_decode_until")
    max_symbols = (1 << 20) if max_symbols is None else int(max_symbols)
    if model.noncontiguous:
        raise ValueError("ans_decode_until: contiguous alphabets only")
    n_streams = encoded.n_words.numel()
    dev = encoded.words.device
    lengths = torch.zeros(n_streams, dtype=torch.int64, device=dev)
    status = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    order = encoded.order if encoded.order is not None and encoded.order.numel() == n_streams else _ragged_order("auto", n_streams, encoded.n_words)
    N.check(N.lib().cst_ans_count_until_ordered(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                                encoded.words.numel(), _ptr(encoded.n_words), n_streams,
                                                _ptr(order) if order is not None else None, int(eof_symbol), int(max_symbols),
                                                _ptr(lengths), _ptr(status), _stream_ptr()), "cst_ans_count_until_ordered")
    lengths = torch.where(status != 0, torch.zeros_like(lengths), lengths)      # (a stream without a terminator is not decoded)
    sym_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lengths, 0, out=sym_offsets[1:])
    symbols, status2 = ans_decode_ragged(encoded, model, sym_offsets, order=order)
    return symbols, sym_offsets, torch.where(status != 0, status, status2)


# ... the same three for the range coder, the reference's QUEUE (one RangeEncoder / RangeDecoder per document, queue.rs): the symbols
# come back in the order they were written, so a document's terminator is simply its last symbol

def _range_jump_every(jump_every) -> object:
    """the `jump_every` argument, judged before any tensor is looked at: "auto", or an int that is 0 or a positive multiple of 8"""
    if isinstance(jump_every, str):
        if jump_every != "auto":
            raise ValueError("jump_every: 'auto', 0 or a multiple of 8")
        return "auto"
    jump_every = int(jump_every or 0)
    if jump_every < 0 or jump_every % 8 != 0:
        raise ValueError("jump_every: 'auto', 0 or a multiple of 8")
    return jump_every


def range_encode_ragged(symbols: torch.Tensor, sym_offsets: torch.Tensor, model: Model, config=(32, 64, 24), order="auto") -> RaggedBatch:
    """One RangeEncoder per stream, streams of different lengths (`symbols` flat, stream s = symbols[sym_offsets[s]:sym_offsets[s+1]]):
    encode_iid_symbols + get_compressed per stream (queue.rs:612-705, 458-523) in ONE launch.  Every stream's words are those of
    range_encode for that stream alone; a slab holds min(n, ceil(n P / W)) + 2 words, rounded up to 4.  The batch says
    `.coder == "range"`, carries no jump points (`.jump` is None) and the schedule it ran with in `.order` (see _ragged_order).
    model: one shared table, or one table per stream (as many tables as streams, contiguous alphabets, presets (32, 64) and (16, 32), the
    config's precision the model's: ValueError otherwise, before a launch); stream s is then coded with table s, its words those of
    range_encode for that stream alone."""
    return _range_encode_ragged(symbols, sym_offsets, model, config, order, 0)


def range_encode_ragged_jump(symbols: torch.Tensor, sym_offsets: torch.Tensor, model: Model, config=(32, 64, 24), order="auto",
                             jump_every="auto") -> RaggedBatch:
    """range_encode_ragged that also notes RangeEncoder.pos() in front of every `jump_every` symbols of every stream (a multiple of 8; the
    words, counts and statuses are unchanged).  The batch carries the table as `.jump` (a RangeRaggedJump), and range_decode_ragged then
    decodes all chunks side by side: a launch lasts as long as its longest CHAIN, and a range step costs more than an ANS step.
    "auto" (default): every RAGGED_JUMP_EVERY symbols if the streams average MORE than RAGGED_JUMP_EVERY symbols, i.e. more than one
    chunk each (not the ANS rule of a quarter of that: 100 000 documents of 200 symbols, one chunk each, encode in 0.133 instead of
    0.104 ms and decode in 0.142 instead of 0.126 ms with a table that buys them nothing, while documents of 20 .. 2000 symbols, 430 on
    average, decode in 0.30 instead of 0.94 ms for 0.55 instead of 0.51 ms of encoding); 0: none -- the result is
    exactly range_encode_ragged's.  A model with one table per stream (see range_encode_ragged): "auto" is 0 -- every chunk lane of the
    decoder stages its own copy of its stream's row, nothing has measured where that pays, and on rectangular per-stream batches the
    points were a loss --, an explicit jump_every is honoured."""
    return _range_encode_ragged(symbols, sym_offsets, model, config, order, _range_jump_every(jump_every))


def _range_encode_ragged(symbols, sym_offsets, model, config, order, jump_every) -> RaggedBatch:
    """the body of range_encode_ragged (jump_every = 0) and range_encode_ragged_jump (jump_every as _range_jump_every returns it)"""
    symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if symbols.dim() != 1 or sym_offsets.dim() != 1 or n_streams < 0:
        raise ValueError("symbols must be flat and sym_offsets hold n_streams + 1 entries")
    per_stream = _ragged_per_stream(model, n_streams, config)
    W, S, P = config
    dev = symbols.device
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    # a stream of n symbols fills at most min(n, ceil(n P / W)) words plus the 2 that seal it (the bound inside cst_range_max_words,
    # without its rounding to 64 bytes: thousands of short streams); 16-byte slabs keep the chunk stores aligned
    bound = torch.minimum(lengths, (lengths * P + (W - 1)) // W) + 2
    slabs = (bound + 3) // 4 * 4
    word_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(slabs, 0, out=word_offsets[1:])
    total = int(word_offsets[-1].item()) if n_streams else 0
    order = _ragged_order(order, n_streams, lengths)
    out = RaggedBatch(torch.empty(max(total, 4), dtype=torch.int32, device=dev), word_offsets,
                      torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config),
                      order, None, "range")
    if n_streams == 0:
        return out
    if jump_every == "auto":
        jump_every = RAGGED_JUMP_EVERY if symbols.numel() > n_streams * RAGGED_JUMP_EVERY and not per_stream else 0
    if jump_every:
        chunk_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        torch.cumsum((lengths + (jump_every - 1)) // jump_every, 0, out=chunk_offsets[1:])
        # (no read-back of the total: sum(ceil(len / I)) <= total / I + n_streams bounds it, entries behind the last chunk stay unused)
        n_chunks = max(symbols.numel() // jump_every + n_streams, 1)
        jump = RangeRaggedJump(jump_every, chunk_offsets, torch.empty(n_chunks, dtype=torch.int32, device=dev),
                               torch.empty(n_chunks, dtype=torch.int64, device=dev), torch.empty(n_chunks, dtype=torch.int64, device=dev))
        N.check(N.lib().cst_range_encode_ragged_jump(model._h, _cfg(*config), _ptr(symbols), _ptr(sym_offsets), n_streams,
                                                     _ptr(order) if order is not None else None, _ptr(out.words), _ptr(word_offsets), 0,
                                                     _ptr(out.n_words), jump_every, _ptr(chunk_offsets), _ptr(jump.pos), _ptr(jump.lower),
                                                     _ptr(jump.range), _ptr(out.status), _stream_ptr()), "cst_range_encode_ragged_jump")
        out.jump = jump
        return out
    N.check(N.lib().cst_range_encode_ragged(model._h, _cfg(*config), _ptr(symbols), _ptr(sym_offsets), n_streams,
                                            _ptr(order) if order is not None else None, _ptr(out.words), _ptr(word_offsets), 0,
                                            _ptr(out.n_words), _ptr(out.status), _stream_ptr()), "cst_range_encode_ragged")
    return out


def range_decode_ragged(encoded: RaggedBatch, model: Model, sym_offsets: torch.Tensor, out: Optional[torch.Tensor] = None, order="auto"):
    """from_compressed + decode_iid_symbols per stream (queue.rs:776-790, 968-1033): stream s yields
    sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:], in the order they were encoded.  Returns (symbols flat,
    status per stream).  `order`: the schedule (see _ragged_order); "auto" reuses the encoder's, or sorts by word count from
    RAGGED_BALANCE_FROM streams on.  A batch with jump points (range_encode_ragged_jump) decodes its chunks side by side when `order` is
    None or "auto"; a schedule handed in is honoured on the whole streams.
    model: the shared table, or the per-stream model the batch was encoded with (as many tables as streams; ValueError otherwise, or if
    the batch's precision is not the model's); a table of jump points is followed for either."""
    _require_coder(encoded, "range")
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    _ragged_per_stream(model, n_streams, encoded.config)
    if sym_offsets.dim() != 1 or encoded.n_words.numel() != n_streams:
        raise ValueError("sym_offsets does not match the number of streams of the batch")
    jump = encoded.jump
    if jump is not None and not isinstance(jump, RangeRaggedJump):
        raise ValueError("the batch carries the jump points of another coder")
    take_jump = jump is not None and (order is None or (isinstance(order, str) and order == "auto"))
    if isinstance(order, str) and order == "auto" and encoded.order is not None and encoded.order.numel() == n_streams:
        order = encoded.order
    order = _ragged_order(order, n_streams, encoded.n_words)
    dev = encoded.words.device
    total = int(sym_offsets[-1].item()) if n_streams > 0 else 0
    if out is None:
        out = torch.empty(total, dtype=torch.int32, device=dev)
    else:
        out = _require_cuda(out, torch.int32, "out")
        if out.dim() != 1 or out.numel() < total:
            raise ValueError("out must be flat and hold every stream's symbols")
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    if n_streams == 0:
        return _to_symbols(model, out), status
    if take_jump and jump.chunk_offsets.numel() == n_streams + 1:
        # every chunk of every stream on a lane of its own (the table is checked against the lengths on the device: a stream it does not
        # describe reports INVALID_DATA); an upper bound of the chunks is enough, entries behind the last chunk are empty
        L = N.lib()
        n_chunks = min(int(jump.pos.numel()), int(jump.lower.numel()), int(jump.range.numel()))
        scratch = _ckpt_scratch("range_ragged_jump", dev, L.cst_range_ragged_jump_scratch_bytes(n_chunks))
        N.check(L.cst_range_decode_ragged_jump(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                               encoded.words.numel(), _ptr(encoded.n_words), _ptr(out), _ptr(sym_offsets), n_streams,
                                               jump.interval, _ptr(jump.chunk_offsets), n_chunks, _ptr(jump.pos), _ptr(jump.lower),
                                               _ptr(jump.range), _ptr(scratch), _ptr(status), _stream_ptr()), "cst_range_decode_ragged_jump")
        return _to_symbols(model, out), status
    N.check(N.lib().cst_range_decode_ragged(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                            encoded.words.numel(), _ptr(encoded.n_words), _ptr(out), _ptr(sym_offsets), n_streams,
                                            _ptr(order) if order is not None else None, _ptr(status), _stream_ptr()),
            "cst_range_decode_ragged")
    return _to_symbols(model, out), status


# ... and random access: selected documents, or ranges of documents, of a ragged batch (what the reference's `Seek` is for)

def _select_piece_counts(first: torch.Tensor, count: torch.Tensor, interval: int) -> torch.Tensor:
    """Pieces of the queries (first, count) of a select call (int64 tensors on any device): one per chunk of `interval` symbols a query
    touches -- ceil((first % interval + count) / interval), none for count 0; without a table (interval 0) one piece per query that
    asks for anything."""
    if interval == 0:
        return (count > 0).to(torch.int64)
    return torch.where(count > 0, (first % interval + count + (interval - 1)) // interval, torch.zeros_like(count))


class _SelectQueries:
    """what _select_queries prepares for a select call: the queries as the entry points take them, and the output"""
    __slots__ = ("sym_offsets", "n_streams", "n_queries", "whole", "query_stream", "first", "count", "interval", "out_offsets", "piece_offsets",
                 "total", "n_pieces", "out", "status", "max_piece")


def _select_queries(encoded, jump, sym_offsets, streams, first, count, out, piece_bound=False, dtype=None, dtypes=None) -> _SelectQueries:
    """The query preparation of every select call (shared-table and per-symbol models alike), once the batch's coder and the type of its
    jump table are judged: the queries as tensors, their sizes and pieces, the two prefix sums, the single read-back (the output
    total), an upper bound of the pieces, the output and the statuses.  `jump`: the batch's table or None.  `piece_bound`: also
    `max_piece`, an upper bound of the symbols any piece decodes, dropped ones included -- the interval, or without a table the largest
    first + count of the queries the device can accept, which travels with the output total in the same read-back.  `dtype` / `dtypes`
    (the symbol codes): the type of a fresh output and the types an `out` may have; by default both are int32."""
    r = _SelectQueries()
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if sym_offsets.dim() != 1 or encoded.n_words.numel() != n_streams:
        raise ValueError("sym_offsets does not match the number of streams of the batch")
    dev = encoded.words.device
    streams = torch.as_tensor(streams, device=dev)
    if streams.dtype.is_floating_point or streams.dtype.is_complex or streams.dtype == torch.bool or streams.dim() != 1:
        raise TypeError("streams: a flat integer tensor or sequence of document indices")
    streams = streams.to(torch.int64)
    n_queries = streams.numel()
    whole = first is None and count is None

    def as_i64(x, name):
        x = torch.as_tensor(x, device=dev)
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool or x.shape != streams.shape:
            raise TypeError(f"{name}: one integer per query")
        return x.to(torch.int64).contiguous()

    # everything below is device arithmetic on caller data the kernels judge again: a query the device will refuse (a stream that is
    # none, a range beyond its document) only has to get SOME slice here -- never one larger than a document
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    known = (streams >= 0) & (streams < n_streams)
    doc = torch.where(known, lengths[streams.clamp(0, max(n_streams - 1, 0))], torch.zeros_like(streams)) if n_streams > 0 else torch.zeros_like(streams)
    query_stream = torch.where(known, streams, torch.full_like(streams, 0xffffffff)).to(torch.int32)
    if not whole:
        first = as_i64(first, "first") if first is not None else torch.zeros_like(streams)
        count = as_i64(count, "count") if count is not None else (doc - first).clamp(min=0)
    sizes = doc if whole else torch.minimum(count.clamp(min=0), doc)
    interval = int(jump.interval) if jump is not None and jump.chunk_offsets.numel() == n_streams + 1 else 0
    pieces = _select_piece_counts(torch.zeros_like(sizes) if whole else first, sizes, interval)
    out_offsets = torch.zeros(n_queries + 1, dtype=torch.int64, device=dev)
    piece_offsets = torch.zeros(n_queries + 1, dtype=torch.int64, device=dev)
    torch.cumsum(sizes, 0, out=out_offsets[1:])
    torch.cumsum(pieces, 0, out=piece_offsets[1:])
    max_piece = interval
    if piece_bound and not interval and n_queries > 0:
        ends = doc if whole else torch.where((first >= 0) & (first <= doc) & (count >= 0) & (count <= doc - first), first + count,
                                             torch.zeros_like(doc))
        total, max_piece = (int(x) for x in torch.stack((out_offsets[-1], ends.max())).tolist())
    else:
        total = int(out_offsets[-1].item()) if n_queries > 0 else 0     # (the only read-back, as ans_decode_ragged reads sym_offsets[-1])
    # a query of `count` symbols has at most count // I + 2 pieces: an upper bound of the pieces, without a second read-back
    n_pieces = (total // interval + 2 * n_queries) if interval else n_queries
    if out is None:
        out = torch.empty(total, dtype=dtype or torch.int32, device=dev)
    else:
        if dtypes is None:
            out = _require_cuda(out, torch.int32, "out")
        elif not isinstance(out, torch.Tensor) or not out.is_cuda or not out.is_contiguous() or out.dtype not in dtypes:
            raise ValueError("out must be a contiguous device tensor of one of the coder's symbol types")
        if out.dim() != 1 or out.numel() < total:
            raise ValueError("out must be flat and hold every query's symbols")
    r.sym_offsets, r.n_streams, r.n_queries, r.whole, r.query_stream, r.first, r.count = sym_offsets, n_streams, n_queries, whole, query_stream, first, count
    r.interval, r.out_offsets, r.piece_offsets, r.total, r.n_pieces, r.out = interval, out_offsets, piece_offsets, total, n_pieces, out
    r.status = torch.empty(n_queries, dtype=torch.int32, device=dev)
    r.max_piece = max_piece
    return r


def _select_tail(r: _SelectQueries):
    """the query block and the output of a select entry point, up to d_out_offsets"""
    return (_ptr(r.query_stream), None if r.whole else _ptr(r.first), None if r.whole else _ptr(r.count), r.n_queries, _ptr(r.piece_offsets),
            r.n_pieces, _ptr(r.out), _ptr(r.out_offsets))


def _symbol_decode_ragged_select(coder, encoded, sym_offsets, streams, first, count, out, dtypes, entry, head):
    """the body of huffman_decode_ragged_select and exp_golomb_decode_ragged_select (`dtypes`: symbol type -> symbol_bytes; `head`: the
    arguments in front of `semantics`, made once the batch has been judged)"""
    from ._huffman import BitJump, _semantics
    _require_coder(encoded, coder)
    jump = encoded.jump
    if jump is not None and not isinstance(jump, BitJump):
        raise ValueError("the batch carries the jump points of another coder")
    semantics, dtype = encoded.config
    r = _select_queries(encoded, jump, sym_offsets, streams, first, count, out, dtype=dtype, dtypes=dtypes)
    if r.n_queries == 0:
        return r.out[:0], r.out_offsets, r.status
    L = N.lib()
    table = (r.interval, _ptr(jump.chunk_offsets), int(jump.bits.numel()), _ptr(jump.bits)) if r.interval else (0, None, 0, None)
    scratch = _ckpt_scratch("ragged_select", encoded.words.device, L.cst_ragged_select_scratch_bytes(r.n_pieces))
    out_ptr = _ptr(r.out) if r.out.numel() else _ptr(torch.empty(4, dtype=torch.int32, device=r.out.device))     # (the ABI refuses NULL)
    N.check(getattr(L, entry)(*head(), _semantics(semantics), _ptr(encoded.words), _ptr(encoded.word_offsets), 0, encoded.words.numel(),
                              _ptr(encoded.n_words), _ptr(r.sym_offsets), r.n_streams, *table, _ptr(r.query_stream),
                              None if r.whole else _ptr(r.first), None if r.whole else _ptr(r.count), r.n_queries, _ptr(r.piece_offsets),
                              r.n_pieces, out_ptr, dtypes[r.out.dtype], _ptr(r.out_offsets), _ptr(scratch), _ptr(r.status), _stream_ptr()),
            entry)
    return r.out[:r.total], r.out_offsets, r.status


def _decode_ragged_select(coder, jump_type, encoded, model, sym_offsets, streams, first, count, out):
    """the body of ans_decode_ragged_select and range_decode_ragged_select"""
    _require_coder(encoded, coder)
    jump = encoded.jump
    if jump is not None and not isinstance(jump, jump_type):
        raise ValueError("the batch carries the jump points of another coder")
    _refuse_per_stream(model, f"{coder}_decode_ragged_select")
    r = _select_queries(encoded, jump, sym_offsets, streams, first, count, out)
    sym_offsets, n_streams, interval, n_pieces, out, out_offsets, status, total = (r.sym_offsets, r.n_streams, r.interval, r.n_pieces, r.out,
                                                                                   r.out_offsets, r.status, r.total)
    dev = encoded.words.device
    if r.n_queries == 0:
        return out[:0], out_offsets, status
    L = N.lib()
    head = (model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0, encoded.words.numel(), _ptr(encoded.n_words),
            _ptr(sym_offsets), n_streams)
    tail = _select_tail(r)
    if coder == "ans":
        table = (interval, _ptr(jump.chunk_offsets), min(int(jump.pos.numel()), int(jump.state.numel())), _ptr(jump.pos),
                 _ptr(jump.state)) if interval else (0, None, 0, None, None)
        scratch = _ckpt_scratch("ragged_select", dev, L.cst_ragged_select_scratch_bytes(n_pieces))
        N.check(L.cst_ans_decode_ragged_select(*head, *table, *tail, _ptr(scratch), _ptr(status), _stream_ptr()), "cst_ans_decode_ragged_select")
    else:
        table = (interval, _ptr(jump.chunk_offsets), min(int(jump.pos.numel()), int(jump.lower.numel()), int(jump.range.numel())), _ptr(jump.pos),
                 _ptr(jump.lower), _ptr(jump.range)) if interval else (0, None, 0, None, None, None)
        scratch = _ckpt_scratch("range_ragged_select", dev, L.cst_range_ragged_select_scratch_bytes(n_pieces))
        N.check(L.cst_range_decode_ragged_select(*head, *table, *tail, _ptr(scratch), _ptr(status), _stream_ptr()), "cst_range_decode_ragged_select")
    return _to_symbols(model, out[:total]), out_offsets, status


def ans_decode_ragged_select(encoded: RaggedBatch, model: Model, sym_offsets: torch.Tensor, streams, first=None, count=None,
                             out: Optional[torch.Tensor] = None):
    """Random access into a ragged ANS batch: query q decodes symbols [first[q], first[q] + count[q]) of document streams[q], and
    nothing else is decoded.  `streams`: an integer tensor or sequence, in any order, repeats and overlaps allowed; `first` / `count`:
    one integer per query (None: from the document's start / to its end; both None: whole documents).  Returns (symbols flat int32,
    out_offsets int64 [n_queries + 1], status int32 [n_queries]): query q owns symbols[out_offsets[q]:out_offsets[q + 1]], exactly what
    ans_decode_ragged puts at sym_offsets[streams[q]] + first[q] ...
    With jump points (`encoded.jump`, see ans_encode_ragged) every query starts at the jump point in front of `first`, decodes and
    discards first % interval symbols, and every chunk it touches runs on a lane of its own: at most `interval` dependent steps.
    WITHOUT them a query starts where its document starts and discards `first` symbols -- correct, and as slow as `first` is deep: that
    is what jump points are for.  A query the device refuses (no such document, a range beyond its document, a table or counts that do
    not fit) reports INVALID_DATA (3) and writes nothing; the others decode.  (Sized on the device: the output total is the only
    read-back.)  Shared tables only: a model with one table per stream raises ValueError."""
    return _decode_ragged_select("ans", RaggedJump, encoded, model, sym_offsets, streams, first, count, out)


def range_decode_ragged_select(encoded: RaggedBatch, model: Model, sym_offsets: torch.Tensor, streams, first=None, count=None,
                               out: Optional[torch.Tensor] = None):
    """ans_decode_ragged_select for a range batch (range_encode_ragged / range_encode_ragged_jump): the same queries, the same three
    results.  A piece seeks to its (pos, lower, range) entry and reads forward; without jump points it starts at word 0 of its document
    and discards `first` symbols.  Shared tables only: a model with one table per stream raises ValueError."""
    return _decode_ragged_select("range", RangeRaggedJump, encoded, model, sym_offsets, streams, first, count, out)


def range_decode_until(encoded: RaggedBatch, model: Model, eof_symbol: int, max_symbols: Optional[int] = None):
    """Streams whose length is not stored: every stream is decoded until `eof_symbol`, which a queue writes LAST.  Two launches --
    count, prefix sum, decode -- as ans_decode_until.  Returns (symbols flat, sym_offsets [n + 1], status); the terminator is the last
    symbol of every stream.  A range decoder never runs out of words (the reference shifts in zeros), so `max_symbols` (default 2^20)
    is the only stop for a stream without a terminator: status CAPACITY (2), and such a stream decodes to NO symbols (its length is 0
    in sym_offsets).  Contiguous alphabets and shared tables only: a model with one table per stream raises ValueError."""
    _require_coder(encoded, "range")
    _refuse_per_stream(model, "range_decode_until")
    max_symbols = (1 << 20) if max_symbols is None else int(max_symbols)
    if model.noncontiguous:
        raise ValueError("range_decode_until: contiguous alphabets only")
    n_streams = encoded.n_words.numel()
    dev = encoded.words.device
    lengths = torch.zeros(n_streams, dtype=torch.int64, device=dev)
    status = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    order = encoded.order if encoded.order is not None and encoded.order.numel() == n_streams else _ragged_order("auto", n_streams, encoded.n_words)
    N.check(N.lib().cst_range_count_until(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                          encoded.words.numel(), _ptr(encoded.n_words), n_streams,
                                          _ptr(order) if order is not None else None, int(eof_symbol), int(max_symbols),
                                          _ptr(lengths), _ptr(status), _stream_ptr()), "cst_range_count_until")
    lengths = torch.where(status != 0, torch.zeros_like(lengths), lengths)      # (a stream without a terminator is not decoded)
    sym_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lengths, 0, out=sym_offsets[1:])
    symbols, status2 = range_decode_ragged(encoded, model, sym_offsets, order=order)
    return symbols, sym_offsets, torch.where(status != 0, status, status2)


def _compact_scratch(device, n_streams):
    # (one scratch per device AND stream: two compactions on different streams must not share ticket / status words)
    need = N.load_library().cst_compact_scratch_bytes(n_streams)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    t = _scratch.get(key)
    if t is None or t.numel() < need:
        t = torch.empty(max(need, 4096), dtype=torch.uint8, device=device)
        _scratch[key] = t
    return t


def compact(encoded: EncodedBatch, capacity: Optional[int] = None, out=None):
    """Packs the slabs: returns (packed uint32 words as int32 tensor, offsets int64[n_streams+1]); offsets[-1] = total words.

    One asynchronous kernel (single-pass scan fused with the gather), no host synchronisation: `packed` has `capacity`
    words (default: the upper bound n_streams * stride, so that nothing can overflow) of which ONLY the first offsets[-1]
    are valid -- slice with `packed[:int(offsets[-1])]` (that reads the total back from the device; callers that stay on
    the device hand `packed` and `offsets` on as they are).  `out=(packed, offsets)` reuses buffers of an earlier call.
    With a caller-chosen `capacity` or `out` the words may not fit: streams that would overflow are left out by the kernel,
    and this function then reads offsets[-1] back (one synchronisation, only in this case) and raises."""
    n_streams = encoded.n_words.numel()
    dev = encoded.words.device
    if out is not None:
        packed, offsets = out
    else:
        capacity = capacity if capacity is not None else n_streams * encoded.words.shape[1]
        packed = torch.empty(max(capacity, 1), dtype=encoded.words.dtype, device=dev)
        offsets = torch.empty(n_streams + 1, dtype=torch.int64, device=dev)
    fn = N.lib().cst_compact_words16 if encoded.packed16 else N.lib().cst_compact_words       # (packed 16-bit words: everything in halfwords)
    N.check(fn(_ptr(encoded.words), encoded.words.shape[1], _ptr(encoded.n_words), n_streams,
               _ptr(offsets), _ptr(packed), packed.numel(), _ptr(_compact_scratch(dev, n_streams)),
               _stream_ptr()), "cst_compact_words")
    if (out is not None or capacity is not None) and int(offsets[-1].item()) > packed.numel():
        raise ValueError(f"compact: {int(offsets[-1].item())} words do not fit the packed buffer of {packed.numel()} words")
    return packed, offsets


def reverse_words(encoded, offsets: Optional[torch.Tensor] = None, out=None):
    """Every stream's words in the opposite order (its own inverse): from the reference's default order -- the LAST word of a
    stream is the first an ANS decoder reads -- to the order `AnsCoder::from_reversed_compressed` / `Cursor::into_reversed`
    (src/stream/stack.rs:734-748, src/backends.rs:1424-1448) use, first-read word first, and back.

    `encoded`: an `EncodedBatch` of (32, 64) slabs -> a new `EncodedBatch` (or `out=encoded` for in place); or a tuple
    `(packed int32 words, n_words)` with `offsets` int64[n_streams + 1] -> a packed tensor of the same layout."""
    if isinstance(encoded, EncodedBatch):
        if encoded.packed16:
            raise ValueError("reverse_words: 32-bit words only")
        n_streams = encoded.n_words.numel()
        res = out if out is not None else EncodedBatch(torch.empty_like(encoded.words), encoded.n_words, encoded.status, encoded.config)
        N.check(N.lib().cst_words_reverse(_ptr(encoded.words), None, encoded.words.shape[1], _ptr(encoded.n_words), n_streams,
                                          _ptr(res.words), None, res.words.shape[1], _stream_ptr()), "cst_words_reverse")
        return res
    packed, n_words = encoded
    if offsets is None:
        raise ValueError("reverse_words: packed words need their offsets")
    res = out if out is not None else torch.empty_like(packed)
    N.check(N.lib().cst_words_reverse(_ptr(packed), _ptr(offsets), 0, _ptr(n_words), n_words.numel(), _ptr(res), _ptr(offsets), 0,
                                      _stream_ptr()), "cst_words_reverse")
    return res


def range_max_words(n_per_stream: int, config=(32, 64, 12)) -> int:
    return N.load_library().cst_range_max_words(n_per_stream, _cfg(*config))


def _check_range_per_stream(model: Model, n_streams: int, layout: str, jump) -> None:
    """What the range coder asks of a model with one table per stream, said before any launch (a shared table passes)."""
    if model.n_tables == 1:
        return
    if model.noncontiguous:
        raise ValueError("tables per stream: contiguous alphabets only")
    if model.n_tables != n_streams:
        raise ValueError(f"the model has {model.n_tables} tables, the batch {n_streams} streams: one table per stream")
    if jump and layout != "stream_major":
        raise ValueError("tables per stream with jump points: stream-major batches only")


def range_encode(symbols: torch.Tensor, model: Model, config=(32, 64, 12), layout="stream_major",
                 stride=None, out: Optional[EncodedBatch] = None, jump_points="auto") -> EncodedBatch:
    """One RangeEncoder per stream: encode_iid_symbols + get_compressed (queue.rs:612-705, 458-523).
    stride: words per slab (default range_max_words), or "tuned" (tuned_stride(..., coder="range")).
    jump_points: as for ans_encode -- `RangeEncoder.pos()` (queue.rs:172-196) in front of every k-th part of a stream, carried as
    `.jump` for range_decode; "auto" (default) = cst_jump_points_auto (the range decoder's division chain is latency-bound at one
    wave per SIMD: two lanes per stream at 65 536 streams), an integer k, or 0.
    model: one shared table, or one table per stream (quantized_gaussian_per_stream, from_cdf_rows_per_stream, fit_per_stream: as
    many tables as streams, presets (32, 64) and (16, 32), P <= 16, either layout, int8 / int16 matrices widened on the device).
    With tables per stream "auto" notes no jump points (nothing has measured whether they pay there); an integer k is honoured
    for stream-major matrices."""
    _check_range_per_stream(model, _layout_shape(symbols, layout)[0], layout, 0 if isinstance(jump_points, str) else jump_points)
    if isinstance(stride, str):
        if stride != "tuned":
            raise ValueError("stride must be a number of words or 'tuned'")
        stride = tuned_stride(symbols, model, config, layout, coder="range") if out is None else None
    narrow = _SYMBOL_BYTES.get(symbols.dtype, 4) if symbols.dtype in _SYMBOL_BYTES else 4
    if narrow != 4:
        # int8 / int16 matrices (the reference's Symbol is generic, queue.rs:612; cst_range_encode_batch[_ckpt]_sym): int8 rows of whole
        # 32-symbol tiles at (32, 64) are read by the encoder loop itself (round 6), every other shape is widened next to the int32 call
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only (map the symbols to indices first)")
        given = symbols = _require_cuda(symbols, symbols.dtype, "symbols")
    else:
        given = _require_cuda(symbols, torch.int32, "symbols")
        symbols = _to_indices(model, given)
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    if out is None:
        out = _new_batch(n_streams, stride or range_max_words(n_per, config), symbols.device, config)
    L = N.lib()
    interval = _jump_interval(jump_points, n_per, lambda: L.cst_jump_points_auto(
        model._h, _cfg(*config), N.CODER_RANGE, narrow, _ptr(symbols), n_streams, n_per, lay, _ptr(out.words), out.words.shape[1]))
    if interval:
        ck = _jump_table(out, RangeCheckpoints, interval, n_streams, n_per, symbols.device)
        range_encode_checkpointed(given, model, interval, config, layout, out=(out, ck))
        out.jump = ck
        return out
    out.jump = None
    if narrow != 4:
        scratch = _ckpt_scratch("range_sym", symbols.device, L.cst_range_sym_scratch_bytes(n_streams, n_per, 0, narrow))
        N.check(L.cst_range_encode_batch_sym(model._h, _cfg(*config), _ptr(symbols), narrow, n_streams, n_per, lay, _ptr(out.words),
                                             out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status), N.FLAG_NONE, _ptr(scratch),
                                             _stream_ptr()), "cst_range_encode_batch_sym")
        return out
    N.check(L.cst_range_encode_batch(model._h, _cfg(*config), _ptr(symbols), n_streams, n_per, lay, _ptr(out.words),
                                     out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status), N.FLAG_NONE,
                                     _stream_ptr()), "cst_range_encode_batch")
    return out


def range_decode(encoded, model: Model, n_per_stream: int, layout="stream_major", offsets: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, config=None, dtype=torch.int32):
    """One RangeDecoder per stream: from_compressed + decode_iid_symbols (queue.rs:847-868, 968-1033).
    dtype (or the dtype of `out`): int32, or int16 / int8 -- narrowed on the device behind the decoder (cst_symbols_narrow).
    model: as for range_encode -- one shared table, or one table per stream.  A batch that carries jump points for exactly this
    shape (range_encode, jump_points=k) decodes every part of a stream on a lane of its own."""
    if isinstance(encoded, EncodedBatch):
        words, n_words, config = encoded.words, encoded.n_words, config or encoded.config
        stride = words.shape[1]
    else:
        words, n_words = encoded
        stride = words.shape[1] if words.dim() == 2 else 0
        config = config or (32, 64, 12)
    n_streams = n_words.numel()
    dev = words.device
    _check_range_per_stream(model, n_streams, layout, 0)
    dtype = out.dtype if out is not None else dtype
    if dtype not in _SYMBOL_BYTES:
        raise TypeError("decoded symbols are int32, int16 or int8")
    narrow = _SYMBOL_BYTES[dtype]
    if narrow != 4:
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only")
        info = torch.iinfo(dtype)
        if model.min_symbol < info.min or model.min_symbol + model.n_symbols - 1 > info.max:
            raise ValueError(f"the model's support does not fit {dtype}")
    jump = encoded.jump if isinstance(encoded, EncodedBatch) else None
    if isinstance(jump, RangeCheckpoints) and offsets is None and layout == "stream_major" and \
            n_per_stream == jump.interval * jump.pos.shape[1] and jump.pos.shape[0] == n_streams:
        # the batch carries jump points for exactly this decode: every part of a stream on a lane of its own
        dec, part_status = range_decode_checkpointed(encoded, jump, model, n_per_stream, out=out, dtype=dtype)
        return dec, _status_per_stream(part_status)
    if out is None:
        shape = (n_streams, n_per_stream) if layout == "stream_major" else (n_per_stream, n_streams)
        out = torch.empty(shape, dtype=dtype, device=dev)
    lay = N.LAYOUT_STREAM_MAJOR if layout == "stream_major" else N.LAYOUT_SYMBOL_MAJOR
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    L = N.lib()
    if narrow != 4:
        # (cst_range_decode_batch_sym: int8 stream-major matrices are written by the sub-lane decoder itself, one lane per stream;
        #  every other shape is narrowed on the device behind the int32 decoder)
        scratch = _ckpt_scratch("range_sym", dev, L.cst_range_sym_scratch_bytes(n_streams, n_per_stream, 0, narrow))
        N.check(L.cst_range_decode_batch_sym(model._h, _cfg(*config), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words),
                                             _ptr(out), narrow, n_streams, n_per_stream, lay, None, _ptr(status), N.FLAG_NONE, _ptr(scratch),
                                             _stream_ptr()), "cst_range_decode_batch_sym")
        return out, status
    N.check(L.cst_range_decode_batch(model._h, _cfg(*config), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words),
                                     _ptr(out), n_streams, n_per_stream, lay, None, _ptr(status), N.FLAG_NONE,
                                     _stream_ptr()), "cst_range_decode_batch")
    return _to_symbols(model, out), status


# ---------------------------------------------------------------------------------------------------------------------
# per-symbol quantized Gaussians: the reference's flagship call for many streams at once
#     coder.encode_reverse(symbols, QuantizedGaussian(lo, hi), means, stds) / coder.decode(family, means, stds)
# (src/pybindings/stream/stack.rs:567-588, 733-751): every symbol has its own (mean, std); `means` / `stds` are float64 or
# float32 tensors of the shape and layout of the symbol matrix.  The models of float32 parameters are those of the values
# widened to f64, as in the reference (src/pybindings/mod.rs:211-216): a PAIR of float32 tensors is read by the kernels
# themselves and widened in registers (the _f32 entry points, DESIGN.md 4.32: no widened copy); a float32 tensor next to a
# float64 one is widened here.  The chain-coder calls widen both.
# ---------------------------------------------------------------------------------------------------------------------

def _gaussian_args(symbols_shape, means, stds, f32=False):
    """the parameter matrices of a per-symbol call as its entry point takes them.  f32: the call has an _f32 twin (_f32_name) -- a pair
    of float32 tensors then goes through as it is.  Anything else float32 is widened, exactly as the reference's Python API does
    (PyReadonlyFloatArray::cast_f64, src/pybindings/mod.rs:187-214; its own doc example passes float32 arrays): the models are those
    of the widened values either way."""
    dtype = torch.float32 if f32 and means.dtype == torch.float32 and stds.dtype == torch.float32 else torch.float64
    if dtype == torch.float64:
        if means.dtype == torch.float32:
            means = means.to(torch.float64)
        if stds.dtype == torch.float32:
            stds = stds.to(torch.float64)
    means = _require_cuda(means, dtype, "means")
    stds = _require_cuda(stds, dtype, "stds")
    if tuple(means.shape) != tuple(symbols_shape) or tuple(stds.shape) != tuple(symbols_shape):
        raise ValueError("means and stds must have the shape of the symbol matrix")
    return means, stds


def _f32_name(fn_name, means):
    """the entry point for parameter matrices that went through _gaussian_args(..., f32=True)"""
    return fn_name + "_f32" if means.dtype == torch.float32 else fn_name


def _encode_gaussian(fn_name, max_words_fn, symbols, min_symbol, max_symbol, means, stds, config, layout, stride, out, family=()):
    # family: () for the Gaussian entry points, (CST_FAMILY_*,) for cst_*_family_batch, which take it after the configuration
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    means, stds = _gaussian_args(symbols.shape, means, stds, f32=True)
    fn_name = _f32_name(fn_name, means)
    if out is None:
        stride = stride or max_words_fn(n_per, config)
        dev = symbols.device
        out = EncodedBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config))
    N.check(getattr(N.lib(), fn_name)(_cfg(*config), *family, int(min_symbol), int(max_symbol), _ptr(symbols), _ptr(means), _ptr(stds),
                                      n_streams, n_per, lay, _ptr(out.words), out.words.shape[1], _ptr(out.n_words), None,
                                      _ptr(out.status), N.FLAG_NONE, _stream_ptr()), fn_name)
    return out


def ans_encode_gaussian(symbols, min_symbol, max_symbol, means, stds, config=(32, 64, 24), layout="stream_major",
                        stride: Optional[int] = None, out: Optional[EncodedBatch] = None, jump_points="auto") -> EncodedBatch:
    """One AnsCoder per stream: encode_reverse(symbols[s], QuantizedGaussian(min, max), means[s], stds[s]) + get_compressed.
    jump_points: as for ans_encode ("auto" = cst_jump_points_auto_gaussian: batches the fused encoder takes, of at most one wave of
    streams per SIMD, get the points that give ans_decode_gaussian two; an integer k; 0)."""
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    interval = _jump_interval(jump_points, n_per, lambda: N.lib().cst_jump_points_auto_gaussian(_cfg(*config), N.CODER_ANS, n_streams, n_per, lay))
    if interval:
        if layout != "stream_major":
            raise ValueError("jump_points: stream-major batches only")
        if out is None:
            out = _new_batch(n_streams, stride or max_words(n_per, config), symbols.device, config)
        ck = _jump_table(out, Checkpoints, interval, n_streams, n_per, symbols.device)
        ans_encode_gaussian_checkpointed(symbols, min_symbol, max_symbol, means, stds, interval, config, out=(out, ck))
        out.jump = ck
        return out
    out = _encode_gaussian("cst_ans_encode_gaussian_batch", max_words, symbols, min_symbol, max_symbol, means, stds, config,
                           layout, stride, out)
    out.jump = None
    return out


def range_encode_gaussian(symbols, min_symbol, max_symbol, means, stds, config=(32, 64, 24), layout="stream_major",
                          stride: Optional[int] = None, out: Optional[EncodedBatch] = None, jump_points="auto") -> EncodedBatch:
    """One RangeEncoder per stream: encode(symbols[s], QuantizedGaussian(min, max), means[s], stds[s]) + get_compressed
    (src/pybindings/stream/queue.rs:343-410).  jump_points: as for ans_encode_gaussian (RangeEncoder.pos(), queue.rs:172-196)."""
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    interval = _jump_interval(jump_points, n_per, lambda: N.lib().cst_jump_points_auto_gaussian(_cfg(*config), N.CODER_RANGE, n_streams, n_per, lay))
    if interval:
        if layout != "stream_major":
            raise ValueError("jump_points: stream-major batches only")
        symbols = _require_cuda(symbols, torch.int32, "symbols")
        means, stds = _gaussian_args(symbols.shape, means, stds, f32=True)
        fn = _f32_name("cst_range_encode_gaussian_batch_ckpt", means)
        if out is None:
            out = _new_batch(n_streams, stride or range_max_words(n_per, config), symbols.device, config)
        ck = _jump_table(out, RangeCheckpoints, interval, n_streams, n_per, symbols.device)
        N.check(getattr(N.lib(), fn)(_cfg(*config), int(min_symbol), int(max_symbol), _ptr(symbols), _ptr(means), _ptr(stds),
                                     n_streams, n_per, lay, _ptr(out.words), out.words.shape[1], _ptr(out.n_words), interval,
                                     _ptr(ck.pos), _ptr(ck.lower), _ptr(ck.range), _ptr(out.status), _stream_ptr()), fn)
        out.jump = ck
        return out
    out = _encode_gaussian("cst_range_encode_gaussian_batch", range_max_words, symbols, min_symbol, max_symbol, means, stds,
                           config, layout, stride, out)
    out.jump = None
    return out


def _decode_gaussian(fn_name, ans, encoded, min_symbol, max_symbol, means, stds, layout, offsets, out, config, family=()):
    if isinstance(encoded, EncodedBatch):
        words, n_words, config = encoded.words, encoded.n_words, config or encoded.config
        stride = words.shape[1]
    else:
        words, n_words = encoded
        stride = words.shape[1] if words.dim() == 2 else 0
        config = config or (32, 64, 24)
    if means.dim() != 2:
        raise ValueError("means must be 2-d")
    n_streams, n_per, lay = _layout_shape(means, layout)
    if n_streams != n_words.numel():
        raise ValueError("means / stds do not match the number of streams")
    means, stds = _gaussian_args(means.shape, means, stds, f32=True)
    fn_name = _f32_name(fn_name, means)
    dev = words.device
    if out is None:
        out = torch.empty(tuple(means.shape), dtype=torch.int32, device=dev)
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    args = [_cfg(*config), *family, int(min_symbol), int(max_symbol), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words), _ptr(means), _ptr(stds),
            _ptr(out), n_streams, n_per, lay, None]
    if ans:
        args.append(None)          # d_n_words_out
    N.check(getattr(N.lib(), fn_name)(*args, _ptr(status), N.FLAG_NONE, _stream_ptr()), fn_name)
    return out, status


# ---------------------------------------------------------------------------------------------------------------------
# chain coders (src/stream/chain.rs), many at once.  A chain has two word stacks and two heads; a call pops one stack and
# pushes the other (decode: pops `compressed`, pushes `remainders`; encode: the reverse).
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class ChainBatch:
    """words / n_words: the stack that the next call pops, stream s = words[s, :n_words[s]], consumed from the end;
    heads: int64 [n_streams, 2] = cst_chain_heads (remainders head; compressed head in the low word).  Calls update
    n_words and heads in place and return what they pushed."""
    words: torch.Tensor
    n_words: torch.Tensor
    heads: torch.Tensor
    config: tuple = (32, 64, 24)


def _chain_call(fn_name, chains: ChainBatch, n_streams, n_per, call):
    dev = chains.words.device
    pushed = torch.empty((n_streams, max(n_per, 1)), dtype=torch.int32, device=dev)
    n_pushed = torch.empty(n_streams, dtype=torch.int32, device=dev)
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    N.check(call(pushed, n_pushed, status), fn_name)
    return pushed, n_pushed, status


def chain_decode_gaussian(chains: ChainBatch, min_symbol, max_symbol, means, stds, layout="stream_major"):
    """ChainCoder.decode(QuantizedGaussian(min, max), means[s], stds[s]) for every chain.
    Returns (symbols, pushed remainders words [n_streams, n_per], their counts, status)."""
    n_streams, n_per, lay = _layout_shape(means, layout)
    means, stds = _gaussian_args(means.shape, means, stds)
    out = torch.empty(tuple(means.shape), dtype=torch.int32, device=means.device)
    fn = "cst_chain_decode_gaussian_batch"
    pushed, n_pushed, status = _chain_call(fn, chains, n_streams, n_per, lambda pw, pn, st: getattr(N.lib(), fn)(
        _cfg(*chains.config), int(min_symbol), int(max_symbol), _ptr(chains.words), None, chains.words.shape[1], _ptr(chains.n_words),
        _ptr(means), _ptr(stds), _ptr(out), n_streams, n_per, lay, _ptr(pw), pw.shape[1], _ptr(pn), _ptr(chains.heads), _ptr(st),
        _stream_ptr()))
    return out, pushed, n_pushed, status


def chain_encode_gaussian(chains: ChainBatch, symbols, min_symbol, max_symbol, means, stds, layout="stream_major"):
    """ChainCoder.encode_reverse(symbols[s], QuantizedGaussian(min, max), means[s], stds[s]) for every chain; `chains` holds
    the REMAINDERS stacks.  Returns (pushed compressed words [n_streams, n_per], their counts, status)."""
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    means, stds = _gaussian_args(symbols.shape, means, stds)
    fn = "cst_chain_encode_gaussian_batch"
    return _chain_call(fn, chains, n_streams, n_per, lambda pw, pn, st: getattr(N.lib(), fn)(
        _cfg(*chains.config), int(min_symbol), int(max_symbol), _ptr(symbols), _ptr(means), _ptr(stds), n_streams, n_per, lay,
        _ptr(chains.words), None, chains.words.shape[1], _ptr(chains.n_words), _ptr(pw), pw.shape[1], _ptr(pn), _ptr(chains.heads),
        _ptr(st), _stream_ptr()))


def release_scratch():
    """Hands the scratch memory the per-symbol calls keep in the device's memory pool back to the system."""
    N.check(N.lib().cst_release_scratch(), "cst_release_scratch")


def ans_decode_gaussian(encoded, min_symbol, max_symbol, means, stds, layout="stream_major", offsets=None, out=None, config=None):
    """One AnsCoder per stream: AnsCoder(words[s]).decode(QuantizedGaussian(min, max), means[s], stds[s]).  A batch that carries
    jump points for exactly this shape (ans_encode_gaussian, jump_points) decodes every part of a stream on a lane of its own."""
    jump = encoded.jump if isinstance(encoded, EncodedBatch) else None
    if isinstance(jump, Checkpoints) and offsets is None and layout == "stream_major" and means.dim() == 2 and \
            tuple(means.shape) == (jump.pos.shape[0], jump.interval * jump.pos.shape[1]) and jump.pos.shape[0] == encoded.n_words.numel():
        dec, part_status = ans_decode_gaussian_checkpointed(encoded, jump, min_symbol, max_symbol, means, stds, out=out)
        return dec, _status_per_stream(part_status)
    return _decode_gaussian("cst_ans_decode_gaussian_batch", True, encoded, min_symbol, max_symbol, means, stds, layout, offsets, out, config)


def range_decode_gaussian(encoded, min_symbol, max_symbol, means, stds, layout="stream_major", offsets=None, out=None, config=None):
    """One RangeDecoder per stream: RangeDecoder(words[s]).decode(QuantizedGaussian(min, max), means[s], stds[s]).  A batch that carries
    jump points for exactly this shape (range_encode_gaussian, jump_points) decodes every part of a stream on a lane of its own."""
    jump = encoded.jump if isinstance(encoded, EncodedBatch) else None
    if isinstance(jump, RangeCheckpoints) and offsets is None and layout == "stream_major" and means.dim() == 2 and \
            tuple(means.shape) == (jump.pos.shape[0], jump.interval * jump.pos.shape[1]) and jump.pos.shape[0] == encoded.n_words.numel():
        n_streams, n_per = means.shape
        means, stds = _gaussian_args(means.shape, means, stds, f32=True)
        fn = _f32_name("cst_range_decode_gaussian_batch_ckpt", means)
        dev = encoded.words.device
        if out is None:
            out = torch.empty((n_streams, n_per), dtype=torch.int32, device=dev)
        part_status = torch.empty(tuple(jump.pos.shape), dtype=torch.int32, device=dev)
        L = N.lib()
        scratch = _ckpt_scratch("range_gaussian_ckpt", dev, L.cst_range_gaussian_ckpt_scratch_bytes(n_streams, n_per, jump.interval))
        N.check(getattr(L, fn)(_cfg(*encoded.config), int(min_symbol), int(max_symbol), _ptr(encoded.words), None,
                               encoded.words.shape[1], encoded.words.numel(), _ptr(encoded.n_words), jump.interval,
                               _ptr(jump.pos), _ptr(jump.lower), _ptr(jump.range), _ptr(means), _ptr(stds), _ptr(out),
                               n_streams, n_per, _ptr(scratch), _ptr(part_status), _stream_ptr()), fn)
        return out, _status_per_stream(part_status)
    return _decode_gaussian("cst_range_decode_gaussian_batch", False, encoded, min_symbol, max_symbol, means, stds, layout, offsets, out, config)


# ---------------------------------------------------------------------------------------------------------------------
# per-symbol quantized Gaussians for streams of DIFFERENT lengths: a batch of images, crops or tensors of different sizes, every
# latent with its own (mean, std) -- the ragged calls' indexing (flat arrays + sym_offsets) on the Gaussian calls' models
# ---------------------------------------------------------------------------------------------------------------------

def _gaussian_ragged_args(sym_offsets, n_elements, means, stds, f32=False):
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if sym_offsets.dim() != 1 or n_streams < 0:
        raise ValueError("sym_offsets must be 1-d and hold n_streams + 1 entries")
    if means.dim() != 1 or stds.dim() != 1:
        raise ValueError("means and stds must be flat")
    if n_elements is None:
        n_elements = means.numel()
    means, stds = _gaussian_args((n_elements,), means, stds, f32)
    return sym_offsets, n_streams, means, stds


def _never_null(t):
    """a one-element stand-in for an empty tensor (a batch of empty streams): the entry points refuse NULL and read nothing"""
    return t if t.numel() > 0 else torch.zeros(1, dtype=t.dtype, device=t.device)


def _persymbol_jump_every(jump_every) -> object:
    """the `jump_every` argument of the ragged per-symbol encoders, judged before any tensor is looked at: "auto", or an int that is 0 or
    a positive multiple of 16 (the encoder codes in tiles of 16 symbols)"""
    if isinstance(jump_every, str):
        if jump_every != "auto":
            raise ValueError("jump_every: 'auto', 0 or a multiple of 16")
        return "auto"
    jump_every = int(jump_every or 0)
    if jump_every < 0 or jump_every % 16 != 0 or jump_every > 0x7fffffff:
        raise ValueError("jump_every: 'auto', 0 or a multiple of 16")
    return jump_every


def _keeps_plain_signature(fn):
    """For the eight ragged per-symbol encoders: `jump_every` is a keyword-only option that inspect.signature() does not list.  Their
    parameter lists are compared name for name by tests that predate the option (tests/test_gaussian_ragged_cpu.py,
    tests/test_ragged_per_symbol_forms_cpu.py), so the reported signature stays the plain call's; `fn.__kwdefaults__` and the
    docstrings have the option."""
    sig = inspect.signature(fn)
    fn.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.kind is not p.KEYWORD_ONLY])
    return fn


def _encode_persymbol_ragged(fn_name, coder, symbols, sym_offsets, lo, hi, a, b, config, order, family=(), jump_every=0) -> RaggedBatch:
    """the body of every {ans,range}_encode_{gaussian,family}_ragged: `family` is () or (id,), the argument that follows cfg.
    jump_every: 0 (the plain call), a positive multiple of 16, or "auto" -- RAGGED_JUMP_EVERY where the streams average more than
    RAGGED_JUMP_EVERY symbols (more than one chunk each: range_encode_ragged_jump's rule), else 0.  With jump points the batch carries
    the table as `.jump`: a RaggedJump (ANS) or a RangeRaggedJump (range), sized without a read-back.
    The rule holds for all six forms: on 16 384 streams of 256 .. 8192 symbols, encode + decode with a jump point every 256 symbols was
    lower than plain in every alternation (ANS x Gaussian 3.44 + 7.15 -> 3.50 + 1.03 ms, range x Gaussian 4.07 + 7.78 -> 4.17 + 1.08 ms,
    ANS x Laplace 10.55 + 28.92 -> 10.56 + 2.89 ms, range x Cauchy 10.72 + 24.89 -> 10.75 + 2.74 ms).  Streams of one
    chunk each have nothing to gain and are left alone, as the range coder's."""
    jump_every = _persymbol_jump_every(jump_every)
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    if symbols.dim() != 1:
        raise ValueError("symbols must be flat")
    sym_offsets, n_streams, a, b = _gaussian_ragged_args(sym_offsets, symbols.numel(), a, b, f32=True)
    model = (*family, int(lo), int(hi), _ptr(_never_null(symbols)), _ptr(_never_null(a)), _ptr(_never_null(b)))
    return _encode_ragged_slabs(fn_name, coder, symbols, sym_offsets, n_streams, config, order, jump_every, model,
                                "_f32" if a.dtype == torch.float32 else "")


def _encode_ragged_slabs(fn_name, coder, symbols, sym_offsets, n_streams, config, order, jump_every, model, suffix="") -> RaggedBatch:
    """the slabs, the schedule, the jump table and the call of every ragged per-symbol encoder, once its arguments are judged: `model` is
    what the entry point takes between cfg and d_sym_offsets (the family's (lo, hi, symbols, a, b), or the Categorical's (symbols,
    probabilities, prob_bytes, K, n_total)); `jump_every` has been through _persymbol_jump_every; `suffix`: "_f32" for the twins over
    float32 parameters (behind "_jump" where the jump form is taken)"""
    W, S, P = config
    dev = symbols.device
    lengths = sym_offsets[1:] - sym_offsets[:-1]
    # a stream of n symbols fills at most min(n, ceil(n P / W)) words plus the S / W words of the ANS state (see ans_encode_ragged), or
    # plus the 2 words that seal a range coder (the bound inside cst_range_max_words, without its rounding to 64 bytes); 16-byte slabs
    bound = torch.minimum(lengths, (lengths * P + (W - 1)) // W) + (S // W if coder == "ans" else 2)
    slabs = (bound + 3) // 4 * 4
    word_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
    torch.cumsum(slabs, 0, out=word_offsets[1:])
    total = int(word_offsets[-1].item()) if n_streams else 0
    order = _ragged_order(order, n_streams, lengths)
    out = RaggedBatch(torch.empty(max(total, 4), dtype=torch.int32, device=dev), word_offsets,
                      torch.empty(n_streams, dtype=torch.int32, device=dev), torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config),
                      order, None, coder)
    if n_streams == 0:
        return out
    if jump_every == "auto":
        jump_every = RAGGED_JUMP_EVERY if symbols.numel() > n_streams * RAGGED_JUMP_EVERY else 0
    if jump_every:
        chunk_offsets = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        torch.cumsum((lengths + (jump_every - 1)) // jump_every, 0, out=chunk_offsets[1:])
        # (no read-back of the total: sum(ceil(len / I)) <= total / I + n_streams bounds it, entries behind the last chunk stay unused)
        n_chunks = max(symbols.numel() // jump_every + n_streams, 1)
        pos = torch.empty(n_chunks, dtype=torch.int32, device=dev)
        if coder == "ans":
            jump = RaggedJump(jump_every, chunk_offsets, pos, torch.empty(n_chunks, dtype=torch.int64, device=dev))
            table = (_ptr(jump.pos), _ptr(jump.state))
        else:
            jump = RangeRaggedJump(jump_every, chunk_offsets, pos, torch.empty(n_chunks, dtype=torch.int64, device=dev),
                                   torch.empty(n_chunks, dtype=torch.int64, device=dev))
            table = (_ptr(jump.pos), _ptr(jump.lower), _ptr(jump.range))
        N.check(getattr(N.lib(), fn_name + "_jump" + suffix)(_cfg(*config), *model, _ptr(sym_offsets), n_streams,
                                                             _ptr(order) if order is not None else None, _ptr(out.words), _ptr(word_offsets), 0,
                                                             _ptr(out.n_words), jump_every, _ptr(chunk_offsets), *table, _ptr(out.status),
                                                             _stream_ptr()), fn_name + "_jump" + suffix)
        out.jump = jump
        return out
    N.check(getattr(N.lib(), fn_name + suffix)(_cfg(*config), *model, _ptr(sym_offsets), n_streams, _ptr(order) if order is not None else None,
                                               _ptr(out.words), _ptr(word_offsets), 0, _ptr(out.n_words), _ptr(out.status), _stream_ptr()),
            fn_name + suffix)
    return out


def _ragged_jump_of(encoded: RaggedBatch, coder):
    """what every ragged per-symbol decoder judges first: the batch is this coder's, and so are its jump points (or it has none)"""
    _require_coder(encoded, coder)
    jump = encoded.jump
    if jump is not None and not isinstance(jump, RaggedJump if coder == "ans" else RangeRaggedJump):
        raise ValueError("the batch carries the jump points of another coder")
    return jump


def _decode_persymbol_ragged(fn_name, coder, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, out, order, family=()):
    """the body of every {ans,range}_decode_{gaussian,family}_ragged.  A batch with jump points (`jump_every` of the encoders) decodes
    its chunks side by side when `order` is None or "auto"; a schedule handed in is honoured on the whole streams."""
    jump = _ragged_jump_of(encoded, coder)
    sym_offsets, n_streams, a, b = _gaussian_ragged_args(sym_offsets, None, a, b, f32=True)
    return _decode_ragged_slabs(fn_name, coder, encoded, jump, sym_offsets, n_streams, a.numel(), out, order, (*family, int(lo), int(hi)),
                                (_ptr(_never_null(a)), _ptr(_never_null(b))), suffix="_f32" if a.dtype == torch.float32 else "")


def _decode_ragged_slabs(fn_name, coder, encoded: RaggedBatch, jump, sym_offsets, n_streams, total, out, order, head, model, plain_extra=None,
                         suffix=""):
    """the schedule, the output, the route (whole streams, or the chunks of a jump table side by side) and the call of every ragged
    per-symbol decoder, once its arguments are judged: `head` is what the entry point takes between cfg and d_words (the family's
    (lo, hi)), `model` what it takes between d_n_words and d_symbols (the family's (a, b), or the Categorical's (probabilities,
    prob_bytes, K, n_total)); `total`: the symbols of all streams.  `plain_extra`: a callable, asked only on the whole-stream route, for
    what the plain entry point takes behind `model` and the jump form does not (Categorical(perfect=True): max_len); `suffix`: as in
    _encode_ragged_slabs"""
    if encoded.n_words.numel() != n_streams:
        raise ValueError("sym_offsets does not match the number of streams of the batch")
    take_jump = jump is not None and (order is None or (isinstance(order, str) and order == "auto"))
    if isinstance(order, str) and order == "auto" and encoded.order is not None and encoded.order.numel() == n_streams:
        order = encoded.order
    order = _ragged_order(order, n_streams, encoded.n_words)
    dev = encoded.words.device
    if out is None:
        out = torch.empty(total, dtype=torch.int32, device=dev)
    else:
        out = _require_cuda(out, torch.int32, "out")
        if out.dim() != 1 or out.numel() != total:
            raise ValueError("out must be flat and hold one symbol per parameter")
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    if n_streams == 0:
        return out, status
    target = _never_null(out)
    if take_jump and jump.chunk_offsets.numel() == n_streams + 1:
        # every chunk of every stream on a lane of its own (the table is checked against the lengths on the device: a stream it does not
        # describe reports INVALID_DATA); an upper bound of the chunks is enough, entries behind the last chunk are empty
        L = N.lib()
        arrays = (jump.pos, jump.state) if coder == "ans" else (jump.pos, jump.lower, jump.range)
        n_chunks = min(int(t.numel()) for t in arrays)
        scratch = _ckpt_scratch("persymbol_ragged_jump", dev, L.cst_persymbol_ragged_jump_scratch_bytes(n_chunks))
        N.check(getattr(L, fn_name + "_jump" + suffix)(_cfg(*encoded.config), *head, _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                              encoded.words.numel(), _ptr(encoded.n_words), *model,
                                              _ptr(target), _ptr(sym_offsets), n_streams, jump.interval, _ptr(jump.chunk_offsets), n_chunks,
                                              *(_ptr(t) for t in arrays), _ptr(scratch), _ptr(status), _stream_ptr()), fn_name + "_jump" + suffix)
        return out, status
    extra = plain_extra() if plain_extra is not None else ()
    N.check(getattr(N.lib(), fn_name + suffix)(_cfg(*encoded.config), *head, _ptr(encoded.words), _ptr(encoded.word_offsets), 0,
                                               encoded.words.numel(), _ptr(encoded.n_words), *model, *extra, _ptr(target),
                                               _ptr(sym_offsets), n_streams, _ptr(order) if order is not None else None, _ptr(status), _stream_ptr()),
            fn_name + suffix)
    return out, status


@_keeps_plain_signature
def ans_encode_gaussian_ragged(symbols, sym_offsets, min_symbol, max_symbol, means, stds, config=(32, 64, 24), order="auto", *,
                               jump_every=0) -> RaggedBatch:
    """One AnsCoder per stream, streams of different lengths: encode_reverse(symbols[lo:hi], QuantizedGaussian(min, max), means[lo:hi],
    stds[lo:hi]) + get_compressed with (lo, hi) = sym_offsets[s], sym_offsets[s + 1], for all streams in ONE launch.  `symbols` flat
    int32; `means` / `stds` flat float64 or float32 of the same numel (a float32 pair is read as it is, see _gaussian_args); `sym_offsets` int64 [n + 1] as `ragged` returns it.
    Every stream's words are those of ans_encode_gaussian for that stream alone.  The slabs are sized as in ans_encode_ragged; the
    batch carries the schedule it ran with in `.order` (see _ragged_order).
    jump_every: 0 (default) -- no jump points, `.jump` is None.  A positive multiple of 16: the encoder also notes AnsCoder.pos() in
    front of every jump_every symbols of every stream (the words are unchanged) and the batch carries the table as `.jump` (a
    RaggedJump); ans_decode_gaussian_ragged then decodes all chunks side by side, and a launch lasts jump_every steps instead of its
    longest stream's length.  Keyword only (see _keeps_plain_signature).  "auto": see _encode_persymbol_ragged and DESIGN.md 4.18.  The same holds for all eight
    {ans,range}_encode_{gaussian,laplace,cauchy,family}_ragged (range batches carry a RangeRaggedJump).
    One kernel for every batch size: built for many streams (16 384 and more); a few streams are coded correctly, but slowly --
    rectangular batches of few streams have ans_encode_gaussian's two-pass route."""
    return _encode_persymbol_ragged("cst_ans_encode_gaussian_ragged", "ans", symbols, sym_offsets, min_symbol, max_symbol, means, stds, config, order,
                                    jump_every=jump_every)


def ans_decode_gaussian_ragged(encoded: RaggedBatch, sym_offsets, min_symbol, max_symbol, means, stds, out: Optional[torch.Tensor] = None,
                               order="auto"):
    """AnsCoder(words of stream s).decode(QuantizedGaussian(min, max), means[lo:hi], stds[lo:hi]) for every stream of a RaggedBatch:
    stream s yields sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:].  Returns (symbols flat, status per stream).
    `order`: "auto" reuses the encoder's schedule, or keys on the word counts (see _ragged_order).  One kernel for every batch size, as
    the encoder: few streams decode correctly, but slowly."""
    return _decode_persymbol_ragged("cst_ans_decode_gaussian_ragged", "ans", encoded, sym_offsets, min_symbol, max_symbol, means, stds, out, order)


@_keeps_plain_signature
def range_encode_gaussian_ragged(symbols, sym_offsets, min_symbol, max_symbol, means, stds, config=(32, 64, 24), order="auto", *,
                                 jump_every=0) -> RaggedBatch:
    """One RangeEncoder per stream, streams of different lengths: encode(symbols[lo:hi], QuantizedGaussian(min, max), means[lo:hi],
    stds[lo:hi]) + get_compressed -- ans_encode_gaussian_ragged for the queue.  Every stream's words are those of range_encode_gaussian
    for that stream alone; a slab holds min(n, ceil(n P / W)) + 2 words, rounded up to 4; the batch says `.coder == "range"`."""
    return _encode_persymbol_ragged("cst_range_encode_gaussian_ragged", "range", symbols, sym_offsets, min_symbol, max_symbol, means, stds, config,
                                    order, jump_every=jump_every)


def range_decode_gaussian_ragged(encoded: RaggedBatch, sym_offsets, min_symbol, max_symbol, means, stds, out: Optional[torch.Tensor] = None,
                                 order="auto"):
    """RangeDecoder(words of stream s).decode(QuantizedGaussian(min, max), means[lo:hi], stds[lo:hi]) for every stream of a RaggedBatch
    that a range encoder wrote.  Returns (symbols flat, status per stream); see ans_decode_gaussian_ragged."""
    return _decode_persymbol_ragged("cst_range_decode_gaussian_ragged", "range", encoded, sym_offsets, min_symbol, max_symbol, means, stds, out,
                                    order)


# ---------------------------------------------------------------------------------------------------------------------
# per-symbol QuantizedLaplace / QuantizedCauchy: the same call with another family,
#     coder.encode_reverse(symbols, QuantizedLaplace(lo, hi), means, scales) / coder.decode(QuantizedCauchy(lo, hi), locs, scales)
# (src/pybindings/stream/model.rs:736-900), over the Gaussian's kernels and routes: the exact CDF is evaluated inside the coder
# kernels, nothing is tabulated.  `a` / `b`: location and scale, float64 or float32 tensors of the symbols' shape (a float32 pair is read
# by the kernels as it is and widened in registers; a float32 tensor next to a float64 one is widened: _gaussian_args).
# ---------------------------------------------------------------------------------------------------------------------

FAMILIES = {"laplace": N.FAMILY_LAPLACE, "cauchy": N.FAMILY_CAUCHY}


def _family_id(family) -> int:
    fam = FAMILIES.get(family, family)
    if fam not in (N.FAMILY_LAPLACE, N.FAMILY_CAUCHY):
        raise ValueError("family must be 'laplace' or 'cauchy' (CST_FAMILY_LAPLACE / CST_FAMILY_CAUCHY)")
    return int(fam)


def ans_encode_family(family, symbols, lo, hi, a, b, config=(32, 64, 24), layout="stream_major", stride: Optional[int] = None,
                      out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """One AnsCoder per stream: encode_reverse(symbols[s], Family(lo, hi), a[s], b[s]) + get_compressed."""
    out = _encode_gaussian("cst_ans_encode_family_batch", max_words, symbols, lo, hi, a, b, config, layout, stride, out, (_family_id(family),))
    out.jump = None
    return out


def range_encode_family(family, symbols, lo, hi, a, b, config=(32, 64, 24), layout="stream_major", stride: Optional[int] = None,
                        out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """One RangeEncoder per stream: encode(symbols[s], Family(lo, hi), a[s], b[s]) + get_compressed."""
    out = _encode_gaussian("cst_range_encode_family_batch", range_max_words, symbols, lo, hi, a, b, config, layout, stride, out,
                           (_family_id(family),))
    out.jump = None
    return out


def ans_decode_family(family, encoded, lo, hi, a, b, layout="stream_major", offsets=None, out=None, config=None):
    """One AnsCoder per stream: AnsCoder(words[s]).decode(Family(lo, hi), a[s], b[s]).  `encoded`: an EncodedBatch, or
    (packed, n_words) with offsets= (compact()).  Returns (symbols, status)."""
    return _decode_gaussian("cst_ans_decode_family_batch", True, encoded, lo, hi, a, b, layout, offsets, out, config, (_family_id(family),))


def range_decode_family(family, encoded, lo, hi, a, b, layout="stream_major", offsets=None, out=None, config=None):
    """One RangeDecoder per stream: RangeDecoder(words[s]).decode(Family(lo, hi), a[s], b[s]).  Returns (symbols, status)."""
    return _decode_gaussian("cst_range_decode_family_batch", False, encoded, lo, hi, a, b, layout, offsets, out, config, (_family_id(family),))


def _named_family(fn, family):
    def call(*args, **kwargs):
        return fn(family, *args, **kwargs)
    call.__name__ = fn.__name__.replace("family", family)
    call.__doc__ = f"{fn.__name__}('{family}', ...)"
    return call


ans_encode_laplace, ans_encode_cauchy = _named_family(ans_encode_family, "laplace"), _named_family(ans_encode_family, "cauchy")
ans_decode_laplace, ans_decode_cauchy = _named_family(ans_decode_family, "laplace"), _named_family(ans_decode_family, "cauchy")
range_encode_laplace, range_encode_cauchy = _named_family(range_encode_family, "laplace"), _named_family(range_encode_family, "cauchy")
range_decode_laplace, range_decode_cauchy = _named_family(range_decode_family, "laplace"), _named_family(range_decode_family, "cauchy")


# ... and for streams of DIFFERENT lengths: the ragged Gaussian calls over another family (flat symbols / a / b + sym_offsets)

@_keeps_plain_signature
def ans_encode_family_ragged(family, symbols, sym_offsets, lo, hi, a, b, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """One AnsCoder per stream: encode_reverse(symbols[s], Family(lo, hi), a[s], b[s]) + get_compressed (see ans_encode_gaussian_ragged)."""
    return _encode_persymbol_ragged("cst_ans_encode_family_ragged", "ans", symbols, sym_offsets, lo, hi, a, b, config, order, (_family_id(family),),
                                    jump_every)


@_keeps_plain_signature
def range_encode_family_ragged(family, symbols, sym_offsets, lo, hi, a, b, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """One RangeEncoder per stream: encode(symbols[s], Family(lo, hi), a[s], b[s]) + get_compressed (see range_encode_gaussian_ragged)."""
    return _encode_persymbol_ragged("cst_range_encode_family_ragged", "range", symbols, sym_offsets, lo, hi, a, b, config, order,
                                    (_family_id(family),), jump_every)


def ans_decode_family_ragged(family, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, out: Optional[torch.Tensor] = None, order="auto"):
    """One AnsCoder per stream: AnsCoder(words of stream s).decode(Family(lo, hi), a[s], b[s]).  Returns (symbols flat, status)."""
    return _decode_persymbol_ragged("cst_ans_decode_family_ragged", "ans", encoded, sym_offsets, lo, hi, a, b, out, order, (_family_id(family),))


def range_decode_family_ragged(family, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, out: Optional[torch.Tensor] = None, order="auto"):
    """One RangeDecoder per stream: RangeDecoder(words of stream s).decode(Family(lo, hi), a[s], b[s]).  Returns (symbols flat, status)."""
    return _decode_persymbol_ragged("cst_range_decode_family_ragged", "range", encoded, sym_offsets, lo, hi, a, b, out, order,
                                    (_family_id(family),))


ans_encode_laplace_ragged, ans_encode_cauchy_ragged = (_named_family(ans_encode_family_ragged, f) for f in ("laplace", "cauchy"))
ans_decode_laplace_ragged, ans_decode_cauchy_ragged = (_named_family(ans_decode_family_ragged, f) for f in ("laplace", "cauchy"))
range_encode_laplace_ragged, range_encode_cauchy_ragged = (_named_family(range_encode_family_ragged, f) for f in ("laplace", "cauchy"))
range_decode_laplace_ragged, range_decode_cauchy_ragged = (_named_family(range_decode_family_ragged, f) for f in ("laplace", "cauchy"))


# ... and random access into them: selected streams, or ranges of streams (ans_decode_ragged_select for models that differ per symbol)

def _decode_persymbol_ragged_select(fn_name, coder, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, streams, first, count, out, family=()):
    """the body of every {ans,range}_decode_{gaussian,family}_ragged_select: the queries of _select_queries on the arguments of
    _decode_persymbol_ragged"""
    jump = _ragged_jump_of(encoded, coder)
    sym_offsets, _, a, b = _gaussian_ragged_args(sym_offsets, None, a, b, f32=True)
    r = _select_queries(encoded, jump, sym_offsets, streams, first, count, out)
    return _persymbol_select_call(_f32_name(fn_name, a), coder, encoded, jump, r, (*family, int(lo), int(hi)), (_ptr(_never_null(a)), _ptr(_never_null(b))))


def _persymbol_select_call(fn_name, coder, encoded: RaggedBatch, jump, r: _SelectQueries, front, model):
    """a per-symbol select entry point on prepared queries: cfg, `front` (what the model puts in front of the words), the words block,
    `model` (its arrays), the streams, the table, the queries, the scratch"""
    if r.n_queries == 0:
        return r.out[:0], r.out_offsets, r.status
    L = N.lib()
    if r.interval:
        arrays = (jump.pos, jump.state) if coder == "ans" else (jump.pos, jump.lower, jump.range)
        table = (r.interval, _ptr(jump.chunk_offsets), min(int(t.numel()) for t in arrays), *(_ptr(t) for t in arrays))
    else:
        table = (0, None, 0, None, None) if coder == "ans" else (0, None, 0, None, None, None)
    # (r.out stands in where it is empty: the entry points refuse NULL and write nothing)
    head = (*_select_tail(r)[:6], _ptr(_never_null(r.out)), _ptr(r.out_offsets))
    scratch = _ckpt_scratch("persymbol_ragged_select", encoded.words.device, L.cst_persymbol_ragged_select_scratch_bytes(r.n_pieces))
    N.check(getattr(L, fn_name)(_cfg(*encoded.config), *front, _ptr(encoded.words), _ptr(encoded.word_offsets), 0, encoded.words.numel(),
                                _ptr(encoded.n_words), *model, _ptr(r.sym_offsets), r.n_streams, *table, *head, _ptr(scratch), _ptr(r.status),
                                _stream_ptr()), fn_name)
    return r.out[:r.total], r.out_offsets, r.status


def ans_decode_gaussian_ragged_select(encoded: RaggedBatch, sym_offsets, min_symbol, max_symbol, means, stds, streams, first=None, count=None,
                                      out: Optional[torch.Tensor] = None):
    """Random access into a batch of ans_encode_gaussian_ragged: query q decodes symbols [first[q], first[q] + count[q]) of stream
    streams[q], and nothing else is decoded.  `means` / `stds`: the batch's full arrays, exactly as ans_decode_gaussian_ragged takes
    them; `streams`, `first`, `count` and the three results (symbols flat int32, out_offsets int64 [n_queries + 1], status int32
    [n_queries]) as in ans_decode_ragged_select.  With jump points (`jump_every` of the encoder) a query starts at the jump point in
    front of `first`, decodes and discards first % interval symbols with THEIR parameters, and every chunk it touches runs on a lane of
    its own; without them it starts where its stream starts.  Only the parameters from that starting point to the query's end can
    influence anything: the rest of `means` / `stds` may hold anything.  A query that meets an invalid model or an impossible quantile,
    in its discarded part too, reports IMPOSSIBLE_SYMBOL (1); a refused one INVALID_DATA (3) and writes nothing.  The same holds for
    all eight {ans,range}_decode_{gaussian,laplace,cauchy,family}_ragged_select."""
    return _decode_persymbol_ragged_select("cst_ans_decode_gaussian_ragged_select", "ans", encoded, sym_offsets, min_symbol, max_symbol, means, stds,
                                           streams, first, count, out)


def range_decode_gaussian_ragged_select(encoded: RaggedBatch, sym_offsets, min_symbol, max_symbol, means, stds, streams, first=None, count=None,
                                        out: Optional[torch.Tensor] = None):
    """ans_decode_gaussian_ragged_select for a batch of range_encode_gaussian_ragged: a piece seeks to its (pos, lower, range) entry
    and reads forward."""
    return _decode_persymbol_ragged_select("cst_range_decode_gaussian_ragged_select", "range", encoded, sym_offsets, min_symbol, max_symbol, means,
                                           stds, streams, first, count, out)


def ans_decode_family_ragged_select(family, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, streams, first=None, count=None,
                                    out: Optional[torch.Tensor] = None):
    """ans_decode_gaussian_ragged_select over Family(lo, hi) with a[s], b[s] (see ans_decode_family_ragged)."""
    return _decode_persymbol_ragged_select("cst_ans_decode_family_ragged_select", "ans", encoded, sym_offsets, lo, hi, a, b, streams, first, count, out,
                                           (_family_id(family),))


def range_decode_family_ragged_select(family, encoded: RaggedBatch, sym_offsets, lo, hi, a, b, streams, first=None, count=None,
                                      out: Optional[torch.Tensor] = None):
    """range_decode_gaussian_ragged_select over Family(lo, hi) with a[s], b[s] (see range_decode_family_ragged)."""
    return _decode_persymbol_ragged_select("cst_range_decode_family_ragged_select", "range", encoded, sym_offsets, lo, hi, a, b, streams, first, count,
                                           out, (_family_id(family),))


ans_decode_laplace_ragged_select, ans_decode_cauchy_ragged_select = (_named_family(ans_decode_family_ragged_select, f) for f in ("laplace", "cauchy"))
range_decode_laplace_ragged_select, range_decode_cauchy_ragged_select = (_named_family(range_decode_family_ragged_select, f)
                                                                         for f in ("laplace", "cauchy"))


# ---------------------------------------------------------------------------------------------------------------------
# per-symbol Categorical models from a matrix of probabilities: the reference's
#     coder.encode_reverse(symbols, Categorical(perfect=False), probabilities) / coder.decode(Categorical(lazy=True), probabilities)
# (src/pybindings/stream/model/internals.rs:399-514) -- what an autoregressive model on the GPU puts out.  `probabilities`: a
# float32 or float64 tensor of shape symbols.shape + (K,), contiguous in the chosen layout; the "fast" quantisation runs in its
# dtype inside the coder kernels (float32 is NOT widened: the reference's tables differ between the two), symbols are 0 .. K - 1.
# perfect=True: Categorical(perfect=True), the reference's default -- `perfectly_quantized_probabilities` in f64 (float32 IS widened,
# as the reference does), one wave per row on the device (csrc/cst_categorical_perfect.hip), K <= 1024.
# ---------------------------------------------------------------------------------------------------------------------

_PROB_BYTES = {torch.float32: 4, torch.float64: 8}


def _categorical_args(matrix_shape, probabilities, precision, perfect=False):
    if not isinstance(probabilities, torch.Tensor):
        raise ValueError("probabilities must live in device memory (HBM)")
    if probabilities.dtype not in _PROB_BYTES:
        raise TypeError("probabilities must have dtype torch.float32 or torch.float64")
    if matrix_shape is not None and tuple(probabilities.shape[:-1]) != tuple(matrix_shape):
        raise ValueError("probabilities must have the shape of the symbol matrix plus one axis of K entries")
    k = int(probabilities.shape[-1]) if probabilities.dim() else 0
    if perfect:
        if k < 2 or k > min(N.CATEGORICAL_PERFECT_MAX_K, 1 << precision):
            raise ValueError(f"a Categorical(perfect=True) model on the device needs 2 <= K <= min({N.CATEGORICAL_PERFECT_MAX_K}, 2**precision) entries")
    elif k < 2 or k >= (1 << precision) - 1:
        raise ValueError("a Categorical model needs 2 <= K < 2**precision - 1 entries")
    if not probabilities.is_cuda:
        raise ValueError("probabilities must live in device memory (HBM)")
    return probabilities.contiguous(), _PROB_BYTES[probabilities.dtype], k


def categorical_cdf_rows(probabilities, precision: int = 24, perfect: bool = False, return_moves: bool = False):
    """The quantised cdf rows of `probabilities` [..., K], tabulated on the GPU: an int32 tensor [..., K + 1] holding uint32 left
    cumulatives and 2^precision, the rows that cst_*_decode_rows_batch use.  perfect=False: the fast quantisation in the dtype of
    the input (cst_categorical_fast_cdf_rows), the rows of model.Categorical(perfect=False).  perfect=True: the cross-entropy-
    optimal one in f64 (cst_categorical_perfect_cdf_rows, one wave per row, K <= 1024), the rows of model.Categorical(perfect=True);
    return_moves=True then returns (rows, moves), `moves` an int32 tensor [...] of the unit moves of every row's search.
    Raises the reference's ValueError if a row is not normalizable, and a RuntimeError naming the row if a search was stopped."""
    if probabilities.dim() < 1:
        raise ValueError("probabilities must have at least one axis")
    if return_moves and not perfect:
        raise ValueError("return_moves needs perfect=True: the fast quantisation does not search")
    probs, nbytes, k = _categorical_args(None, probabilities, precision, perfect)
    n_rows = probs.numel() // k
    rows = torch.empty(tuple(probs.shape[:-1]) + (k + 1,), dtype=torch.int32, device=probs.device)
    bad = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=probs.device)
    moves = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=probs.device) if perfect else None
    if n_rows:
        if perfect:
            N.check(N.lib().cst_categorical_perfect_cdf_rows(int(precision), _ptr(probs), nbytes, n_rows, k, _ptr(rows), _ptr(bad), _ptr(moves),
                                                             _stream_ptr()), "cst_categorical_perfect_cdf_rows")
        else:
            N.check(N.lib().cst_categorical_fast_cdf_rows(int(precision), _ptr(probs), nbytes, n_rows, k, _ptr(rows), _ptr(bad), _stream_ptr()),
                    "cst_categorical_fast_cdf_rows")
        codes = bad[:n_rows]
        if bool(codes.any().item()):
            stopped = (codes == 2).nonzero()
            if stopped.numel():
                raise RuntimeError(f"Categorical(perfect=True): the search of row {int(stopped[0].item())} did not converge "
                                   f"within {16 * k + 1024} unit moves")
            raise ValueError("Probability distribution not normalizable (the array of probabilities\n"
                             "might be empty, contain negative values or NaNs, or sum to infinity).")
    if return_moves:
        return rows, moves[:n_rows].reshape(tuple(probs.shape[:-1]))
    return rows


def _perfect_name(fn_name, perfect):
    return fn_name.replace("_categorical_batch", "_categorical_perfect_batch") if perfect else fn_name


def _encode_categorical(fn_name, max_words_fn, symbols, probabilities, config, layout, stride, out, perfect=False):
    fn_name = _perfect_name(fn_name, perfect)
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    probs, nbytes, k = _categorical_args(symbols.shape, probabilities, config[2], perfect)
    if out is None:
        out = _new_batch(n_streams, stride or max_words_fn(n_per, config), symbols.device, config)
    N.check(getattr(N.lib(), fn_name)(_cfg(*config), _ptr(symbols), _ptr(probs), nbytes, k, n_streams, n_per, lay, _ptr(out.words),
                                      out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status), N.FLAG_NONE, _stream_ptr()), fn_name)
    out.jump = None
    return out


def ans_encode_categorical(symbols, probabilities, config=(32, 64, 24), layout="stream_major", stride: Optional[int] = None,
                           out: Optional[EncodedBatch] = None, perfect: bool = False) -> EncodedBatch:
    """One AnsCoder per stream: encode_reverse(symbols[s], Categorical(perfect=perfect), probabilities[s]) + get_compressed.
    perfect=True: every row quantised by one wave (cst_ans_encode_categorical_perfect_batch, K <= 1024)."""
    return _encode_categorical("cst_ans_encode_categorical_batch", max_words, symbols, probabilities, config, layout, stride, out, perfect)


def range_encode_categorical(symbols, probabilities, config=(32, 64, 24), layout="stream_major", stride: Optional[int] = None,
                             out: Optional[EncodedBatch] = None, perfect: bool = False) -> EncodedBatch:
    """One RangeEncoder per stream: encode(symbols[s], Categorical(perfect=perfect), probabilities[s]) + get_compressed."""
    return _encode_categorical("cst_range_encode_categorical_batch", range_max_words, symbols, probabilities, config, layout, stride, out,
                               perfect)


def _decode_categorical(fn_name, ans, encoded, probabilities, layout, offsets, out, config, perfect=False):
    fn_name = _perfect_name(fn_name, perfect)
    if isinstance(encoded, EncodedBatch):
        words, n_words, config = encoded.words, encoded.n_words, config or encoded.config
        stride = words.shape[1]
    else:
        words, n_words = encoded
        stride = words.shape[1] if words.dim() == 2 else 0
        config = config or (32, 64, 24)
    if not isinstance(probabilities, torch.Tensor) or probabilities.dim() != 3:
        raise ValueError("probabilities must be 3-d: the symbol matrix's two axes and one of K entries")
    n_streams, n_per, lay = _layout_shape(probabilities[..., 0], layout)
    if n_streams != n_words.numel():
        raise ValueError("probabilities do not match the number of streams")
    probs, nbytes, k = _categorical_args(probabilities.shape[:2], probabilities, config[2], perfect)
    dev = words.device
    if out is None:
        out = torch.empty(tuple(probs.shape[:2]), dtype=torch.int32, device=dev)
    status = torch.empty(n_streams, dtype=torch.int32, device=dev)
    args = [_cfg(*config), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words), _ptr(probs), nbytes, k, _ptr(out), n_streams, n_per,
            lay, None]
    if ans:
        args.append(None)          # d_n_words_out
    N.check(getattr(N.lib(), fn_name)(*args, _ptr(status), N.FLAG_NONE, _stream_ptr()), fn_name)
    return out, status


def ans_decode_categorical(encoded, probabilities, layout="stream_major", offsets=None, out=None, config=None, perfect: bool = False):
    """One AnsCoder per stream: AnsCoder(words[s]).decode(Categorical(perfect=perfect), probabilities[s]).  `encoded`: an
    EncodedBatch, or (packed, n_words) with offsets= (compact()).  Returns (symbols, status)."""
    return _decode_categorical("cst_ans_decode_categorical_batch", True, encoded, probabilities, layout, offsets, out, config, perfect)


def range_decode_categorical(encoded, probabilities, layout="stream_major", offsets=None, out=None, config=None, perfect: bool = False):
    """One RangeDecoder per stream: RangeDecoder(words[s]).decode(Categorical(perfect=perfect), probabilities[s]).  Returns
    (symbols, status)."""
    return _decode_categorical("cst_range_decode_categorical_batch", False, encoded, probabilities, layout, offsets, out, config, perfect)


# ---------------------------------------------------------------------------------------------------------------------
# ... for streams of DIFFERENT lengths: the ragged calls' indexing (flat symbols + sym_offsets) on a flat matrix of rows,
# `probabilities` [symbols.numel(), K], plain and with jump points (Categorical(perfect=False) / Categorical(lazy=True); perfect=True: the
# *_categorical_perfect_ragged names behind them)
# ---------------------------------------------------------------------------------------------------------------------

def _categorical_ragged_args(sym_offsets, n_rows, probabilities, precision, perfect=False):
    sym_offsets = _require_cuda(sym_offsets, torch.int64, "sym_offsets")
    n_streams = sym_offsets.numel() - 1
    if sym_offsets.dim() != 1 or n_streams < 0:
        raise ValueError("sym_offsets must be 1-d and hold n_streams + 1 entries")
    if not isinstance(probabilities, torch.Tensor) or probabilities.dim() != 2:
        raise ValueError("probabilities must be 2-d: one row of K entries per symbol")
    probs, nbytes, k = _categorical_args(None if n_rows is None else (n_rows,), probabilities, precision, perfect)
    return sym_offsets, n_streams, probs, nbytes, k


def _encode_categorical_ragged(fn_name, coder, symbols, sym_offsets, probabilities, config, order, jump_every, perfect=False) -> RaggedBatch:
    """the body of {ans,range}_encode_categorical_ragged: _encode_persymbol_ragged with a matrix of rows in place of (lo, hi, a, b).
    jump_every="auto" keeps the RAGGED_JUMP_EVERY rule of the other families -- a jump point every 256 symbols where the streams average
    more than 256.  That rule was measured for the Gaussian, Laplace and Cauchy forms.  For the Categorical it was
    measured at one shape and not tuned: 16 384 streams of 256 .. 8192 symbols, K = 64, float32, ANS: encode + decode 7.46 + 110.2 ->
    7.56 + 9.07 ms, lower in every alternation under both coders; other K and other intervals were not measured."""
    jump_every = _persymbol_jump_every(jump_every)
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    if symbols.dim() != 1:
        raise ValueError("symbols must be flat")
    sym_offsets, n_streams, probs, nbytes, k = _categorical_ragged_args(sym_offsets, symbols.numel(), probabilities, config[2], perfect)
    model = (_ptr(_never_null(symbols)), _ptr(_never_null(probs)), nbytes, k, symbols.numel())
    return _encode_ragged_slabs(fn_name, coder, symbols, sym_offsets, n_streams, config, order, jump_every, model)


def _decode_categorical_ragged(fn_name, coder, encoded: RaggedBatch, sym_offsets, probabilities, out, order, perfect=False):
    jump = _ragged_jump_of(encoded, coder)
    sym_offsets, n_streams, probs, nbytes, k = _categorical_ragged_args(sym_offsets, None, probabilities, encoded.config[2], perfect)
    n_total = int(probs.shape[0])
    # perfect=True, whole streams: the host loops over pieces of positions up to the longest stream -- the one value read back
    longest = (lambda: (max(int((sym_offsets[1:] - sym_offsets[:-1]).max().item()), 0),)) if perfect else None
    return _decode_ragged_slabs(fn_name, coder, encoded, jump, sym_offsets, n_streams, n_total, out, order, (),
                                (_ptr(_never_null(probs)), nbytes, k, n_total), longest)


def ans_encode_categorical_ragged(symbols, sym_offsets, probabilities, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """One AnsCoder per stream, streams of different lengths: encode_reverse(symbols[lo:hi], Categorical(perfect=False),
    probabilities[lo:hi]) + get_compressed with (lo, hi) = sym_offsets[s], sym_offsets[s + 1], for all streams in ONE call.  `symbols`
    flat int32; `probabilities` [symbols.numel(), K], float32 or float64 (quantised in its dtype, as ans_encode_categorical does);
    `sym_offsets` int64 [n + 1] as `ragged` returns it.  Every stream's words are those of ans_encode_categorical for that stream alone.
    The slabs, `.order` and `jump_every` (0, a positive multiple of 16, or "auto"; the batch then carries a RaggedJump as `.jump`) are
    those of ans_encode_gaussian_ragged.  Two passes -- the entries of all rows, then one lane per stream -- whatever the batch: built
    for many streams; a few are coded correctly, but slowly."""
    return _encode_categorical_ragged("cst_ans_encode_categorical_ragged", "ans", symbols, sym_offsets, probabilities, config, order, jump_every)


def ans_decode_categorical_ragged(encoded: RaggedBatch, sym_offsets, probabilities, out: Optional[torch.Tensor] = None, order="auto"):
    """AnsCoder(words of stream s).decode(Categorical(lazy=True), probabilities[lo:hi]) for every stream of a RaggedBatch: stream s
    yields sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:].  Returns (symbols flat, status per stream).  A batch
    with jump points decodes its chunks side by side when `order` is None or "auto"; a schedule handed in decodes whole streams."""
    return _decode_categorical_ragged("cst_ans_decode_categorical_ragged", "ans", encoded, sym_offsets, probabilities, out, order)


def range_encode_categorical_ragged(symbols, sym_offsets, probabilities, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """One RangeEncoder per stream, streams of different lengths: ans_encode_categorical_ragged for the queue.  Every stream's words
    are those of range_encode_categorical for that stream alone; the batch says `.coder == "range"` and carries a RangeRaggedJump."""
    return _encode_categorical_ragged("cst_range_encode_categorical_ragged", "range", symbols, sym_offsets, probabilities, config, order,
                                      jump_every)


def range_decode_categorical_ragged(encoded: RaggedBatch, sym_offsets, probabilities, out: Optional[torch.Tensor] = None, order="auto"):
    """RangeDecoder(words of stream s).decode(Categorical(lazy=True), probabilities[lo:hi]) for every stream of a RaggedBatch that a
    range encoder wrote.  Returns (symbols flat, status per stream); see ans_decode_categorical_ragged."""
    return _decode_categorical_ragged("cst_range_decode_categorical_ragged", "range", encoded, sym_offsets, probabilities, out, order)


# ... and with the perfect quantisation, Categorical(perfect=True), the reference's default: new names, the signatures of the four above

def ans_encode_categorical_perfect_ragged(symbols, sym_offsets, probabilities, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """ans_encode_categorical_ragged with Categorical(perfect=True): every row is quantised by one wave of the device quantiser
    (cst_ans_encode_categorical_perfect_ragged, 2 <= K <= min(1024, 2**precision)), in f64 whatever the dtype of `probabilities`
    (float32 is widened, as the reference does).  Every stream's words are those of ans_encode_categorical(..., perfect=True) for that
    stream alone.  Slabs, `.order`, `jump_every` (0, a positive multiple of 16, or "auto": the RAGGED_JUMP_EVERY rule) and `.jump` are
    those of ans_encode_categorical_ragged; DESIGN.md 4.23 has what was measured."""
    return _encode_categorical_ragged("cst_ans_encode_categorical_perfect_ragged", "ans", symbols, sym_offsets, probabilities, config, order,
                                      jump_every, True)


def ans_decode_categorical_perfect_ragged(encoded: RaggedBatch, sym_offsets, probabilities, out: Optional[torch.Tensor] = None, order="auto"):
    """AnsCoder(words of stream s).decode(Categorical(perfect=True), probabilities[lo:hi]) for every stream of a RaggedBatch.  Returns
    (symbols flat, status per stream).  The rows are tabulated on the device, a piece of positions of a group of streams at a time,
    and looked up.  A batch with jump points decodes its chunks side by side when `order` is None or "auto", and reads nothing back;
    whole streams (no jump points, or a schedule handed in) read back one value, the longest stream's length."""
    return _decode_categorical_ragged("cst_ans_decode_categorical_perfect_ragged", "ans", encoded, sym_offsets, probabilities, out, order, True)


def range_encode_categorical_perfect_ragged(symbols, sym_offsets, probabilities, config=(32, 64, 24), order="auto", *, jump_every=0) -> RaggedBatch:
    """ans_encode_categorical_perfect_ragged for the queue: every stream's words are those of range_encode_categorical(...,
    perfect=True) for that stream alone; the batch says `.coder == "range"` and carries a RangeRaggedJump."""
    return _encode_categorical_ragged("cst_range_encode_categorical_perfect_ragged", "range", symbols, sym_offsets, probabilities, config, order,
                                      jump_every, True)


def range_decode_categorical_perfect_ragged(encoded: RaggedBatch, sym_offsets, probabilities, out: Optional[torch.Tensor] = None, order="auto"):
    """RangeDecoder(words of stream s).decode(Categorical(perfect=True), probabilities[lo:hi]) for every stream of a RaggedBatch that
    a range encoder wrote.  Returns (symbols flat, status per stream); see ans_decode_categorical_perfect_ragged."""
    return _decode_categorical_ragged("cst_range_decode_categorical_perfect_ragged", "range", encoded, sym_offsets, probabilities, out, order,
                                      True)


# ... and random access into the eight batches above: ans_decode_gaussian_ragged_select with a matrix of rows in place of the parameters

def _decode_categorical_ragged_select(fn_name, coder, encoded: RaggedBatch, sym_offsets, probabilities, streams, first, count, out, perfect=False):
    """the body of {ans,range}_decode_categorical[_perfect]_ragged_select: the queries of _select_queries on the arguments of
    _decode_categorical_ragged.  perfect: the call also takes the longest piece, which the queries' single read-back brings along."""
    jump = _ragged_jump_of(encoded, coder)
    sym_offsets, _, probs, nbytes, k = _categorical_ragged_args(sym_offsets, None, probabilities, encoded.config[2], perfect)
    r = _select_queries(encoded, jump, sym_offsets, streams, first, count, out, piece_bound=perfect)
    n_total = int(probs.shape[0])
    model = (_ptr(_never_null(probs)), nbytes, k, n_total) + ((int(r.max_piece),) if perfect else ())
    return _persymbol_select_call(fn_name, coder, encoded, jump, r, (), model)


def ans_decode_categorical_ragged_select(encoded: RaggedBatch, sym_offsets, probabilities, streams, first=None, count=None,
                                         out: Optional[torch.Tensor] = None):
    """Random access into a batch of ans_encode_categorical_ragged: query q decodes symbols [first[q], first[q] + count[q]) of stream
    streams[q], and nothing else is decoded.  `probabilities`: the batch's full [n_total, K] matrix, exactly as
    ans_decode_categorical_ragged takes it; `streams`, `first`, `count` and the three results (symbols flat int32, out_offsets int64
    [n_queries + 1], status int32 [n_queries]) as in ans_decode_ragged_select.  With jump points (`jump_every` of the encoder) a query
    starts at the jump point in front of `first`, decodes and discards first % interval symbols with THEIR rows, and every chunk it
    touches runs on a lane of its own; without them it starts where its stream starts.  Only the rows from that starting point to the
    query's end can influence anything: the rest of `probabilities` may hold anything.  A query that meets a bad row or an impossible
    quantile, in its discarded part too, reports IMPOSSIBLE_SYMBOL (1); a refused one -- also one whose stream's rows reach beyond the
    matrix -- INVALID_DATA (3) and writes nothing.  The same holds for all four
    {ans,range}_decode_categorical[_perfect]_ragged_select."""
    return _decode_categorical_ragged_select("cst_ans_decode_categorical_ragged_select", "ans", encoded, sym_offsets, probabilities, streams, first,
                                             count, out)


def range_decode_categorical_ragged_select(encoded: RaggedBatch, sym_offsets, probabilities, streams, first=None, count=None,
                                           out: Optional[torch.Tensor] = None):
    """ans_decode_categorical_ragged_select for a batch of range_encode_categorical_ragged: a piece seeks to its (pos, lower, range)
    entry and reads forward."""
    return _decode_categorical_ragged_select("cst_range_decode_categorical_ragged_select", "range", encoded, sym_offsets, probabilities, streams,
                                             first, count, out)


def ans_decode_categorical_perfect_ragged_select(encoded: RaggedBatch, sym_offsets, probabilities, streams, first=None, count=None,
                                                 out: Optional[torch.Tensor] = None):
    """ans_decode_categorical_ragged_select for a batch of ans_encode_categorical_perfect_ragged: only the rows the queries' pieces walk
    are quantised, a wave each, within the row budget of ans_decode_categorical_perfect_ragged -- a selection costs what its rows cost."""
    return _decode_categorical_ragged_select("cst_ans_decode_categorical_perfect_ragged_select", "ans", encoded, sym_offsets, probabilities,
                                             streams, first, count, out, True)


def range_decode_categorical_perfect_ragged_select(encoded: RaggedBatch, sym_offsets, probabilities, streams, first=None, count=None,
                                                   out: Optional[torch.Tensor] = None):
    """ans_decode_categorical_perfect_ragged_select for a batch of range_encode_categorical_perfect_ragged."""
    return _decode_categorical_ragged_select("cst_range_decode_categorical_perfect_ragged_select", "range", encoded, sym_offsets, probabilities,
                                             streams, first, count, out, True)


# ---------------------------------------------------------------------------------------------------------------------
# checkpointed streams (the reference's Pos / Seek jump tables, src/stream/stack.rs:1107-1139): one long stream decodes
# on as many lanes as it has chunks
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Checkpoints:
    interval: int
    pos: torch.Tensor        # int32 [n_streams, n_chunks]: words in the bulk in front of chunk j (AnsCoder.pos()[0])
    state: torch.Tensor      # int64 [n_streams, n_chunks]: coder state there (AnsCoder.pos()[1])


def ans_encode_checkpointed(symbols: torch.Tensor, model: Model, interval: int, config=(32, 64, 24), layout="stream_major",
                            stride: Optional[int] = None, out=None):
    """ans_encode + a checkpoint in front of every `interval` symbols.  Returns (EncodedBatch, Checkpoints); the words are
    those of ans_encode.  Models with one table per stream are taken too (stream-major): see DESIGN.md 4.12 (sub-lanes).
    out: (EncodedBatch, Checkpoints) of an earlier call with the same shapes, to code into the same buffers."""
    narrow = _SYMBOL_BYTES.get(symbols.dtype, 4) if symbols.dtype in _SYMBOL_BYTES else 4
    if narrow != 4:        # int8 / int16 matrices (round 5: cst_ans_encode_batch_ckpt_sym; int8 lines are read by the encoder loops themselves)
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only (map the symbols to indices first)")
        symbols = _require_cuda(symbols, symbols.dtype, "symbols")
    else:
        symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    dev = symbols.device
    n_chunks = (n_per + interval - 1) // interval
    if out is not None:
        out, ck = out
        stride = out.words.shape[1]
        if ck.interval != int(interval) or tuple(ck.pos.shape) != (n_streams, n_chunks):
            raise ValueError("out: checkpoints of another shape")
    else:
        stride = stride or max_words(n_per, config)
        out = EncodedBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config))
        ck = Checkpoints(int(interval), torch.zeros((n_streams, n_chunks), dtype=torch.int32, device=dev),
                         torch.zeros((n_streams, n_chunks), dtype=torch.int64, device=dev))
    if narrow != 4:
        L = N.lib()
        scratch = _ckpt_scratch("ckpt_widen", dev, L.cst_ckpt_sym_scratch_bytes(n_streams, n_per, int(interval), narrow))
        N.check(L.cst_ans_encode_batch_ckpt_sym(model._h, _cfg(*config), _ptr(symbols), narrow, n_streams, n_per, lay, _ptr(out.words), stride,
                                                _ptr(out.n_words), int(interval), _ptr(ck.pos), _ptr(ck.state), _ptr(out.status), _ptr(scratch),
                                                _stream_ptr()), "cst_ans_encode_batch_ckpt_sym")
        return out, ck
    N.check(N.lib().cst_ans_encode_batch_ckpt(model._h, _cfg(*config), _ptr(symbols), n_streams, n_per, lay, _ptr(out.words), stride,
                                              _ptr(out.n_words), int(interval), _ptr(ck.pos), _ptr(ck.state), _ptr(out.status),
                                              _stream_ptr()), "cst_ans_encode_batch_ckpt")
    return out, ck


def _ckpt_scratch(kind, dev, nbytes):
    """a scratch buffer per purpose, device AND HIP stream (two calls on different streams must not share one: the kernels of
    both may be in flight), grown on demand.  A buffer is only ever used on the stream it was allocated on -- the stream in its
    key -- so the caching allocator's stream-ordered reuse holds when a larger one replaces it."""
    key = (kind, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf


def _status_per_stream(part_status: torch.Tensor) -> torch.Tensor:
    """[n_streams, n_chunks] -> [n_streams]: a stream's status is the worst of its chunks' (cst_ckpt_status_per_stream)"""
    n_streams, n_chunks = part_status.shape
    out = torch.empty(n_streams, dtype=torch.int32, device=part_status.device)
    N.check(N.lib().cst_ckpt_status_per_stream(_ptr(part_status), n_streams, n_chunks, _ptr(out), _stream_ptr()), "cst_ckpt_status_per_stream")
    return out


def _check_jump_shape(checkpoints, n_per_stream: int) -> None:
    """The C calls index the jump tables as [n_streams][n_per_stream / interval]: a table with another number of points per stream
    (a prefix decode of a batch encoded with more) would be read with the wrong row stride -- refuse it."""
    if tuple(checkpoints.pos.shape[1:]) != (n_per_stream // checkpoints.interval,) or n_per_stream % checkpoints.interval != 0:
        raise ValueError(f"jump points every {checkpoints.interval} symbols, {checkpoints.pos.shape[1]} per stream, do not describe streams of "
                         f"{n_per_stream} symbols (decode them whole, or without the jump points)")
    for t in vars(checkpoints).values():
        if isinstance(t, torch.Tensor) and tuple(t.shape) != tuple(checkpoints.pos.shape):
            raise ValueError("jump points: tensors of different shapes")


def _decode_jump_composed(encoded: EncodedBatch, ck: Checkpoints, model: Model, n_per_stream: int, out, status, layout: str):
    """AnsCoder.seek + decode of every chunk for the two batch forms cst_ans_decode_batch_ckpt does not take, composed of the plain
    batched decode (raw states, counts = the jump points' word counts):
      packed 16-bit words (stream-major): the n_streams * k chunks are streams of their own at their stream's slab (offsets in
        16-bit words) and rows of the matrix [n_streams * k][interval] -- ONE launch;
      symbol-major: chunk j of all streams is the symbol-major matrix [interval][n_streams] behind row j * interval -- k launches.
    A jump point with more words than its stream holds is caller data gone wrong: CST_STREAM_INVALID_DATA, nothing is read."""
    n_streams, k = ck.pos.shape
    interval = ck.interval
    dev = encoded.words.device
    L = N.lib()
    words = encoded.words
    stride = words.shape[1]
    flags = N.FLAG_RAW_STATE | (N.FLAG_PACKED_W16 if encoded.packed16 else N.FLAG_NONE)
    bad = (ck.pos.view(torch.int32) < 0) | (ck.pos > encoded.n_words.view(-1, 1)) | (ck.pos > stride)
    pos = torch.where(bad, torch.zeros_like(ck.pos), ck.pos)
    if layout == "stream_major":
        v_off = (torch.arange(n_streams, device=dev, dtype=torch.int64) * stride).view(-1, 1).expand(n_streams, k).contiguous()
        v_n, v_state = pos.contiguous().view(-1), ck.state.clone().view(-1)     # (CST_FLAG_RAW_STATE: the state array is in AND out)
        part = torch.empty(n_streams * k, dtype=torch.int32, device=dev)
        N.check(L.cst_ans_decode_batch(model._h, _cfg(*encoded.config), _ptr(words), _ptr(v_off), 0, words.numel(), _ptr(v_n), _ptr(out),
                                       n_streams * k, interval, N.LAYOUT_STREAM_MAJOR, _ptr(v_state), None, _ptr(part), flags, _stream_ptr()),
                "cst_ans_decode_batch")
        status.copy_(part.view(n_streams, k))
    else:
        part = torch.empty(n_streams, dtype=torch.int32, device=dev)
        for j in range(k):
            n_j, st_j = pos[:, j].contiguous(), ck.state[:, j].clone()
            N.check(L.cst_ans_decode_batch(model._h, _cfg(*encoded.config), _ptr(words), None, stride, words.numel(), _ptr(n_j),
                                           _ptr(out[j * interval:(j + 1) * interval]), n_streams, interval, N.LAYOUT_SYMBOL_MAJOR, _ptr(st_j), None,
                                           _ptr(part), flags, _stream_ptr()), "cst_ans_decode_batch")
            status[:, j] = part
    status.masked_fill_(bad, N.STREAM_INVALID_DATA)
    return _to_symbols(model, out), status


def ans_decode_checkpointed(encoded, checkpoints: Checkpoints, model: Model, n_per_stream: int, out=None, status=None,
                            dtype=torch.int32, offsets: Optional[torch.Tensor] = None, config=None, layout="stream_major"):
    """Decodes every chunk on its own lane (AnsCoder.seek(pos, state) + `interval` symbols per chunk).
    Returns (symbols [n_streams, n_per_stream], status [n_streams, n_chunks]).  dtype (or the dtype of `out`): int32, or int16 / int8 for
    a narrow symbol matrix (cst_ans_decode_batch_ckpt_sym: int8 chunks of whole 128-symbol lines are written by the decoder loops).
    `encoded`: an EncodedBatch (slabs), or the PACKED words of compact() / container.load() / a gather with `offsets` (int64
    [n_streams + 1]) and `config` -- jump points count words from the start of their stream, wherever the stream lies."""
    if not isinstance(encoded, EncodedBatch):
        if offsets is None:
            raise ValueError("packed words need their offsets")
        words = encoded[0] if isinstance(encoded, (tuple, list)) else encoded
        encoded = EncodedBatch(words.view(1, -1), checkpoints.pos[:, 0], checkpoints.pos[:, 0], tuple(config or (32, 64, 12)))
    n_streams = checkpoints.pos.shape[0]
    stride_arg = 0 if offsets is not None else encoded.words.shape[1]
    dev = encoded.words.device
    n_chunks = checkpoints.pos.shape[1]
    _check_jump_shape(checkpoints, n_per_stream)
    if layout not in ("stream_major", "symbol_major"):
        raise ValueError("layout")
    if out is None:
        out = torch.empty((n_streams, n_per_stream) if layout == "stream_major" else (n_per_stream, n_streams), dtype=dtype, device=dev)
    if status is None:
        status = torch.empty((n_streams, n_chunks), dtype=torch.int32, device=dev)
    L = N.lib()
    narrow = _SYMBOL_BYTES.get(out.dtype)
    if narrow is None:
        raise TypeError("decoded symbols are int32, int16 or int8")
    if encoded.packed16 or layout == "symbol_major":
        if offsets is not None or narrow != 4:
            raise ValueError("jump points of packed 16-bit or symbol-major batches: slabs and int32 symbols")
        return _decode_jump_composed(encoded, checkpoints, model, n_per_stream, out, status, layout)
    if narrow != 4:
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only")
        scratch = _ckpt_scratch("ans_ckpt_sym", dev,
                                L.cst_ckpt_sym_scratch_bytes(n_streams, n_per_stream, checkpoints.interval, narrow))
        N.check(L.cst_ans_decode_batch_ckpt_sym(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(offsets), stride_arg,
                                                encoded.words.numel(), checkpoints.interval, _ptr(checkpoints.pos), _ptr(checkpoints.state), _ptr(out),
                                                narrow, n_streams, n_per_stream, _ptr(scratch), _ptr(status), _stream_ptr()),
                "cst_ans_decode_batch_ckpt_sym")
        return out, status
    scratch = _ckpt_scratch("ans_ckpt", dev, L.cst_ckpt_scratch_bytes(n_streams, n_per_stream, checkpoints.interval))
    N.check(L.cst_ans_decode_batch_ckpt(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(offsets), stride_arg,
                                        encoded.words.numel(), checkpoints.interval, _ptr(checkpoints.pos), _ptr(checkpoints.state), _ptr(out), n_streams,
                                        n_per_stream, _ptr(scratch), _ptr(status), _stream_ptr()), "cst_ans_decode_batch_ckpt")
    return _to_symbols(model, out), status


@dataclass
class RangeCheckpoints:
    """RangeEncoder.pos() in front of every chunk (queue.rs:182-196): words emitted so far incl. held-back ones, and the state"""
    interval: int
    pos: torch.Tensor        # int32 [n_streams, n_chunks]
    lower: torch.Tensor      # int64 [n_streams, n_chunks]  (uint64 values)
    range: torch.Tensor      # int64 [n_streams, n_chunks]


def range_encode_checkpointed(symbols: torch.Tensor, model: Model, interval: int, config=(32, 64, 12), layout="stream_major",
                              stride: Optional[int] = None, out=None):
    """range_encode + a jump point in front of every `interval` symbols.  Returns (EncodedBatch, RangeCheckpoints); the words
    are those of range_encode.  One table per stream (as for range_encode): stream-major only, any interval >= 1."""
    _check_range_per_stream(model, _layout_shape(symbols, layout)[0], layout, interval)
    narrow = _SYMBOL_BYTES.get(symbols.dtype, 4) if symbols.dtype in _SYMBOL_BYTES else 4
    if narrow != 4:        # int8 / int16 matrices (round 6: cst_range_encode_batch_ckpt_sym; int8 tiles are read by the encoder loop itself)
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only (map the symbols to indices first)")
        symbols = _require_cuda(symbols, symbols.dtype, "symbols")
    else:
        symbols = _to_indices(model, _require_cuda(symbols, torch.int32, "symbols"))
    n_streams, n_per, lay = _layout_shape(symbols, layout)
    dev = symbols.device
    n_chunks = (n_per + interval - 1) // interval
    if out is not None:
        out, ck = out
        stride = out.words.shape[1]
        if ck.interval != int(interval) or tuple(ck.pos.shape) != (n_streams, n_chunks):
            raise ValueError("out: checkpoints of another shape")
    else:
        stride = stride or range_max_words(n_per, config)
        out = EncodedBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config))
        ck = RangeCheckpoints(int(interval), *(torch.zeros((n_streams, n_chunks), dtype=dt, device=dev)
                                               for dt in (torch.int32, torch.int64, torch.int64)))
    if narrow != 4:
        L = N.lib()
        scratch = _ckpt_scratch("range_sym", dev, L.cst_range_sym_scratch_bytes(n_streams, n_per, int(interval), narrow))
        N.check(L.cst_range_encode_batch_ckpt_sym(model._h, _cfg(*config), _ptr(symbols), narrow, n_streams, n_per, lay, _ptr(out.words), stride,
                                                  _ptr(out.n_words), int(interval), _ptr(ck.pos), _ptr(ck.lower), _ptr(ck.range),
                                                  _ptr(out.status), _ptr(scratch), _stream_ptr()), "cst_range_encode_batch_ckpt_sym")
        return out, ck
    N.check(N.lib().cst_range_encode_batch_ckpt(model._h, _cfg(*config), _ptr(symbols), n_streams, n_per, lay, _ptr(out.words), stride,
                                                _ptr(out.n_words), int(interval), _ptr(ck.pos), _ptr(ck.lower), _ptr(ck.range),
                                                _ptr(out.status), _stream_ptr()), "cst_range_encode_batch_ckpt")
    return out, ck


def range_decode_checkpointed(encoded, checkpoints: RangeCheckpoints, model: Model, n_per_stream: int, out=None, status=None,
                              offsets: Optional[torch.Tensor] = None, config=None, dtype=torch.int32):
    """Every chunk on its own lane: RangeDecoder.seek(pos, (lower, range)) + `interval` symbols per chunk.
    Returns (symbols [n_streams, n_per_stream], status [n_streams, n_chunks]).  `encoded`: an EncodedBatch, or (packed words, n_words)
    with `offsets` (int64 [n_streams + 1]) and `config` for the words of compact() / container.load() / a gather.
    model: one shared table, or one table per stream (every chunk lane then holds its own copy of its stream's row)."""
    stride_arg = None
    if not isinstance(encoded, EncodedBatch):
        if offsets is None:
            raise ValueError("packed words need their offsets")
        words, n_words = encoded
        encoded = EncodedBatch(words.view(1, -1), n_words, n_words, tuple(config or (32, 64, 12)))
        stride_arg = 0
    n_streams = encoded.n_words.numel()
    dev = encoded.words.device
    n_chunks = checkpoints.pos.shape[1]
    _check_jump_shape(checkpoints, n_per_stream)
    _check_range_per_stream(model, n_streams, "stream_major", checkpoints.interval)
    if checkpoints.pos.shape[0] != n_streams:
        raise ValueError("jump points of another batch: one row per stream")
    if out is None:
        out = torch.empty((n_streams, n_per_stream), dtype=dtype, device=dev)
    if status is None:
        status = torch.empty((n_streams, n_chunks), dtype=torch.int32, device=dev)
    L = N.lib()
    narrow = _SYMBOL_BYTES.get(out.dtype)
    if narrow is None:
        raise TypeError("decoded symbols are int32, int16 or int8")
    if narrow != 4:        # (round 6: int8 matrices are written by the sub-lane decoder itself, cst_range_decode_batch_ckpt_sym)
        if model.noncontiguous:
            raise ValueError("narrow symbol matrices: contiguous alphabets only")
        scratch = _ckpt_scratch("range_sym", dev, L.cst_range_sym_scratch_bytes(n_streams, n_per_stream, checkpoints.interval, narrow))
        N.check(L.cst_range_decode_batch_ckpt_sym(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(offsets),
                                                  encoded.words.shape[1] if stride_arg is None else stride_arg, encoded.words.numel(), _ptr(encoded.n_words),
                                                  checkpoints.interval, _ptr(checkpoints.pos), _ptr(checkpoints.lower), _ptr(checkpoints.range), _ptr(out),
                                                  narrow, n_streams, n_per_stream, _ptr(scratch), _ptr(status), _stream_ptr()),
                "cst_range_decode_batch_ckpt_sym")
        return out, status
    scratch = _ckpt_scratch("range_ckpt", dev, L.cst_range_ckpt_scratch_bytes(n_streams, n_per_stream, checkpoints.interval))
    N.check(L.cst_range_decode_batch_ckpt(model._h, _cfg(*encoded.config), _ptr(encoded.words), _ptr(offsets),
                                          encoded.words.shape[1] if stride_arg is None else stride_arg, encoded.words.numel(), _ptr(encoded.n_words), checkpoints.interval, _ptr(checkpoints.pos),
                                          _ptr(checkpoints.lower), _ptr(checkpoints.range), _ptr(out), n_streams, n_per_stream,
                                          _ptr(scratch), _ptr(status), _stream_ptr()), "cst_range_decode_batch_ckpt")
    return _to_symbols(model, out), status


def ans_encode_gaussian_checkpointed(symbols, min_symbol, max_symbol, means, stds, interval: int, config=(32, 64, 24),
                                     stride: Optional[int] = None, out=None):
    """ans_encode_gaussian + a jump point in front of every `interval` symbols (a multiple of 16 that divides the row length;
    batches of at least 16 384 streams, stream-major).  Returns (EncodedBatch, Checkpoints); the words are ans_encode_gaussian's."""
    symbols = _require_cuda(symbols, torch.int32, "symbols")
    n_streams, n_per, lay = _layout_shape(symbols, "stream_major")
    means, stds = _gaussian_args(symbols.shape, means, stds, f32=True)
    fn = _f32_name("cst_ans_encode_gaussian_batch_ckpt", means)
    dev = symbols.device
    n_chunks = (n_per + interval - 1) // interval
    if out is not None:
        out, ck = out
    else:
        stride = stride or max_words(n_per, config)
        out = EncodedBatch(torch.empty((n_streams, stride), dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev),
                           torch.empty(n_streams, dtype=torch.int32, device=dev), tuple(config))
        ck = Checkpoints(int(interval), torch.zeros((n_streams, n_chunks), dtype=torch.int32, device=dev),
                         torch.zeros((n_streams, n_chunks), dtype=torch.int64, device=dev))
    N.check(getattr(N.lib(), fn)(_cfg(*config), int(min_symbol), int(max_symbol), _ptr(symbols), _ptr(means), _ptr(stds),
                                 n_streams, n_per, lay, _ptr(out.words), out.words.shape[1], _ptr(out.n_words),
                                 int(interval), _ptr(ck.pos), _ptr(ck.state), _ptr(out.status), _stream_ptr()), fn)
    return out, ck


def ans_decode_gaussian_checkpointed(encoded: EncodedBatch, checkpoints: Checkpoints, min_symbol, max_symbol, means, stds, out=None, status=None):
    """Every chunk on its own lane: AnsCoder.seek(pos, state) + decode(QuantizedGaussian(min, max), means[chunk], stds[chunk]).
    Returns (symbols [n_streams, n_per_stream], status [n_streams, n_chunks])."""
    if means.dim() != 2:
        raise ValueError("means must be 2-d")
    n_streams, n_per = means.shape
    means, stds = _gaussian_args(means.shape, means, stds, f32=True)
    fn = _f32_name("cst_ans_decode_gaussian_batch_ckpt", means)
    dev = encoded.words.device
    n_chunks = checkpoints.pos.shape[1]
    _check_jump_shape(checkpoints, n_per)
    if checkpoints.pos.shape[0] != n_streams:
        raise ValueError("jump points of another batch: one row per stream")
    if out is None:
        out = torch.empty((n_streams, n_per), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((n_streams, n_chunks), dtype=torch.int32, device=dev)
    L = N.lib()
    scratch = _ckpt_scratch("ans_ckpt", dev, L.cst_ckpt_scratch_bytes(n_streams, n_per, checkpoints.interval))
    N.check(getattr(L, fn)(_cfg(*encoded.config), int(min_symbol), int(max_symbol), _ptr(encoded.words), None,
                           encoded.words.shape[1], encoded.words.numel(), checkpoints.interval, _ptr(checkpoints.pos),
                           _ptr(checkpoints.state), _ptr(means), _ptr(stds), _ptr(out), n_streams, n_per, _ptr(scratch),
                           _ptr(status), _stream_ptr()), fn)
    return out, status


# ---------------------------------------------------------------------------------------------------------------------
# Huffman symbol codes (constriction.symbol): one bit container per stream, a shared codebook (_huffman.py)
# ---------------------------------------------------------------------------------------------------------------------

from ._huffman import (BitJump, HuffmanBatch, HuffmanCodebook, huffman_count_bits, huffman_decode, huffman_decode_ragged,  # noqa: E402,F401
                       huffman_decode_ragged_select, huffman_encode, huffman_encode_ragged, huffman_tree)
from ._exp_golomb import (exp_golomb_count_bits, exp_golomb_decode, exp_golomb_decode_ragged, exp_golomb_decode_ragged_select,  # noqa: E402,F401
                          exp_golomb_encode, exp_golomb_encode_ragged, exp_golomb_max_words)


# ---------------------------------------------------------------------------------------------------------------------
# indexed table coding: every symbol names one of K tabulated models (csrc/cst_indexed.hip) -- what a learned
# codec does whose hyperprior quantises every latent's scale to one of K levels:
#     coder.encode_symbols_reverse(symbols.zip(indices.map(|k| &tables[k])))      src/stream/stack.rs:784-849
# ---------------------------------------------------------------------------------------------------------------------

class TableSet:
    """K cdfs that share a support and a precision (include/constriction_amd.h, cst_table_set): at most 256 tables whose LDS image
    fits beside the coder's rings and tiles (64 tables of 255 symbols at any precision, 256 tables of 64 symbols up to P = 16)."""

    def __init__(self, handle, cdfs: np.ndarray, min_symbol: int, precision: int):
        self._h = handle
        self._cdfs = cdfs
        self._min_symbol, self._precision = int(min_symbol), int(precision)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.load_library().cst_table_set_destroy(h)
            except Exception:
                pass

    @classmethod
    def from_cdfs(cls, cdfs, min_symbol: int, precision: int) -> "TableSet":
        """cdfs [K, n + 1], every row with cdf[0] = 0 < cdf[1] < ... < cdf[n] = 2^P (ValueError otherwise, and for a set that does
        not fit)."""
        cdfs = np.ascontiguousarray(cdfs, dtype=np.uint32)
        if cdfs.ndim != 2 or cdfs.shape[1] < 3:
            raise ValueError("cdfs must be 2-d: one row of n_symbols + 1 >= 3 cumulatives per table")
        if not 1 <= cdfs.shape[0] <= 256:
            raise ValueError("a table set holds 1 to 256 tables")
        if not 1 <= int(precision) <= 24:
            raise ValueError("precision must be 1 .. 24")
        h = C.c_void_p()
        N.check(N.load_library().cst_table_set_create(int(precision), int(min_symbol), cdfs.shape[1] - 1, cdfs.shape[0], cdfs.ctypes.data,
                                                      C.byref(h)), "cst_table_set_create")
        return cls(h, cdfs, min_symbol, precision)

    @classmethod
    def quantized_gaussians(cls, min_symbol: int, max_symbol: int, means, stds, precision: int) -> "TableSet":
        """K tables LeakyQuantizer(min..=max) x Gaussian(means[k], stds[k]), tabulated on the GPU in bit-exact f64 by the kernel behind
        Model.quantized_gaussian / Model.quantized_gaussian_per_stream."""
        means = torch.as_tensor(means, dtype=torch.float64).reshape(-1)
        stds = torch.as_tensor(stds, dtype=torch.float64).reshape(-1)
        if means.numel() != stds.numel() or not 1 <= means.numel() <= 256:
            raise ValueError("means and stds: one entry per table, 1 to 256 tables")
        dev = torch.device("cuda", torch.cuda.current_device())
        if precision <= 16:
            rows = Model.quantized_gaussian_per_stream(min_symbol, max_symbol, means.to(dev), stds.to(dev), precision).cdfs_device()
            cdfs = rows.cpu().numpy().view(np.uint32)
        else:       # (per-stream models stop at 16 bits: one shared-table model per level, the same kernel)
            cdfs = np.stack([Model.quantized_gaussian(min_symbol, max_symbol, float(m), float(s), precision).cdf()
                             for m, s in zip(means.tolist(), stds.tolist())])
        return cls.from_cdfs(cdfs, min_symbol, precision)

    @classmethod
    def fit(cls, symbols, indices, n_tables: int, min_symbol: int, max_symbol: int, precision: int, perfect: bool = False) -> "TableSet":
        """K tables, table k fitted on the device to the symbols whose index is k (count_symbols + fit_cdf_rows): the factorised
        prior of static two-pass coding.  A class nobody names gets the uniform table.  ValueError if a symbol lies outside
        [min_symbol, max_symbol] or an index outside [0, n_tables)."""
        _fit_precision(precision, 24)
        if indices is None or n_tables is None:
            raise ValueError("TableSet.fit needs indices and n_tables")
        counts, outside = count_symbols(symbols, min_symbol, max_symbol, indices=indices, n_tables=n_tables)
        _fit_refuse_outside(outside)
        rows = fit_cdf_rows(counts, precision, perfect)
        return cls.from_cdfs(rows.cpu().numpy().view(np.uint32), min_symbol, precision)

    @property
    def precision(self):
        return self._precision

    @property
    def min_symbol(self):
        return self._min_symbol

    @property
    def n_symbols(self):
        return self._cdfs.shape[1] - 1

    @property
    def n_tables(self):
        return self._cdfs.shape[0]

    def cdfs(self) -> np.ndarray:
        """uint32 [n_tables, n_symbols + 1]: the rows the set was built from"""
        return self._cdfs.copy()


def _indexed_args(symbols_shape, device, indices, tables, config):
    """the checks of the indexed calls that need no device: ValueError before any native call"""
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    if tuple(config[:2]) != (32, 64) or int(config[2]) != tables.precision:
        raise ValueError("indexed coding: config must be (32, 64, precision of the table set)")
    if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.uint8, torch.int32):
        raise ValueError("indices must be a torch.uint8 or torch.int32 tensor")
    if tuple(indices.shape) != tuple(symbols_shape):
        raise ValueError("indices must have the shape of the symbol matrix")
    if not indices.is_cuda or indices.device != device:
        raise ValueError("indices must live in device memory (HBM), on the device of the symbols / words")
    return indices.contiguous(), (1 if indices.dtype == torch.uint8 else 4)


def _encode_indexed(fn_name, max_words_fn, symbols, indices, tables, config, stride, out):
    if not isinstance(symbols, torch.Tensor) or symbols.dim() != 2 or symbols.dtype != torch.int32 or not symbols.is_cuda:
        raise ValueError("symbols must be a 2-d torch.int32 tensor [n_streams, n_per_stream] in device memory (HBM)")
    indices, index_bytes = _indexed_args(symbols.shape, symbols.device, indices, tables, config)
    symbols = symbols.contiguous()
    n_streams, n_per = symbols.shape
    if out is None:
        out = _new_batch(n_streams, stride or max_words_fn(n_per, config), symbols.device, config)
    N.check(getattr(N.lib(), fn_name)(tables._h, _cfg(*config), _ptr(symbols), _ptr(indices), index_bytes, n_streams, n_per,
                                      N.LAYOUT_STREAM_MAJOR, _ptr(out.words), out.words.shape[1], _ptr(out.n_words), None, _ptr(out.status),
                                      N.FLAG_NONE, _stream_ptr()), fn_name)
    out.jump = None
    return out


def ans_encode_indexed(symbols, indices, tables: TableSet, config=(32, 64, 16), stride: Optional[int] = None,
                       out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """One AnsCoder per stream: encode_symbols_reverse(symbols[s] zipped with tables[indices[s]]) + get_compressed.  `indices`:
    torch.uint8 or torch.int32, the symbols' shape.  No jump points; the batch works with compact / reverse_words / container.save."""
    return _encode_indexed("cst_ans_encode_indexed_batch", max_words, symbols, indices, tables, config, stride, out)


def range_encode_indexed(symbols, indices, tables: TableSet, config=(32, 64, 16), stride: Optional[int] = None,
                         out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """One RangeEncoder per stream: encode_symbols(symbols[s] zipped with tables[indices[s]]) + get_compressed."""
    return _encode_indexed("cst_range_encode_indexed_batch", range_max_words, symbols, indices, tables, config, stride, out)


def _decode_indexed(fn_name, ans, encoded, indices, tables, n_per_stream, offsets, out):
    if isinstance(encoded, EncodedBatch):
        words, n_words = encoded.words, encoded.n_words
        stride = words.shape[1]
    else:
        words, n_words = encoded
        stride = words.shape[1] if words.dim() == 2 else 0
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    n_streams = n_words.numel()
    indices, index_bytes = _indexed_args((n_streams, int(n_per_stream)), words.device, indices, tables, (32, 64, tables.precision))
    if isinstance(encoded, EncodedBatch) and tuple(encoded.config) != (32, 64, tables.precision):
        raise ValueError("the batch was not coded with (32, 64, precision of the table set)")
    if stride == 0 and offsets is None:
        raise ValueError("packed words need their offsets")
    if out is None:
        out = torch.empty((n_streams, int(n_per_stream)), dtype=torch.int32, device=words.device)
    elif tuple(out.shape) != (n_streams, int(n_per_stream)) or out.dtype != torch.int32 or out.device != words.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous int32 tensor [n_streams, n_per_stream] on the device of the words")
    status = torch.empty(n_streams, dtype=torch.int32, device=words.device)
    args = [tables._h, _cfg(32, 64, tables.precision), _ptr(words), _ptr(offsets), stride, words.numel(), _ptr(n_words), _ptr(indices),
            index_bytes, _ptr(out), n_streams, int(n_per_stream), N.LAYOUT_STREAM_MAJOR, None]
    if ans:
        args.append(None)          # d_n_words_out
    N.check(getattr(N.lib(), fn_name)(*args, _ptr(status), N.FLAG_NONE, _stream_ptr()), fn_name)
    return out, status


def ans_decode_indexed(encoded, indices, tables: TableSet, n_per_stream: int, offsets=None, out=None):
    """One AnsCoder per stream: AnsCoder(words[s]).decode_symbols(tables[indices[s]]).  `encoded`: an EncodedBatch, or
    (packed, n_words) with offsets= (compact()).  Returns (symbols, status)."""
    return _decode_indexed("cst_ans_decode_indexed_batch", True, encoded, indices, tables, n_per_stream, offsets, out)


def range_decode_indexed(encoded, indices, tables: TableSet, n_per_stream: int, offsets=None, out=None):
    """One RangeDecoder per stream: RangeDecoder(words[s]).decode_symbols(tables[indices[s]]).  Returns (symbols, status)."""
    return _decode_indexed("cst_range_decode_indexed_batch", False, encoded, indices, tables, n_per_stream, offsets, out)


# ---- ... for streams of different lengths, plain and with jump points (csrc/cst_indexed_ragged.hip) ----

def _indexed_ragged_args(n_elements, device, indices, tables, config):
    """_indexed_args for flat arrays: the checks of the ragged indexed calls that need no device handle.  `n_elements`: the numel the
    indices must have, or None (the decoders: the indices say how many symbols there are)"""
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    if tuple(config[:2]) != (32, 64) or int(config[2]) != tables.precision:
        raise ValueError("indexed coding: config must be (32, 64, precision of the table set)")
    if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.uint8, torch.int32):
        raise ValueError("indices must be a torch.uint8 or torch.int32 tensor")
    if indices.dim() != 1 or (n_elements is not None and indices.numel() != n_elements):
        raise ValueError("indices must be flat, one per symbol")
    if not indices.is_cuda or (device is not None and indices.device != device):
        raise ValueError("indices must live in device memory (HBM), on the device of the symbols / words")
    return indices.contiguous(), (1 if indices.dtype == torch.uint8 else 4)


def _indexed_ragged_offsets(sym_offsets, device):
    if not isinstance(sym_offsets, torch.Tensor) or sym_offsets.dtype != torch.int64 or sym_offsets.dim() != 1 or sym_offsets.numel() < 1:
        raise ValueError("sym_offsets must be a flat torch.int64 tensor [n_streams + 1]")
    if not sym_offsets.is_cuda or sym_offsets.device != device:
        raise ValueError("sym_offsets must live in device memory (HBM), on the device of the symbols / words")
    # (no read-back: that the offsets run from 0 to the number of symbols is the caller's word, as in every ragged call)
    return sym_offsets.contiguous(), sym_offsets.numel() - 1


def _encode_indexed_ragged(fn_name, coder, symbols, indices, sym_offsets, tables, config, order, jump_every):
    # "auto": see DESIGN.md 4.30 for what the rule of _encode_ragged_slabs gives here
    jump_every = _persymbol_jump_every(jump_every)
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    if tuple(config[:2]) != (32, 64) or int(config[2]) != tables.precision:
        raise ValueError("indexed coding: config must be (32, 64, precision of the table set)")
    if not isinstance(symbols, torch.Tensor) or symbols.dim() != 1 or symbols.dtype != torch.int32 or not symbols.is_cuda:
        raise ValueError("symbols must be a flat torch.int32 tensor in device memory (HBM)")
    indices, index_bytes = _indexed_ragged_args(symbols.numel(), symbols.device, indices, tables, config)
    symbols = symbols.contiguous()
    sym_offsets, n_streams = _indexed_ragged_offsets(sym_offsets, symbols.device)
    model = (tables._h, _ptr(_never_null(symbols)), _ptr(_never_null(indices)), index_bytes)
    return _encode_ragged_slabs(fn_name, coder, symbols, sym_offsets, n_streams, tuple(int(c) for c in config), order, jump_every, model)


@_keeps_plain_signature
def ans_encode_indexed_ragged(symbols, indices, sym_offsets, tables: TableSet, config=(32, 64, 16), order="auto", *, jump_every=0) -> RaggedBatch:
    """ans_encode_indexed for streams of different lengths, in ONE launch: stream s is encode_symbols_reverse(symbols[lo:hi] zipped with
    tables[indices[lo:hi]]) + get_compressed, (lo, hi) = sym_offsets[s], sym_offsets[s + 1].  `symbols` flat int32; `indices` flat
    torch.uint8 or torch.int32 of the same numel; `sym_offsets` int64 [n + 1] as `ragged` returns it.  Every stream's words are those of
    ans_encode_indexed for that stream alone.  Slabs, the schedule (`order`, carried in `.order`) and `jump_every` (0, a positive
    multiple of 16, or "auto"; the table travels as `.jump`, a RaggedJump) are those of ans_encode_gaussian_ragged."""
    return _encode_indexed_ragged("cst_ans_encode_indexed_ragged", "ans", symbols, indices, sym_offsets, tables, config, order, jump_every)


@_keeps_plain_signature
def range_encode_indexed_ragged(symbols, indices, sym_offsets, tables: TableSet, config=(32, 64, 16), order="auto", *, jump_every=0) -> RaggedBatch:
    """range_encode_indexed for streams of different lengths: ans_encode_indexed_ragged for the queue.  The batch says `.coder == "range"`
    and carries a RangeRaggedJump where jump points were asked for."""
    return _encode_indexed_ragged("cst_range_encode_indexed_ragged", "range", symbols, indices, sym_offsets, tables, config, order, jump_every)


def _decode_indexed_ragged(fn_name, coder, encoded, indices, sym_offsets, tables, out, order):
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    if not isinstance(encoded, RaggedBatch):
        raise ValueError("encoded must be a RaggedBatch")
    jump = _ragged_jump_of(encoded, coder)
    if tuple(encoded.config) != (32, 64, tables.precision):
        raise ValueError("the batch was not coded with (32, 64, precision of the table set)")
    indices, index_bytes = _indexed_ragged_args(None, None, indices, tables, encoded.config)
    if indices.device != encoded.words.device:
        raise ValueError("indices must live on the device of the words")
    sym_offsets, n_streams = _indexed_ragged_offsets(sym_offsets, indices.device)
    return _decode_ragged_slabs(fn_name, coder, encoded, jump, sym_offsets, n_streams, indices.numel(), out, order, (tables._h,),
                                (_ptr(_never_null(indices)), index_bytes))


def ans_decode_indexed_ragged(encoded: RaggedBatch, indices, sym_offsets, tables: TableSet, out: Optional[torch.Tensor] = None, order="auto"):
    """AnsCoder(words of stream s).decode_symbols(tables[indices[lo:hi]]) for every stream of a RaggedBatch: stream s yields
    sym_offsets[s + 1] - sym_offsets[s] symbols at out[sym_offsets[s]:].  Returns (symbols flat, status per stream).  A batch with a
    jump table decodes its chunks side by side when `order` is None or "auto", and by whole streams when a schedule is handed in."""
    return _decode_indexed_ragged("cst_ans_decode_indexed_ragged", "ans", encoded, indices, sym_offsets, tables, out, order)


def range_decode_indexed_ragged(encoded: RaggedBatch, indices, sym_offsets, tables: TableSet, out: Optional[torch.Tensor] = None, order="auto"):
    """RangeDecoder(words of stream s).decode_symbols(tables[indices[lo:hi]]) for every stream: ans_decode_indexed_ragged for the queue."""
    return _decode_indexed_ragged("cst_range_decode_indexed_ragged", "range", encoded, indices, sym_offsets, tables, out, order)


# ... and random access into them: selected streams, or ranges of streams

def _decode_indexed_ragged_select(fn_name, coder, encoded, indices, sym_offsets, tables, streams, first, count, out):
    """the body of {ans,range}_decode_indexed_ragged_select: the queries of _select_queries on the arguments of _decode_indexed_ragged"""
    if not isinstance(tables, TableSet):
        raise ValueError("tables must be a batched.TableSet")
    if not isinstance(encoded, RaggedBatch):
        raise ValueError("encoded must be a RaggedBatch")
    jump = _ragged_jump_of(encoded, coder)
    if tuple(encoded.config) != (32, 64, tables.precision):
        raise ValueError("the batch was not coded with (32, 64, precision of the table set)")
    indices, index_bytes = _indexed_ragged_args(None, None, indices, tables, encoded.config)
    if indices.device != encoded.words.device:
        raise ValueError("indices must live on the device of the words")
    sym_offsets, _ = _indexed_ragged_offsets(sym_offsets, indices.device)
    r = _select_queries(encoded, jump, sym_offsets, streams, first, count, out)
    return _persymbol_select_call(fn_name, coder, encoded, jump, r, (tables._h,), (_ptr(_never_null(indices)), index_bytes))


def ans_decode_indexed_ragged_select(encoded: RaggedBatch, indices, sym_offsets, tables: TableSet, streams, first=None, count=None,
                                     out: Optional[torch.Tensor] = None):
    """Random access into a batch of ans_encode_indexed_ragged: query q decodes symbols [first[q], first[q] + count[q]) of stream
    streams[q], and nothing else is decoded.  `indices`: the batch's FULL flat array, exactly as ans_decode_indexed_ragged takes it;
    `streams`, `first`, `count` and the three results (symbols flat int32, out_offsets int64 [n_queries + 1], status int32 [n_queries])
    as in ans_decode_ragged_select.  With jump points (`jump_every` of the encoder) a query starts at the jump point in front of
    `first`, decodes and discards first % interval symbols with THEIR tables, and every chunk it touches runs on a lane of its own;
    without them it starts where its stream starts.  Only the indices from that starting point to the query's end are read: the rest of
    `indices` may hold anything.  A query that meets an index >= n_tables, in its discarded part too, reports INVALID_DATA (3) and may
    leave anything in its own slice; a refused one reports INVALID_DATA and writes nothing."""
    return _decode_indexed_ragged_select("cst_ans_decode_indexed_ragged_select", "ans", encoded, indices, sym_offsets, tables, streams, first, count,
                                         out)


def range_decode_indexed_ragged_select(encoded: RaggedBatch, indices, sym_offsets, tables: TableSet, streams, first=None, count=None,
                                       out: Optional[torch.Tensor] = None):
    """ans_decode_indexed_ragged_select for a batch of range_encode_indexed_ragged: a piece seeks to its (pos, lower, range) entry and
    reads forward."""
    return _decode_indexed_ragged_select("cst_range_decode_indexed_ragged_select", "range", encoded, indices, sym_offsets, tables, streams, first,
                                         count, out)
