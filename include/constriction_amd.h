/*
 * constriction_amd.h -- C ABI of the MI355X-native batched entropy-coding backend.
 *
 * This is the drop-in boundary for constriction's stream-coder hot path.
 * The reference has NO FFI surface for this path (only PyO3 bindings); each entry point below
 * names the reference interface it replaces (paths relative to the reference checkout).  A Rust
 * `extern "C"` block / ctypes stub binding exactly these symbols is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types.  `stream` is a hipStream_t passed as void*
 *    (NULL = the default stream).  All `d_*` pointers are DEVICE pointers (HBM), all `h_*`
 *    pointers are host pointers.  The library never frees caller memory.
 *  - all batched calls are asynchronous on `stream`; results are valid after the caller
 *    synchronises that stream.  Functions are re-entrant; no coder call writes global state (the only process-wide data are
 *    the debug switches below: read once when the library is loaded).
 *  - every function returns a cst_status (0 = ok, negative = call-level error).  Per-stream
 *    outcomes go to the caller's `d_status` array (cst_stream_status), mirroring the
 *    reference's per-coder Result values (src/lib.rs:313-316, 376-385).
 *  - coder presets are given as (word_bits, state_bits, precision) = (W, S, P):
 *      (32,64,24) DefaultAnsCoder + the Python API        src/stream/stack.rs:139
 *      (32,64,12) benches/lookup.rs:32-34, BASELINE config C2/C3
 *      (16,32,12) SmallAnsCoder                            src/stream/stack.rs:153
 *    Supported: W=32,S=64,1<=P<=24 and W=16,S=32,1<=P<=16 (hand-scheduled kernels, every entry point), and -- through
 *    cst_ans_encode_batch / cst_ans_decode_batch with table models -- the rest of the reference's type grid
 *    (src/stream/stack.rs:1293-1356): W=32,S=64,24<P<=32; W=16,S=64,P<=16; W=8 with S=64, 32 or 16, P<=8.  Compressed
 *    words are always stored one per uint32_t slot (narrower words occupy the low bits).
 */
#ifndef CONSTRICTION_AMD_H
#define CONSTRICTION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CST_ABI_VERSION 5

typedef enum cst_status {
    CST_OK = 0,
    CST_ERR_INVALID_ARGUMENT = -1, /* bad sizes / NULL pointers / unsupported (W,S,P) */
    CST_ERR_HIP = -2,              /* a HIP runtime call failed (see cst_last_hip_error) */
    CST_ERR_NO_DEVICE = -3,        /* no gfx950 device visible: the product path has NO CPU fallback */
    CST_ERR_MODEL = -4,            /* model cannot be built (support too large, sigma<=0, zero probability) */
    CST_ERR_OUT_OF_MEMORY = -5
} cst_status;

/* per-stream result codes written to d_status[stream] */
typedef enum cst_stream_status {
    CST_STREAM_OK = 0,
    CST_STREAM_IMPOSSIBLE_SYMBOL = 1, /* DefaultEncoderFrontendError::ImpossibleSymbol, src/lib.rs:376-385
                                         (Python: KeyError, src/pybindings/stream/mod.rs:82-89) */
    CST_STREAM_CAPACITY = 2,          /* output slab too small (reference: backend WriteError) */
    CST_STREAM_INVALID_DATA = 3,      /* trailing zero word (src/stream/stack.rs:299-318) or
                                         range-decoder InvalidData (src/stream/queue.rs:989-993) */
    CST_STREAM_OUT_OF_DATA = 4        /* chain coder: DecoderFrontendError::OutOfCompressedData /
                                         EncoderFrontendError::OutOfRemainders (src/stream/chain.rs:854-890) */
} cst_stream_status;

/* memory layout of the int32 symbol matrix */
typedef enum cst_layout {
    CST_LAYOUT_STREAM_MAJOR = 0, /* symbols[stream][t]  (BASELINE config C2) */
    CST_LAYOUT_SYMBOL_MAJOR = 1  /* symbols[t][stream]  (lane-coalesced without LDS staging) */
} cst_layout;

typedef struct cst_coder_config {
    int32_t word_bits;  /* W */
    int32_t state_bits; /* S */
    int32_t precision;  /* P */
} cst_coder_config;

/* flags for the batched coder calls */
#define CST_FLAG_NONE 0u
/* encode: do not append the final state words (leave the state in d_state);
 * decode: do not read the initial state from the end of each stream's words (take it from d_state).
 * Used by the single-coder drop-in object to continue an existing coder
 * (AnsCoder::encode_symbols_reverse on a non-empty coder, src/stream/stack.rs:784-849). */
#define CST_FLAG_RAW_STATE 1u
/* decode (a hint; results do not depend on it): the compressed words are NOT expected in the GPU's caches -- they arrived by
 * DMA from the host or a peer, or were written long ago -- as opposed to words an encode call has just left there.  The
 * (32,64), P <= 12 decoder then reads them as whole 64-byte segments moved by lane quads (cst_ans_dq.hip): 11 - 17 % faster on
 * words that come from HBM, 7 % slower on cache-resident ones at a well-chosen slab stride.  Other kernels
 * ignore it. */
#define CST_FLAG_COLD_WORDS 2u
/* ABI 4, the (16,32) preset only (SmallAnsCoder, src/stream/stack.rs:153: the reference holds its words in a Vec<u16>): the
 * compressed words are PACKED, two per uint32 slot -- d_words is an array of uint16_t (little endian, exactly the bytes of the
 * reference's Vec<u16>), and stride_words, d_n_words, d_offsets, words_capacity all count 16-bit words.  Without the flag every
 * word of this preset occupies a uint32 slot (low half), which doubles the word bytes the kernels move.  cst_ans_encode_batch
 * and cst_ans_decode_batch take it for shared-table models, stream-major symbols, 8 <= precision <= 12 (anything else:
 * CST_ERR_INVALID_ARGUMENT); the slabs pack with cst_compact_words16.  The fast path wants 64-byte aligned slabs
 * (stride_words a multiple of 32: cst_ans_max_words rounds to that). */
#define CST_FLAG_PACKED_W16 4u

/* ------------------------------------------------------------------------------------------
 * library / device
 * ---------------------------------------------------------------------------------------- */

/* ABI version of the loaded library (== CST_ABI_VERSION of the header it was built from). */
int32_t cst_abi_version(void);

/* Number of visible gfx950 devices, or a negative cst_status. */
int32_t cst_device_count(void);

/* Text of the most recent HIP error seen by the calling thread ("" if none). */
const char *cst_last_hip_error(void);

/* ABI 4, diagnostics: the kernel family the calling thread's last batched coder call (cst_ans_* / cst_range_* _batch and their
 * _ckpt forms) launched -- "ans_encode_pc_kernel", "ans_decode_dq_kernel", "range_decode_sub_kernel", ... ; "" before any.
 * The dispatcher picks by shape, alignment and flags; a profile or a benchmark that labels its numbers asks here. */
const char *cst_last_kernel_name(void);

/* Upper bound on the words one stream can produce, min(n, ceil(n*P/W)) + S/W, rounded up to a whole number of
 * 64-byte units so that slabs laid out at this stride from a 64-byte aligned base are all 64-byte aligned (the
 * encoder then writes whole aligned 64-byte groups).  Any other stride remains legal.
 * (At most one word per symbol: src/stream/stack.rs:1035-1040; final state: stack.rs:891-895.) */
size_t cst_ans_max_words(size_t n_symbols, cst_coder_config cfg);

/* Same bound for the range coder: one word per symbol (queue.rs:671-702) + seal words (queue.rs:498-522), rounded
 * up to 64-byte units in the same way (the hand-scheduled encoder needs 64-byte aligned slabs). */
size_t cst_range_max_words(size_t n_symbols, cst_coder_config cfg);

/* ------------------------------------------------------------------------------------------
 * entropy models (device-resident cumulative-frequency tables)
 *
 * A cst_model is the device image of one of the reference's entropy models restricted to a
 * contiguous i32 support [min_symbol, min_symbol + n_symbols):
 *   encode side  = EncoderModel::left_cumulative_and_probability as a table
 *                  (ContiguousCategoricalEntropyModel, src/stream/model/categorical/contiguous.rs:673-700)
 *   decode side  = DecoderModel::quantile_function as ContiguousLookupDecoderModel
 *                  (src/stream/model/categorical/lookup_contiguous.rs:169-187, 564-605)
 * cdf[0] = 0 < cdf[1] < ... < cdf[n] = 2^P.
 * ---------------------------------------------------------------------------------------- */

typedef struct cst_model cst_model;

/* One table shared by all streams, from a host cdf[n_symbols+1] (any tabulated model: the
 * "fast" categorical tables of src/stream/model/categorical.rs:16-54, a LeakyQuantizer table, ...). */
cst_status cst_model_create_table(int32_t precision, int32_t min_symbol, int32_t n_symbols,
                                  const uint32_t *h_cdf, cst_model **out);

/* One shared table = LeakyQuantizer<f64,i32,u{prob_bits},P>(min..=max) x Gaussian(mean,std),
 * i.e. constriction.stream.model.QuantizedGaussian(min, max, mean, std)
 * (src/stream/model/quantize.rs:284-308, 525-568; src/pybindings/stream/model.rs:649-660).
 * The table is computed ON DEVICE in bit-exact f64.  prob_bits = 32 for W=32, 16 for W=16. */
cst_status cst_model_create_gaussian(int32_t precision, int32_t min_symbol, int32_t max_symbol,
                                     double mean, double std, void *stream, cst_model **out);

/* One table PER STREAM (BASELINE config C3): stream s uses Gaussian(d_means[s], d_stds[s]).
 * d_means/d_stds are device arrays of n_streams doubles.  Per-stream tables are coded from LDS: precision <= 16 and
 * a support of at most 1023 symbols (larger ones make the coding calls return CST_ERR_INVALID_ARGUMENT; shared
 * tables have no such limit). */
cst_status cst_model_create_gaussian_per_stream(int32_t precision, int32_t min_symbol, int32_t max_symbol,
                                                const double *d_means, const double *d_stds,
                                                size_t n_streams, void *stream, cst_model **out);

/* One table PER STREAM from cdf rows that are in device memory already: d_cdfs [n_tables][n_symbols + 1], row s the table of
 * stream s -- the general form of cst_model_create_gaussian_per_stream (the same limits: precision <= 16, at most 1023 symbols
 * for the coding calls; the same kernels code with it) and the inverse of cst_model_copy_cdfs.  The rows are copied on `stream`;
 * every row is validated on the device as cst_model_create_table validates its one row (cdf[0] = 0 < cdf[1] < ... < cdf[n] = 2^P),
 * and one bad row makes the call return CST_ERR_MODEL.  Rows fitted to data come from cst_fit_cdf_rows. */
cst_status cst_model_create_tables_per_stream(int32_t precision, int32_t min_symbol, int32_t n_symbols,
                                              const uint32_t *d_cdfs, size_t n_tables, void *stream, cst_model **out);

/* A tabulated model over an ARBITRARY alphabet of distinct i32 symbols (NonContiguousCategoricalEncoderModel /
 * NonContiguousLookupDecoderModel, src/stream/model/categorical/{non_contiguous,lookup_noncontiguous}.rs:429-470, 602-646):
 * h_symbols[i] is the symbol with left cumulative h_cdf[i].  The model proper works on the indices 0..n-1; the two
 * kernels below translate (in place if wanted): encode = cst_symbols_to_indices + cst_ans_encode_batch (a symbol that is
 * not in the alphabet becomes index n, which the coder reports as CST_STREAM_IMPOSSIBLE_SYMBOL), decode =
 * cst_ans_decode_batch + cst_indices_to_symbols. */
cst_status cst_model_create_table_noncontiguous(int32_t precision, int32_t n_symbols, const int32_t *h_symbols,
                                               const uint32_t *h_cdf, cst_model **out);
cst_status cst_symbols_to_indices(const cst_model *model, const int32_t *d_symbols, size_t count, int32_t *d_indices,
                                  void *stream);
cst_status cst_indices_to_symbols(const cst_model *model, const int32_t *d_indices, size_t count, int32_t *d_symbols,
                                  void *stream);

cst_status cst_model_destroy(cst_model *model);

/* Introspection (tests, and get_cdf for host-side tooling). */
int32_t cst_model_precision(const cst_model *model);
int32_t cst_model_min_symbol(const cst_model *model);
int32_t cst_model_n_symbols(const cst_model *model);
size_t cst_model_n_tables(const cst_model *model); /* 1 = shared, else n_streams */
/* Copies table `index`'s cdf[n_symbols+1] to host (synchronises `stream`). */
cst_status cst_model_get_cdf(const cst_model *model, size_t index, uint32_t *h_cdf, void *stream);
/* Copies the cdfs of tables [first, first + count) -- (n_symbols + 1) entries each, back to back -- into DEVICE memory,
 * asynchronously on `stream` (e.g. to draw test symbols from per-stream models without a host round trip). */
cst_status cst_model_copy_cdfs(const cst_model *model, size_t first, size_t count, uint32_t *d_cdfs, void *stream);

/* ------------------------------------------------------------------------------------------
 * model families other than the quantized Gaussian
 * ---------------------------------------------------------------------------------------- */

typedef enum cst_family {
    CST_FAMILY_LAPLACE = 1, /* constriction.stream.model.QuantizedLaplace(min, max, mean, scale), src/pybindings/stream/model.rs:736-800 */
    CST_FAMILY_CAUCHY = 2,  /* QuantizedCauchy(min, max, loc, scale), model.rs:836-900 */
    CST_FAMILY_BINOMIAL = 3 /* Binomial(n, p) over 0..=n, model.rs:903-966 */
} cst_family;

/* LeakyQuantizer<f64,i32,u32,P>(min..=max) x family(a[row], b[row]) tabulated on the device, one row of
 * (max - min + 2) left cumulatives per parameter pair (src/stream/model/quantize.rs:284-308, 525-568 over the
 * `probability` crate's Laplace / Cauchy / Binomial CDFs, evaluated with the libm-crate algorithms in bit-exact f64).
 * Laplace: a = mean, b = scale.  Cauchy: a = loc, b = scale.  Binomial: a = p, d_b unused (may be NULL), min_symbol
 * must be 0 and max_symbol = n; with d_n_per_row != NULL row r is the model over 0..=d_n_per_row[r] (<= max_symbol)
 * and entries past its own 2^P repeat 2^P (the family form `Binomial()` with per-symbol n).  d_bad (optional, one
 * int32 per row) is set to 1 where a row is not strictly increasing, i.e. where the reference panics
 * (quantize.rs:560-566).  The rows feed cst_model_create_table / the *_rows_batch / *_cp_batch entry points. */
cst_status cst_family_cdf_rows(int32_t family, int32_t precision, int32_t min_symbol, int32_t max_symbol,
                               const double *d_a, const double *d_b, const int32_t *d_n_per_row, size_t n_rows,
                               uint32_t *d_rows, int32_t *d_bad, void *stream);

/* Categorical(probabilities, perfect=True): `perfectly_quantized_probabilities` + cumulation
 * (src/stream/model/categorical.rs:56-177, contiguous.rs:301-313) for Probability = u32.  HOST function (a sequential
 * greedy search); h_probs are f64 (f32 inputs widened by the caller, as `F: Into<f64>` does); writes h_cdf[n + 1].
 * CST_ERR_MODEL where the reference returns Err (n < 2, negative / non-normalisable probabilities). */
cst_status cst_categorical_perfect_cdf(const double *h_probs, size_t n, int32_t precision, uint32_t *h_cdf);

/* test hooks: the elementary functions behind the two calls above as the device evaluates them
 * (which: 0 log, 1 log1p, 2 atan, 3 lgamma for x > 0, 4 exp), and the host's log1p */
cst_status cst_debug_family_fn(int32_t which, const double *d_x, double *d_out, size_t n, void *stream);
double cst_debug_host_log1p(double x);

/* ------------------------------------------------------------------------------------------
 * batched ANS coder: one independent AnsCoder<W,S> per stream
 * ---------------------------------------------------------------------------------------- */

/* Replaces, for every stream s in [0, n_streams):
 *     let mut coder = AnsCoder::new();                             src/stream/stack.rs:249
 *     coder.encode_iid_symbols_reverse(symbols[s], &model)?;       src/stream/stack.rs:835-849
 *     out[s] = coder.into_compressed();                            src/stream/stack.rs:891-895
 * (Python: AnsCoder().encode_reverse(symbols, model); get_compressed(),
 *  src/pybindings/stream/stack.rs:529-591, 411-429.)
 *
 * d_symbols   int32 [n_streams][n_per_stream] (or transposed, see layout)
 * d_words     uint32 slabs: stream s writes d_words[s*stride_words ...], in emission order
 * d_n_words   out: words written per stream
 * d_state     uint64 [n_streams] in/out, only with CST_FLAG_RAW_STATE (else may be NULL)
 * d_status    out: cst_stream_status per stream.  On IMPOSSIBLE_SYMBOL / CAPACITY the stream's
 *             n_words is 0 and its slab content is unspecified.
 */
cst_status cst_ans_encode_batch(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                size_t n_streams, size_t n_per_stream, cst_layout layout,
                                uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);

/* Replaces, for every stream s:
 *     let mut coder = AnsCoder::from_compressed(words[s])?;        src/stream/stack.rs:299-318, 440-462
 *     symbols[s] = coder.decode_iid_symbols(n_per_stream, &model)  src/stream/mod.rs:1016-1031, stack.rs:1070-1100
 * (Python: AnsCoder(compressed).decode(model, n), src/pybindings/stream/stack.rs:217-241, 688-752.)
 *
 * The words of stream s are d_words[off(s) .. off(s) + d_n_words[s]) with
 *     off(s) = d_offsets ? d_offsets[s] : s * stride_words
 * so both the slab layout written by cst_ans_encode_batch and the packed layout written by
 * cst_compact_words decode without a copy.  Decoding past the end of a stream is legal and
 * deterministic, exactly as in the reference (stack.rs:1062-1065).
 * Memory safety on corrupt metadata (the reference's decoder pops from a Vec and cannot leave it, src/backends.rs:495-507):
 * `words_capacity` = the number of uint32 slots behind d_words.  A stream whose slice [off(s), off(s) + d_n_words[s])
 * leaves the buffer -- or, in slab form, whose d_n_words[s] exceeds stride_words (checked always) -- is decoded as an
 * EMPTY stream and reports CST_STREAM_INVALID_DATA; nothing outside the buffer is read.  words_capacity = 0 means
 * "unknown": the caller vouches for the packed offsets as in ABI 2.  (The kernels read whole aligned 16-byte chunks:
 * up to 12 bytes before the first and after the last word of a stream are touched, never interpreted; with
 * CST_FLAG_COLD_WORDS whole aligned 64-byte groups: up to 60 bytes either side, inside the allocation that holds d_words
 * -- hipMalloc aligns and pads allocations to 256 bytes -- and that decoder is only taken when the span of the words is known,
 * i.e. never for packed offsets with words_capacity = 0.  A capacity that is the true size of a hipMalloc'ed buffer
 * satisfies both.)  Every decode entry point below takes the same argument.
 * The model must have been created on the current device (CST_ERR_INVALID_ARGUMENT otherwise).
 * With CST_FLAG_RAW_STATE the initial state comes from d_state and the remaining state and word
 * count are written back to d_state / d_n_words_out (d_n_words_out may alias nothing; NULL = discard).
 */
cst_status cst_ans_decode_batch(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                const uint64_t *d_offsets, size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                int32_t *d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                uint64_t *d_state, uint32_t *d_n_words_out, int32_t *d_status,
                                uint32_t flags, void *stream);

/* ABI 4: NARROW symbol matrices.  The reference's coders are generic over the symbol type (`Symbol: PrimInt + ...`,
 * src/stream/model/quantize.rs:229-255); the kernels here code int32 matrices.  What a narrow matrix saves is the LINK: a batch
 * that comes from and returns to host memory is bound by PCIe, and int8 symbols are a quarter of its bytes.  symbol_bytes = 1, 2
 * (signed two's complement) or 4; the narrow types are widened / narrowed on the device next to the coder call through
 * d_scratch (cst_symbols_scratch_bytes(...) bytes, 0 for symbol_bytes = 4; contents irrelevant).  Words, counts and status are
 * those of the int32 calls on the widened values; an encoder symbol outside the model's support is an impossible symbol as ever,
 * a decoder whose model's support does not fit the type returns CST_ERR_INVALID_ARGUMENT.  The two conversions are exported on
 * their own for the other coders (range, per-symbol, checkpointed calls take int32).
 * NARROW MATRICES INSIDE THE LOOPS (round 5): symbol_bytes = 1 or 2 with the default preset (32,64), 8 <= P <= 24, a shared table,
 * stream-major rows that are whole 128-BYTE lines (128 int8 / 64 int16 symbols) of a 128-byte aligned matrix, any number of streams
 * (encode: 64-byte aligned slabs with stride_words % 16 == 0, at most 256 (int8) / 1024 (int16) symbols; decode: a known span of
 * the words) are coded by kernels that read / write the narrow matrix themselves -- no conversion, d_scratch is not touched and
 * may be NULL; the same words, counts, status (cst_last_kernel_name: "ans_encode_pc_n8_kernel" / "ans_decode_n8_kernel" /
 * "ans_decode_small_n8_kernel" and their n16 forms; 12 < P <= 24: "ans_encode_pc_n8_kernel<wide>" / "ans_decode_b16_n8_kernel").
 * Every other shape takes the conversion. */
cst_status cst_symbols_widen(const void *d_in, int32_t symbol_bytes, size_t n, int32_t *d_out, void *stream);
cst_status cst_symbols_narrow(const int32_t *d_in, size_t n, void *d_out, int32_t symbol_bytes, void *stream);
size_t cst_symbols_scratch_bytes(size_t n_streams, size_t n_per_stream, int32_t symbol_bytes);
cst_status cst_ans_encode_batch_sym(const cst_model *model, cst_coder_config cfg, const void *d_symbols, int32_t symbol_bytes,
                                    size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                    size_t stride_words, uint32_t *d_n_words, uint64_t *d_state, int32_t *d_status,
                                    uint32_t flags, void *d_scratch, void *stream);
cst_status cst_ans_decode_batch_sym(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                    const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                    const uint32_t *d_n_words, void *d_symbols, int32_t symbol_bytes, size_t n_streams,
                                    size_t n_per_stream, cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                    int32_t *d_status, uint32_t flags, void *d_scratch, void *stream);

/* Streams of DIFFERENT lengths -- thousands of small coders with a shared model in one launch: the reference's "compressed
 * index" pattern (tests/issue52.rs:27-60, 63-80: one DefaultAnsCoder per document, `encode_symbol` per character last to
 * first, `into_compressed`; `from_compressed` + `decode_symbol` per document), which costs one device round trip per document
 * through the single-coder binding.
 *     symbols of stream s = d_symbols[d_sym_offsets[s] .. d_sym_offsets[s + 1])      (d_sym_offsets: uint64 [n_streams + 1])
 *     slab of stream s    = d_words[d_word_offsets[s] .. d_word_offsets[s + 1])      (uint64 [n_streams + 1]; a slab of
 *                           cst_ans_max_words(length of s, cfg) words always suffices), or, with d_word_offsets = NULL,
 *                           d_words[s * stride_words .. + stride_words)
 * Every stream's words, count and status are those of cst_ans_encode_batch / the reference coder for that stream alone; the
 * decoder takes the same offsets (only d_word_offsets[s] and d_n_words[s] are read) or a packed layout, with the bounds
 * check of cst_ans_decode_batch.  Stream-major symbols.  A wave of 64 consecutive streams runs as long as its longest one.
 * The model has one shared table (any preset), or ONE TABLE PER STREAM (cst_model_create_gaussian_per_stream /
 * cst_model_create_tables_per_stream, e.g. rows fitted per document from cst_count_symbols_per_stream with d_sym_offsets): table s
 * codes stream s, and every stream's words are those of cst_ans_encode_batch with that per-stream model for that stream alone.
 * With a per-stream model n_tables must equal n_streams, the presets are (32,64) and (16,32), P <= 16, and the tables of a
 * workgroup live in LDS (a support too large for that is CST_ERR_INVALID_ARGUMENT, as in cst_ans_encode_batch); all of
 * cst_ans_{encode,decode}_ragged[_ordered] and cst_ans_{encode,decode}_ragged_jump take such a model (cst_last_kernel_name:
 * "ans_{encode,decode}_ragged_ps_kernel", with "<jump>" appended by the jump calls). */
cst_status cst_ans_encode_ragged(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                 const uint64_t *d_sym_offsets, size_t n_streams, uint32_t *d_words,
                                 const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                 int32_t *d_status, void *stream);
cst_status cst_ans_decode_ragged(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                 const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                 const uint32_t *d_n_words, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                 size_t n_streams, int32_t *d_status, void *stream);
/* The reference's index stores no lengths: a document ends where its terminator symbol is decoded
 * (tests/issue52.rs:63-80, `core::iter::from_fn(|| { let id = coder.decode_symbol(..); alphabet.get(id) })`).  This is
 * the first pass of that: every stream is decoded until `eof_symbol` appears, nothing is stored but the number of
 * symbols decoded, terminator included (d_lengths, uint64 [n_streams]); a stream without a terminator among its first
 * `max_symbols` symbols reports CST_STREAM_CAPACITY and max_symbols.  An exclusive prefix sum of d_lengths is the
 * d_sym_offsets of cst_ans_decode_ragged.  Shared-table models only: a per-stream model is CST_ERR_INVALID_ARGUMENT. */
cst_status cst_ans_count_until(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                               const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                               const uint32_t *d_n_words, size_t n_streams, int32_t eof_symbol, size_t max_symbols,
                               uint64_t *d_lengths, int32_t *d_status, void *stream);

/* ABI 5: jump points for ragged batches.  A launch of many small coders lasts as long as its LONGEST document's chain (100 000
 * documents of 20 .. 2000 symbols decode in 0.61 ms however few they are: 2000 dependent steps).  The reference's own remedy is the jump
 * table of Pos / Seek (src/stream/stack.rs:1107-1139): the encoder notes AnsCoder::pos() -- (words in the bulk, coder state) -- in front
 * of every chunk of `jump_interval` symbols of every stream (a multiple of 8) on its way, the words are those of cst_ans_encode_ragged,
 * and the decoder runs every chunk as a coder of its own (AnsCoder::seek + at most jump_interval symbols): the longest chain is
 * jump_interval steps.  Chunk j of stream s is entry d_chunk_offsets[s] + j of d_jump_pos / d_jump_state, with
 * d_chunk_offsets[n_streams + 1] the exclusive prefix sum of ceil(length / jump_interval) (n_chunks_total = its last entry).  The
 * decoder writes one status per STREAM (the worst of its chunks'; a table that does not describe its stream, or a jump point with more
 * words than the stream has, reports CST_STREAM_INVALID_DATA).  d_scratch: cst_ragged_jump_scratch_bytes(n_chunks_total) bytes.
 * Both calls take a per-stream model as cst_ans_{encode,decode}_ragged do (n_tables == n_streams): the encoder's table is the one
 * the reference's AnsCoder gives under that stream's table, and every chunk lane of the decoder holds its own copy of the row of the
 * stream that owns its chunk (found on the device from d_chunk_offsets: a table entry no stream owns decodes nothing). */
size_t cst_ragged_jump_scratch_bytes(size_t n_chunks_total);
cst_status cst_ans_encode_ragged_jump(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                      const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order, uint32_t *d_words,
                                      const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                      size_t jump_interval, const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos,
                                      uint64_t *d_jump_state, int32_t *d_status, void *stream);
cst_status cst_ans_decode_ragged_jump(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                      const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                      const uint32_t *d_n_words, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                      size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                      size_t n_chunks_total, const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                      void *d_scratch, int32_t *d_status, void *stream);

/* The same three calls with a SCHEDULE: lane slot i of the launch codes stream d_order[i] (uint32 [n_streams], a permutation of
 * 0 .. n_streams - 1; NULL = the identity, i.e. the calls above).  A wave of 64 slots runs as long as its longest stream, so a
 * batch whose lengths differ by orders of magnitude should put streams of similar length side by side, longest first:
 * d_order = the stream indices sorted by length (or, for the decoders, by d_n_words) in descending order.  Results (words,
 * counts, symbols, status, all indexed by STREAM as above) do not depend on the order; an entry that is not a stream index
 * leaves its slot idle, a stream that no entry names is not coded.  1 000 000 documents of 20 .. 2000 symbols: encode
 * 2.0 -> 1.3 ms, decode 4.9 -> 1.4 ms (scripts/bench_ragged_big.py).  The two coding calls take a per-stream model
 * (n_tables == n_streams; a lane's table is that of the stream its slot names); cst_ans_count_until_ordered does not. */
cst_status cst_ans_encode_ragged_ordered(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                         const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                         uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                         uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_ragged_ordered(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                         const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                         const uint32_t *d_n_words, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                         size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_ans_count_until_ordered(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                       const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                       const uint32_t *d_n_words, size_t n_streams, const uint32_t *d_order,
                                       int32_t eof_symbol, size_t max_symbols, uint64_t *d_lengths, int32_t *d_status,
                                       void *stream);

/* Per-symbol quantized Gaussians for streams of DIFFERENT lengths: cst_ans_{encode,decode}_gaussian_batch with the indexing of
 * the ragged calls above -- what a learned codec has in a batch of images, crops or tensors of different sizes, every latent with
 * its own (mean, std).
 *     symbols, means, stds of stream s = d_symbols / d_means / d_stds [d_sym_offsets[s] .. d_sym_offsets[s + 1])   (all three flat,
 *                                        f64 parameters, d_sym_offsets: uint64 [n_streams + 1])
 *     slabs, d_word_offsets / stride_words / words_capacity / d_n_words: exactly as in cst_ans_{encode,decode}_ragged (the bounds
 *                                        check included; a slab whose offsets run backwards reports CST_STREAM_CAPACITY).  A slab of
 *                                        min(n, ceil(n P / W)) + S / W words always suffices for a stream of n symbols.
 *     d_order                            as in the *_ragged_ordered calls: lane slot i codes stream d_order[i]; NULL = the identity.
 * Words, count and status of every stream are those of the reference coder -- and of cst_ans_encode_gaussian_batch -- for that
 * stream alone, bit for bit; std <= 0, a non-finite parameter or a symbol outside [min_symbol, max_symbol] flags that one stream
 * CST_STREAM_IMPOSSIBLE_SYMBOL (n_words = 0); a stream of length 0 yields 0 words and CST_STREAM_OK.  Presets (32,64) and (16,32),
 * any precision the rectangular calls take.  CST_ERR_INVALID_ARGUMENT, before the device is touched: a NULL symbols / means / stds /
 * sym_offsets / words / n_words / status pointer, an unsupported configuration, max_symbol <= min_symbol, d_word_offsets == NULL
 * with stride_words == 0.  n_streams == 0: CST_OK, nothing is launched.  One kernel each for every batch size: built for many
 * streams (from ~16 000 on); a handful of streams is coded correctly but leaves most of the device idle. */
cst_status cst_ans_encode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                          const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                          const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                          uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                          uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_encode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                              const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                              const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                              uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                              uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                          const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                          size_t words_capacity, const uint32_t *d_n_words, const double *d_means,
                                          const double *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                          size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_ans_decode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                              const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                              size_t words_capacity, const uint32_t *d_n_words, const void *d_means,
                                              const void *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                              size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);

/* ... the same pair for the range coder (a queue: the decoder reads the symbols in the order they were written), and both coders
 * over QuantizedLaplace / QuantizedCauchy.  Arguments, checks, statuses and the order / word_offsets conventions are those of
 * cst_ans_{encode,decode}_gaussian_ragged; words, count and status of every stream are those of the reference RangeEncoder /
 * AnsCoder -- and of the rectangular cst_{ans,range}_{encode,decode}_{gaussian,family}_batch -- for that stream alone.
 *     range coder slabs                  min(n, ceil(n P / W)) + 2 words always suffice for a stream of n symbols (the bound inside
 *                                        cst_range_max_words); a stream of length 0 yields 0 words and CST_STREAM_OK.
 *     family                             CST_FAMILY_LAPLACE (d_a = means, d_b = scales) or CST_FAMILY_CAUCHY (d_a = locs, d_b =
 *                                        scales), as in cst_ans_encode_family_batch; anything else: CST_ERR_INVALID_ARGUMENT.
 * Jump points: cst_{ans,range}_{encode,decode}_{gaussian,family}_ragged_jump below. */
cst_status cst_range_encode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                            const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                            const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                            uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                            uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_encode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                                const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_decode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                            const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                            size_t words_capacity, const uint32_t *d_n_words, const double *d_means,
                                            const double *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                            size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_range_decode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                size_t words_capacity, const uint32_t *d_n_words, const void *d_means,
                                                const void *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                                size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_ans_encode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                        const int32_t *d_symbols, const double *d_a, const double *d_b,
                                        const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                        uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                        uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_encode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                            const int32_t *d_symbols, const void *d_a, const void *d_b,
                                            const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                            uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                            uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                        const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                        size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                        const double *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                        size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_ans_decode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                            const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                            size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                            const void *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                            size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_range_encode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                          const int32_t *d_symbols, const double *d_a, const double *d_b,
                                          const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                          uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                          uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_encode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                              const int32_t *d_symbols, const void *d_a, const void *d_b,
                                              const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                              uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                              uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_decode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                          const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                          size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                          const double *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                          size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_range_decode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                              const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                              size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                              const void *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                              size_t n_streams, const uint32_t *d_order, int32_t *d_status, void *stream);

/* Jump points (the reference's Pos / Seek: src/stream/stack.rs:1107-1139, src/stream/queue.rs:172-196, 900-926) for the eight calls above.
 * Their decoders are chains -- one lane walks one stream, a launch lasts as long as its longest stream -- so the encoder notes the
 * coder's pos() in front of every chunk of `jump_interval` symbols of every stream on its way, and the decoder runs every chunk as a
 * coder of its own (seek + at most jump_interval symbols) on a lane of its own: the longest chain is jump_interval steps.
 *   - jump_interval: a positive multiple of 16 (the encoder codes in tiles of 16 symbols), at most 2^31 - 1.
 *   - Chunk j of stream s is entry d_chunk_offsets[s] + j of the table arrays; d_chunk_offsets[n_streams + 1] (uint64, read by both calls)
 *     is the exclusive prefix sum of ceil(length / jump_interval) -- the layout of cst_{ans,range}_{encode,decode}_ragged_jump.  Table
 *     arrays are uint32 d_jump_pos and uint64 d_jump_state (ANS) or uint64 d_jump_lower / d_jump_range (range) for both presets.
 *       ANS    d_jump_pos = words in the bulk, d_jump_state = the coder state once the symbols from the chunk's first on are encoded
 *              (AnsCoder::pos()): chunk 0 is (the words in the bulk: n_words - S / W where the state fills S / W words, the final state).
 *       range  d_jump_pos = words emitted so far INCLUDING held-back ones, d_jump_lower / d_jump_range = the RangeCoderState before the
 *              chunk's first symbol is encoded (RangeEncoder::pos()): chunk 0 is (0, 0, all ones of the state width).
 *     No chunk starts at the end of a stream.  The entries of a stream whose status is not CST_STREAM_OK are unspecified.
 *   - Encoder: the arguments of the plain call (d_order included), then the interval and the table; words, d_n_words and d_status are
 *     exactly those of the plain call.
 *   - Decoder: the arguments of the plain call WITHOUT d_order (chunks are at most jump_interval long: nothing to schedule), then the
 *     interval, the table (const) and d_scratch of cst_persymbol_ragged_jump_scratch_bytes(n_chunks_total) bytes.  n_chunks_total: the
 *     entries of the table arrays; d_chunk_offsets[n_streams] or any upper bound of it (entries behind the last chunk decode nothing).
 *   - An ANS chunk reads the words in front of its jump point.  A range chunk reads forward from its jump point, on past its chunk if
 *     need be, never past its stream's d_n_words.  The slice of every stream is checked as the plain decoder checks it.
 *   - One status per STREAM: the worst of its chunks'.  A table that does not describe its stream (chunks != ceil(length /
 *     jump_interval), offsets beyond n_chunks_total) or a d_jump_pos beyond the stream's d_n_words reports CST_STREAM_INVALID_DATA for
 *     that stream; the others decode, and nothing outside words_capacity or the stream's own symbols is touched, whatever the table holds.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: every refusal of the plain call; jump_interval 0, not a multiple of 16 or
 *     > 2^31 - 1; n_chunks_total > 2^32 - 1; a NULL d_chunk_offsets, table array or d_scratch; an unknown family.  n_streams == 0: CST_OK,
 *     nothing is launched.
 * cst_last_kernel_name(): {ans,range}_{encode,decode}_{gaussian,laplace,cauchy}_ragged_kernel<jump>. */
size_t cst_persymbol_ragged_jump_scratch_bytes(size_t n_chunks_total);
cst_status cst_ans_encode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                               const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                               const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                               uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                               uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                               uint32_t *d_jump_pos, uint64_t *d_jump_state, int32_t *d_status,
                                               void *stream);
cst_status cst_ans_encode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                   const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                                   const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                   uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                   uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                   uint32_t *d_jump_pos, uint64_t *d_jump_state, int32_t *d_status,
                                                   void *stream);
cst_status cst_ans_decode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                               const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                               size_t words_capacity, const uint32_t *d_n_words, const double *d_means,
                                               const double *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                               size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                               size_t n_chunks_total, const uint32_t *d_jump_pos,
                                               const uint64_t *d_jump_state, void *d_scratch, int32_t *d_status,
                                               void *stream);
cst_status cst_ans_decode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                   const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                   size_t words_capacity, const uint32_t *d_n_words, const void *d_means,
                                                   const void *d_stds, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                   size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                   const uint64_t *d_jump_state, void *d_scratch, int32_t *d_status,
                                                   void *stream);
cst_status cst_range_encode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                 const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                                 const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                 uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                 uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                 uint32_t *d_jump_pos, uint64_t *d_jump_lower, uint64_t *d_jump_range,
                                                 int32_t *d_status, void *stream);
cst_status cst_range_encode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                     const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                                     const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                     uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                     uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                     uint32_t *d_jump_pos, uint64_t *d_jump_lower, uint64_t *d_jump_range,
                                                     int32_t *d_status, void *stream);
cst_status cst_range_decode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                 const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                 size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                 const double *d_means, const double *d_stds, int32_t *d_symbols,
                                                 const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                 const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                 const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status,
                                                 void *stream);
cst_status cst_range_decode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                     const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                     size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                     const void *d_means, const void *d_stds, int32_t *d_symbols,
                                                     const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                     const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                     const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status,
                                                     void *stream);
cst_status cst_ans_encode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                             const int32_t *d_symbols, const double *d_a, const double *d_b,
                                             const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                             uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                             uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                             uint32_t *d_jump_pos, uint64_t *d_jump_state, int32_t *d_status, void *stream);
cst_status cst_ans_encode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                 const int32_t *d_symbols, const void *d_a, const void *d_b,
                                                 const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                 uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                 uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                 uint32_t *d_jump_pos, uint64_t *d_jump_state, int32_t *d_status, void *stream);
cst_status cst_ans_decode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                             const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                             size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                             const double *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                             size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                             size_t n_chunks_total, const uint32_t *d_jump_pos,
                                             const uint64_t *d_jump_state, void *d_scratch, int32_t *d_status,
                                             void *stream);
cst_status cst_ans_decode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                 const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                 size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                                 const void *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                                 size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                 size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                 const uint64_t *d_jump_state, void *d_scratch, int32_t *d_status,
                                                 void *stream);
cst_status cst_range_encode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                               const int32_t *d_symbols, const double *d_a, const double *d_b,
                                               const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                               uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                               uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                               uint32_t *d_jump_pos, uint64_t *d_jump_lower, uint64_t *d_jump_range,
                                               int32_t *d_status, void *stream);
cst_status cst_range_encode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                   const int32_t *d_symbols, const void *d_a, const void *d_b,
                                                   const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                   uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                   uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                   uint32_t *d_jump_pos, uint64_t *d_jump_lower, uint64_t *d_jump_range,
                                                   int32_t *d_status, void *stream);
cst_status cst_range_decode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                               const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                               size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                               const double *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                               size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                               size_t n_chunks_total, const uint32_t *d_jump_pos,
                                               const uint64_t *d_jump_lower, const uint64_t *d_jump_range, void *d_scratch,
                                               int32_t *d_status, void *stream);
cst_status cst_range_decode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                   const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                   size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                                   const void *d_b, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                   size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                   const uint64_t *d_jump_lower, const uint64_t *d_jump_range, void *d_scratch,
                                                   int32_t *d_status, void *stream);

/* Random access into a ragged per-symbol batch: cst_{ans,range}_decode_ragged_select (below, where queries, pieces, d_out_offsets,
 * d_piece_offsets and the per-query statuses are described) for the eight decoders above.  The arguments are the model's (cfg, the
 * family, min_symbol, max_symbol), then the words block, d_means / d_stds (d_a / d_b) -- the batch's FULL arrays, laid out exactly as
 * the plain decode call takes them -- d_sym_offsets and n_streams, then the table block and the query block of
 * cst_{ans,range}_decode_ragged_select with the same conventions: jump_interval 0 and every table pointer NULL is no table; both of
 * d_query_first / d_query_count NULL is whole documents; n_queries == 0 returns CST_OK and launches nothing.
 *   - A piece reads its parameters from the element of its jump point on: element d_sym_offsets[s] + (first / jump_interval + j) *
 *     jump_interval for piece j of a query, d_sym_offsets[s] without a table.  The symbols in front of `first` are decoded with their
 *     own parameters and dropped.  ONLY the parameters of elements [that first element, d_sym_offsets[s] + first + count) of a query can
 *     influence any result or status: everything else in d_means / d_stds may hold anything (NaN included).
 *   - Statuses, one per QUERY: CST_STREAM_INVALID_DATA (nothing is written) for every query cst_{ans,range}_decode_ragged_select refuse.
 *     A query whose decoded range, the dropped symbols included, meets an invalid model or an impossible quantile reports
 *     CST_STREAM_IMPOSSIBLE_SYMBOL and may leave anything inside its own output slice, nothing outside it; the other queries are
 *     unaffected.
 *   - d_scratch: cst_persymbol_ragged_select_scratch_bytes(n_pieces_total) bytes (a piece's record also holds where its parameters
 *     start and its coder's state at the jump point).
 *   - CST_ERR_INVALID_ARGUMENT / CST_ERR_MODEL, before the device is touched: every refusal of the plain decode call (d_symbols_out in
 *     the place of d_symbols; d_order does not exist here), a support too large for the precision included; with a table, every refusal
 *     of the _jump decoders (jump_interval not a multiple of 16 or > 2^31 - 1, a NULL d_chunk_offsets or table array, n_chunks_total >
 *     2^32 - 1); table arrays without an interval; n_pieces_total > 2^32 - 1; exactly one of d_query_first / d_query_count NULL; with
 *     n_queries > 0 a NULL d_query_stream, d_piece_offsets, d_out_offsets or d_scratch; an unknown family.
 * cst_last_kernel_name(): {ans,range}_decode_{gaussian,laplace,cauchy}_ragged_kernel<select>.  (The Categorical ragged decoders:
 * cst_{ans,range}_decode_categorical[_perfect]_ragged_select, with those calls.) */
size_t cst_persymbol_ragged_select_scratch_bytes(size_t n_pieces_total);
cst_status cst_ans_decode_gaussian_ragged_select(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                 const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                 size_t words_capacity, const uint32_t *d_n_words, const double *d_means,
                                                 const double *d_stds, const uint64_t *d_sym_offsets, size_t n_streams,
                                                 size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                                 const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                 const uint64_t *d_query_count, size_t n_queries,
                                                 const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                 const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status,
                                                 void *stream);
cst_status cst_ans_decode_gaussian_ragged_select_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                     const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                     size_t words_capacity, const uint32_t *d_n_words, const void *d_means,
                                                     const void *d_stds, const uint64_t *d_sym_offsets, size_t n_streams,
                                                     size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                                     const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                     const uint64_t *d_query_count, size_t n_queries,
                                                     const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                     const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status,
                                                     void *stream);
cst_status cst_range_decode_gaussian_ragged_select(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                   const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                   size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                   const double *d_means, const double *d_stds, const uint64_t *d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                   size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                   const uint64_t *d_jump_lower, const uint64_t *d_jump_range,
                                                   const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                   const uint64_t *d_query_count, size_t n_queries,
                                                   const uint64_t *d_piece_offsets, size_t n_pieces_total,
                                                   int32_t *d_symbols_out, const uint64_t *d_out_offsets, void *d_scratch,
                                                   int32_t *d_status, void *stream);
cst_status cst_range_decode_gaussian_ragged_select_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                       const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                       size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                       const void *d_means, const void *d_stds, const uint64_t *d_sym_offsets,
                                                       size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                       size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                       const uint64_t *d_jump_lower, const uint64_t *d_jump_range,
                                                       const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                       const uint64_t *d_query_count, size_t n_queries,
                                                       const uint64_t *d_piece_offsets, size_t n_pieces_total,
                                                       int32_t *d_symbols_out, const uint64_t *d_out_offsets, void *d_scratch,
                                                       int32_t *d_status, void *stream);
cst_status cst_ans_decode_family_ragged_select(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                               const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                               size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                               const double *d_b, const uint64_t *d_sym_offsets, size_t n_streams,
                                               size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                               const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                               const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                               const uint64_t *d_query_count, size_t n_queries,
                                               const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                               const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_ans_decode_family_ragged_select_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                   const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                   size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                                   const void *d_b, const uint64_t *d_sym_offsets, size_t n_streams,
                                                   size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                   const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                                   const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                   const uint64_t *d_query_count, size_t n_queries,
                                                   const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                   const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_range_decode_family_ragged_select(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                 const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                 size_t words_capacity, const uint32_t *d_n_words, const double *d_a,
                                                 const double *d_b, const uint64_t *d_sym_offsets, size_t n_streams,
                                                 size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                 const uint64_t *d_jump_range, const uint32_t *d_query_stream,
                                                 const uint64_t *d_query_first, const uint64_t *d_query_count, size_t n_queries,
                                                 const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                 const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status,
                                                 void *stream);
cst_status cst_range_decode_family_ragged_select_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                     const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                     size_t words_capacity, const uint32_t *d_n_words, const void *d_a,
                                                     const void *d_b, const uint64_t *d_sym_offsets, size_t n_streams,
                                                     size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                     const uint64_t *d_jump_range, const uint32_t *d_query_stream,
                                                     const uint64_t *d_query_first, const uint64_t *d_query_count, size_t n_queries,
                                                     const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                     const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status,
                                                     void *stream);

/* The range coder for streams of different lengths, with ONE SHARED TABLE or one table per stream: cst_ans_{encode,decode}_ragged / cst_ans_count_until for the
 * reference's queue -- one RangeEncoder / RangeDecoder per document (src/stream/queue.rs), the symbols decoded in the order they were
 * encoded, so that a terminator is simply written last.  Symbols, slabs, d_word_offsets / stride_words / words_capacity / d_n_words
 * and d_order (NULL = the identity; an entry that is no stream index idles its slot) are those of the ragged calls above.
 *   - Words, count and status of every stream are those of the reference RangeEncoder / RangeDecoder for that stream alone, bit for
 *     bit -- and those of cst_range_{encode,decode}_batch.
 *   - A slab of min(n, ceil(n P / W)) + 2 words always suffices for a stream of n symbols (checked against the CPU oracle for
 *     n = 0 .. 70, 255 .. 257 and 700 at about P bits per symbol on six presets: the oracle stays one word below the bound).  A slab
 *     whose offsets run backwards is a slab of no words: CST_STREAM_CAPACITY, nothing written.
 *   - A stream of length 0 yields 0 words and CST_STREAM_OK.
 *   - An impossible symbol flags its stream only: CST_STREAM_IMPOSSIBLE_SYMBOL, n_words = 0.
 *   - Corrupt counts or offsets on the decoder side give CST_STREAM_INVALID_DATA and nothing outside words_capacity is read (the
 *     bounds check of cst_range_decode_batch).
 *   - cst_range_count_until: every stream is decoded until `eof_symbol` appears; d_lengths[s] = symbols decoded, terminator included.
 *     A range decoder that has run out of words keeps decoding (the reference shifts in zeros), so `max_symbols` is the only stop
 *     for a stream without a terminator: it reports CST_STREAM_CAPACITY and max_symbols.  An exclusive prefix sum of d_lengths is the
 *     d_sym_offsets of cst_range_decode_ragged.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: a NULL model or a NULL sym_offsets / words (encoder) / n_words /
 *     lengths / status pointer, an unsupported configuration, cfg.precision != the model's (as cst_range_encode_batch refuses it), a
 *     per-stream model whose n_tables != n_streams (cst_range_count_until: any per-stream model), d_word_offsets == NULL with
 *     stride_words == 0, n_streams > 2^32 - 1 with an order.
 *   - n_streams == 0: CST_OK, nothing is launched.
 *   - One table per stream (cst_model_create_gaussian_per_stream / cst_model_create_tables_per_stream with as many tables as
 *     streams): cst_range_{encode,decode}_ragged and cst_range_{encode,decode}_ragged_jump code stream s with table s -- the words of
 *     the reference RangeEncoder over that stream's table, those of cst_range_encode_batch with the per-stream model.  P <= 16; the
 *     tables of a workgroup live in LDS, a support too large for that is CST_ERR_INVALID_ARGUMENT.  cst_last_kernel_name:
 *     "range_{encode,decode}_ragged_ps_kernel", with "<jump>" appended by the jump calls.  cst_range_count_until,
 *     cst_range_decode_ragged_select and cst_ans_decode_ragged_select keep refusing such a model.
 * Presets (32,64) and (16,32), every precision cst_range_encode_batch takes.
 *
 * Jump points (RangeEncoder::pos / RangeDecoder::seek, src/stream/queue.rs:172-196, 900-926) -- cst_range_{encode,decode}_ragged_jump,
 * the counterparts of cst_ans_{encode,decode}_ragged_jump: a launch lasts as long as its longest document's chain, and a range step
 * (its quantile is a quotient) costs more than an ANS step.  The encoder notes RangeEncoder::pos() in front of every chunk of
 * `jump_interval` symbols (a multiple of 8) of every stream on its way; words, d_n_words and d_status are exactly those of
 * cst_range_encode_ragged.  The decoder runs every chunk as a coder of its own (seek + at most jump_interval symbols) on a lane of its
 * own: the longest chain is jump_interval steps.
 *   - Chunk j of stream s is entry d_chunk_offsets[s] + j of the three table arrays, d_chunk_offsets[n_streams + 1] (uint64, read by both
 *     calls) the exclusive prefix sum of ceil(length / jump_interval) -- the layout of the ANS calls.  A jump point is d_jump_pos (uint32:
 *     words emitted so far INCLUDING held-back ones, as d_ckpt_pos of cst_range_encode_batch_ckpt), d_jump_lower / d_jump_range (uint64
 *     for both presets: the RangeCoderState there).  Chunk 0 is (0, 0, all ones); no chunk starts at the end of a stream.  The table
 *     entries of a stream whose status is not CST_STREAM_OK are unspecified.
 *   - n_chunks_total: the entries of the table arrays; d_chunk_offsets[n_streams] or any upper bound of it (entries behind the last chunk
 *     decode nothing).  d_scratch: cst_range_ragged_jump_scratch_bytes(n_chunks_total) bytes.
 *   - A chunk reads forward from its jump point, on past its chunk if need be, never past its stream's d_n_words; the slice of every
 *     stream is checked as cst_range_decode_ragged checks it.  One status per STREAM: the worst of its chunks'.  A table that does not
 *     describe its stream (chunks != ceil(length / jump_interval), offsets beyond n_chunks_total) or a d_jump_pos beyond the stream's
 *     d_n_words reports CST_STREAM_INVALID_DATA for that stream; the others decode, and nothing outside words_capacity or the stream's
 *     own symbols is touched.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: every refusal of cst_range_{encode,decode}_ragged (the decoder takes no
 *     order), jump_interval 0, not a multiple of 8 or > 2^31 - 1, n_chunks_total > 2^32 - 1, a NULL d_chunk_offsets / d_jump_pos /
 *     d_jump_lower / d_jump_range / d_scratch.  n_streams == 0: CST_OK, nothing is launched. */
cst_status cst_range_encode_ragged(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                   const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order, uint32_t *d_words,
                                   const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words, int32_t *d_status,
                                   void *stream);
cst_status cst_range_decode_ragged(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                   const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                   const uint32_t *d_n_words, int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                   const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_range_count_until(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                 const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                 const uint32_t *d_n_words, size_t n_streams, const uint32_t *d_order, int32_t eof_symbol,
                                 size_t max_symbols, uint64_t *d_lengths, int32_t *d_status, void *stream);
size_t cst_range_ragged_jump_scratch_bytes(size_t n_chunks_total);
cst_status cst_range_encode_ragged_jump(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                        const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order, uint32_t *d_words,
                                        const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                        size_t jump_interval, const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos,
                                        uint64_t *d_jump_lower, uint64_t *d_jump_range, int32_t *d_status, void *stream);
cst_status cst_range_decode_ragged_jump(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                        const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                        const uint32_t *d_n_words, int32_t *d_symbols, const uint64_t *d_sym_offsets,
                                        size_t n_streams, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                        size_t n_chunks_total, const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                        const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status, void *stream);

/* Random access into a ragged batch -- what the reference's `Seek` is FOR (src/stream/stack.rs:1107-1139, queue.rs:900-926): decode
 * selected documents, or ranges of documents, and nothing else.  cst_ans_decode_ragged_select / cst_range_decode_ragged_select take the
 * batch exactly as cst_{ans,range}_decode_ragged[_jump] take it (words, d_word_offsets or stride_words, words_capacity, d_n_words,
 * d_sym_offsets, and optionally a jump table) and a list of n_queries queries:
 *     query q = symbols [d_query_first[q], d_query_first[q] + d_query_count[q]) of document d_query_stream[q]
 *     (d_query_stream uint32 [n_queries]; d_query_first / d_query_count uint64 [n_queries], or BOTH NULL: whole documents)
 * in any order, repeats and overlaps allowed, count 0 allowed.  The output is a ragged array of its own: query q owns
 * d_symbols_out[d_out_offsets[q] .. d_out_offsets[q + 1]) (d_out_offsets uint64 [n_queries + 1], the exclusive prefix sum of the counts)
 * and receives exactly the symbols a full decode puts at d_sym_offsets[stream] + first ...; d_status holds one entry per QUERY.
 *   - With a jump table (jump_interval a positive multiple of 8, d_chunk_offsets / n_chunks_total / d_jump_pos / d_jump_state or
 *     d_jump_lower + d_jump_range as the jump decoders take them) a query is cut into PIECES, one per chunk it touches:
 *     ceil((first % jump_interval + count) / jump_interval) for count > 0, none for count 0.  The first piece starts at jump point
 *     first / jump_interval, decodes and DISCARDS first % jump_interval symbols, then stores up to the chunk's or the query's end; the
 *     others are whole chunks or a chunk's head.  Every piece is one lane and at most jump_interval dependent steps.
 *   - Without a table (jump_interval 0 and every table pointer NULL; n_chunks_total is ignored) a query is ONE piece that starts where
 *     its document starts and discards `first` symbols: correct, and as slow as its `first` is deep -- this is what jump points are for.
 *   - d_piece_offsets: uint64 [n_queries + 1], the exclusive prefix sum of the piece counts (the d_chunk_offsets convention);
 *     n_pieces_total: its last entry or any upper bound of it.  d_scratch: cst_ragged_select_scratch_bytes(n_pieces_total) /
 *     cst_range_ragged_select_scratch_bytes(n_pieces_total) bytes.
 *   - Everything above is caller data and checked on the device.  A query reports CST_STREAM_INVALID_DATA and writes NOTHING if
 *     its stream is >= n_streams; first + count lies beyond the document (judged without forming the sum: no 64-bit wrap); its slice of
 *     d_out_offsets is not `count` long or its slice of d_piece_offsets not its piece count (or beyond n_pieces_total); its stream's
 *     words leave the buffer (the check of cst_{ans,range}_decode_ragged); its stream's slice of the table is not
 *     ceil(length / jump_interval) entries inside n_chunks_total; or a table entry it touches has a d_jump_pos above the stream's
 *     d_n_words.  (A document longer than 2^32 - 1 symbols: CST_STREAM_CAPACITY, as in the plain decoders.)  The other queries still
 *     decode.  Otherwise a query's status is the worst of its pieces', as a stream's is in the jump decoders; piece offsets that do not
 *     ascend may leave a query with a piece the device gave to another one: CST_STREAM_INVALID_DATA for that query.  Nothing is written
 *     outside the output slices of valid queries, nothing is read outside words_capacity.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: every refusal of cst_ans_decode_ragged / cst_range_decode_ragged; a
 *     jump_interval that is neither 0 nor a multiple of 8, or above 2^31 - 1; a table given in part (an interval without all of its
 *     arrays, arrays without an interval); n_chunks_total or n_pieces_total > 2^32 - 1; exactly one of d_query_first / d_query_count
 *     NULL; with n_queries > 0 a NULL d_query_stream, d_piece_offsets, d_out_offsets, d_scratch or d_status.  n_queries == 0: CST_OK,
 *     nothing is launched.
 * cst_last_kernel_name: "ans_decode_ragged_kernel<select>" / "range_decode_ragged_kernel<select>".  Shared-table models only (a
 * per-stream model, which the plain and jump decoders of ragged batches take, is CST_ERR_INVALID_ARGUMENT here); the
 * per-symbol ragged coders (Gaussian, Laplace, Cauchy) have cst_{ans,range}_decode_{gaussian,family}_ragged_select, where a piece also
 * carries the position its parameters start at. */
size_t cst_ragged_select_scratch_bytes(size_t n_pieces_total);
size_t cst_range_ragged_select_scratch_bytes(size_t n_pieces_total);
cst_status cst_ans_decode_ragged_select(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                        const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                        const uint32_t *d_n_words, const uint64_t *d_sym_offsets, size_t n_streams,
                                        size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                        const uint32_t *d_jump_pos, const uint64_t *d_jump_state, const uint32_t *d_query_stream,
                                        const uint64_t *d_query_first, const uint64_t *d_query_count, size_t n_queries,
                                        const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                        const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_range_decode_ragged_select(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                          const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                          const uint32_t *d_n_words, const uint64_t *d_sym_offsets, size_t n_streams,
                                          size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                          const uint32_t *d_jump_pos, const uint64_t *d_jump_lower, const uint64_t *d_jump_range,
                                          const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                          const uint64_t *d_query_count, size_t n_queries, const uint64_t *d_piece_offsets,
                                          size_t n_pieces_total, int32_t *d_symbols_out, const uint64_t *d_out_offsets,
                                          void *d_scratch, int32_t *d_status, void *stream);

/* Checkpointed streams -- the reference's Pos / Seek jump tables (src/stream/stack.rs:1107-1139; test :1456-1548) for the
 * batched coder.  The encoder notes, in front of every chunk of `ckpt_interval` symbols, what `AnsCoder::pos()` returns
 * there: d_ckpt_pos[s][j] = words in the bulk, d_ckpt_state[s][j] = coder state once symbols [j * interval, n) are
 * encoded (n_chunks = ceil(n_per_stream / interval) entries per stream).  The compressed words are exactly those of
 * cst_ans_encode_batch.  The decoder then treats every (stream, chunk) as an independent coder --
 * `AnsCoder::seek(pos, state)` + interval decoded symbols -- so that ONE long stream (BASELINE config C1) spreads over
 * n_chunks lanes: it is the ordinary batched decode of n_streams * n_chunks virtual streams (stream-major symbols,
 * shared-table models, n_per_stream a multiple of the interval; d_status has n_streams * n_chunks entries;
 * d_scratch: cst_ckpt_scratch_bytes(...) bytes, contents irrelevant).
 * ABI 4: jump points as SUB-LANES of a batch.  Many streams gain from them too: a decoder of 65 536 streams runs one wave per
 * SIMD and waits for its table lookups; with k = n_per_stream / interval jump points per stream the same words decode on k
 * lanes per stream, two waves per SIMD.  Models with one table per stream (config C3; stream-major, the compact-row shapes of
 * cst_model_create_gaussian_per_stream) are taken by both calls: the encoder notes the jump points at the speed of
 * cst_ans_encode_batch when the chunks are whole 32-symbol tiles, the decoder runs k = 2, 4, 8 or 16 lanes per stream that
 * share the stream's table in on-chip memory.  Any other k decodes the streams whole: the jump points are side information,
 * the symbols and the per-chunk status (the stream's status, repeated) are the same. */
cst_status cst_ans_encode_batch_ckpt(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                     size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                     size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                     uint32_t *d_ckpt_pos, uint64_t *d_ckpt_state, int32_t *d_status, void *stream);
size_t cst_ckpt_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval);
/* ABI 5: the per-chunk status of a *_decode_batch_ckpt call as one status per stream (the worst of its chunks: what the plain
 * decoder of the whole stream reports in d_status[s]).  d_chunk_status[n_streams][n_chunks] -> d_stream_status[n_streams]. */
cst_status cst_ckpt_status_per_stream(const int32_t *d_chunk_status, size_t n_streams, size_t n_chunks,
                                      int32_t *d_stream_status, void *stream);
cst_status cst_ans_decode_batch_ckpt(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                     const uint64_t *d_offsets, size_t stride_words, size_t words_capacity, size_t ckpt_interval,
                                     const uint32_t *d_ckpt_pos, const uint64_t *d_ckpt_state, int32_t *d_symbols,
                                     size_t n_streams, size_t n_per_stream, void *d_scratch, int32_t *d_status,
                                     void *stream);

/* Round 5 (additions to ABI 4): jump points at the speed of the plain encoder, and for NARROW symbol matrices.
 * cst_ans_encode_batch_ckpt on a shared-table model, preset (32,64), 8 <= P <= 12, whole workgroups of 256 stream-major rows that
 * are whole aligned tiles, chunks of whole 32-symbol tiles that divide the rows: the producer / consumer encoder notes the jump
 * points on its way ("ans_encode_pc_kernel<ckpt>").  The _sym forms take symbol_bytes = 1, 2 or 4 as cst_ans_*_batch_sym do: an int8
 * matrix of whole 128-symbol lines is read by the encoder loops themselves ("ans_encode_pc_n8_kernel<ckpt>") and, chunk by chunk
 * (ckpt_interval a multiple of 128), written by the decoder loops -- k x n_streams virtual streams, two waves per SIMD from
 * 65 537 of them on ("ans_decode_small_n8_kernel"): 65 536 x 4096 at k = 2 decode in 0.17 ms against 0.24 ms whole.  Every other
 * shape converts next to the int32 calls.  d_scratch: cst_ckpt_sym_scratch_bytes(...) bytes for both calls (the encoder touches
 * it only when it converts; NULL is accepted where it does not). */
cst_status cst_ans_encode_batch_ckpt_sym(const cst_model *model, cst_coder_config cfg, const void *d_symbols, int32_t symbol_bytes,
                                         size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                         size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval, uint32_t *d_ckpt_pos,
                                         uint64_t *d_ckpt_state, int32_t *d_status, void *d_scratch, void *stream);
size_t cst_ckpt_sym_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval, int32_t symbol_bytes);
cst_status cst_ans_decode_batch_ckpt_sym(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                         const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                         size_t ckpt_interval, const uint32_t *d_ckpt_pos, const uint64_t *d_ckpt_state,
                                         void *d_symbols, int32_t symbol_bytes, size_t n_streams, size_t n_per_stream,
                                         void *d_scratch, int32_t *d_status, void *stream);

/* The same for the reference's flagship call, every symbol its own (mean, std) (cst_ans_encode_gaussian_batch): the fused encoder
 * notes the jump points (batches of at least 16 384 streams; ckpt_interval a multiple of 16 that divides n_per_stream), and the
 * decoder runs every (stream, chunk) pair as a coder of its own -- the parameter matrices have the symbols' shape, so a chunk's
 * models are a row of the [n_streams * n_chunks][interval] view of d_means / d_stds.  Stream-major.  With two jump points per
 * stream a 65 536-stream batch decodes with two resident waves per SIMD (3.4 -> 2.6 ms at 4096 symbols per stream).
 * d_scratch: cst_ckpt_scratch_bytes(...). */
cst_status cst_ans_encode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                              const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                              size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                              size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                              uint32_t *d_ckpt_pos, uint64_t *d_ckpt_state, int32_t *d_status, void *stream);
cst_status cst_ans_encode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                  const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                                  size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                                  size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                                  uint32_t *d_ckpt_pos, uint64_t *d_ckpt_state, int32_t *d_status, void *stream);
cst_status cst_ans_decode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                              const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                              size_t words_capacity, size_t ckpt_interval, const uint32_t *d_ckpt_pos,
                                              const uint64_t *d_ckpt_state, const double *d_means, const double *d_stds,
                                              int32_t *d_symbols, size_t n_streams, size_t n_per_stream, void *d_scratch,
                                              int32_t *d_status, void *stream);
cst_status cst_ans_decode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                  const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                                  size_t words_capacity, size_t ckpt_interval, const uint32_t *d_ckpt_pos,
                                                  const uint64_t *d_ckpt_state, const void *d_means, const void *d_stds,
                                                  int32_t *d_symbols, size_t n_streams, size_t n_per_stream, void *d_scratch,
                                                  int32_t *d_status, void *stream);

/* The same for the range coder: RangeEncoder::pos() / RangeDecoder::seek (src/stream/queue.rs:172-196, 900-926; test
 * :1333-1396).  A jump point is (d_ckpt_pos[s][j] = words emitted so far INCLUDING held-back ones, (d_ckpt_lower[s][j],
 * d_ckpt_range[s][j]) = RangeCoderState) in front of chunk j; seeking continues reading at word `pos`, re-reads `point` from
 * there and takes the state.  The words are exactly those of cst_range_encode_batch.  Shared-table models, any preset and
 * layout on the encoder side (the hand-scheduled (32,64) kernel for stream-major batches notes the jump points on its way);
 * the decoder wants stream-major symbols and n_per_stream a multiple of the interval, takes the whole streams' counts
 * (d_n_words: a lane reads past its chunk, never past its stream) and writes n_streams * n_chunks status entries; a jump point
 * beyond its stream's words reports CST_STREAM_INVALID_DATA for that chunk.  d_scratch: cst_range_ckpt_scratch_bytes(...).
 * One table per stream (cst_model_create_gaussian_per_stream / cst_model_create_tables_per_stream with as many tables as
 * streams): taken by both calls, stream-major only, any ckpt_interval >= 1 on the encoder side ("range_encode_ps_kernel<ckpt>");
 * the decoder runs one lane per chunk, each with its own copy of its stream's row ("range_decode_ps_kernel<chunks>"). */
cst_status cst_range_encode_batch_ckpt(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                       size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                       size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                       uint32_t *d_ckpt_pos, uint64_t *d_ckpt_lower, uint64_t *d_ckpt_range,
                                       int32_t *d_status, void *stream);
size_t cst_range_ckpt_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval);
cst_status cst_range_decode_batch_ckpt(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                       const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                       const uint32_t *d_n_words, size_t ckpt_interval, const uint32_t *d_ckpt_pos,
                                       const uint64_t *d_ckpt_lower, const uint64_t *d_ckpt_range, int32_t *d_symbols,
                                       size_t n_streams, size_t n_per_stream, void *d_scratch, int32_t *d_status,
                                       void *stream);

/* ABI 5: which jump points should a batch carry?  Jump points never change a stream's words; what they buy is lanes -- k jump
 * points per stream let the same words decode on k lanes, and every decoder of this library except the int32 shared-table one
 * (P <= 12) is latency-bound at one wave of streams per SIMD.  The library's own answer for a batch about to be
 * ENCODED with the given arguments (the same meaning as in cst_ans_encode_batch_sym / cst_range_encode_batch; symbol_bytes = 1, 2
 * or 4; d_symbols / d_words / stride_words are looked at for alignment only):
 *   returns the ckpt_interval to pass to cst_ans_encode_batch_ckpt[_sym] / cst_range_encode_batch_ckpt and to the matching
 *   *_decode_batch_ckpt call, or 0 = carry none (the plain decoder is as fast, or the shape is not one the checkpointing encoders
 *   take at the plain encoders' speed).
 * coder: CST_CODER_ANS or CST_CODER_RANGE.  cst_jump_points_auto_gaussian: the same for cst_ans_encode_gaussian_batch_ckpt (every
 * symbol its own mean and std).  The Python layer (constriction_amd.batched, jump_points="auto", the default) and the Rust
 * wrappers ask here; CST_AUTO_JUMP=0 in the environment makes both answer 0. */
#define CST_CODER_ANS 0
#define CST_CODER_RANGE 1
size_t cst_jump_points_auto(const cst_model *model, cst_coder_config cfg, int32_t coder, int32_t symbol_bytes,
                            const void *d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                            const void *d_words, size_t stride_words);
size_t cst_jump_points_auto_gaussian(cst_coder_config cfg, int32_t coder, size_t n_streams, size_t n_per_stream,
                                     cst_layout layout);

/* Debug switches (ABI 5).  The dispatcher's A/B switches are environment variables read ONCE, when the library is loaded --
 * no coder call reads the environment.  Each selects among kernels that produce the same words and symbols (the parity suite
 * runs under every one of them, scripts/alt_paths.sh):
 *   CST_NO_PC_ENCODER=1      never the producer / consumer encoders          CST_NO_PC_WIDE=1   12 < P <= 24 on ans_encode_wide_kernel
 *   CST_PC_COMBINED=1        their helper waves load AND store                CST_NO_N8=1        narrow matrices through the conversion kernels
 *   CST_SMALL_KERNELS=0|enc|dec   never / only the encoder / only the decoder of the small-footprint kernels
 *   CST_DQ_DECODER=1         the lane-quad decoder without CST_FLAG_COLD_WORDS CST_PT_SUB_WAVES=8 sub-lane decoder: never sixteen waves
 *   CST_SUB_ORDER=0          range sub-lane decoder: chunks side by side      CST_LANE_GEO=big|small   per-symbol lane decoder geometry
 *   CST_FUSED_MIN_STREAMS=n  from how many streams the fused per-symbol encoder runs         CST_CATEGORICAL_ROUTE=fused|rows   per-symbol Categorical decoders: the route
 *   CST_AUTO_JUMP=0          cst_jump_points_auto* answer 0                  CST_RAGGED_GROUP=8|16|32   ragged encoder: symbols per memory point
 *   CST_PERFECT_RAGGED_BUDGET=n   ragged Categorical(perfect=True) decoders: 32-bit words of tabulated rows per step (default 16777216 = 64 MiB)
 *   CST_INDEXED_BUCKET_BITS=0..8  table sets built from now on: the most bits of bucket index (default 8; 0: the indexed decoders search whole rows)
 *   CST_FIT_REPLICAS=1|2|4|8  cst_count_symbols: the most LDS replicas of a bin (default 8)      CST_FIT_WAVE_UNIFORM=0   ... no single add for a wave of one bin
 * (CST_RCCL_LIB=<path>, read at the first collective call, names the RCCL library to open.)
 * cst_debug_reload_knobs re-reads them: for tests that drive several paths inside one process; not thread-safe against
 * concurrent coder calls. */
void cst_debug_reload_knobs(void);

/* Exclusive prefix sum of d_n_words into d_offsets[n_streams+1] and gather of the slabs into one packed buffer (the
 * concatenation of every stream's `into_compressed()` result) -- ONE kernel (single-pass scan with decoupled
 * look-back, fused with the copy), fully asynchronous on `stream`: no host synchronisation, no allocation.
 *   d_offsets        out: offsets[s] = first word of stream s in the packed buffer; offsets[n_streams] = total words
 *   d_packed         may be NULL to compute the offsets only
 *   packed_capacity  words available at d_packed (an upper bound such as n_streams * stride_words always suffices);
 *                    a stream that would end beyond it is not copied -- the caller sees offsets[n_streams] > capacity
 *   d_scratch        cst_compact_scratch_bytes(n_streams) bytes of device memory, contents irrelevant on entry
 * (The reference has no counterpart: its coders each own a Vec<u32>; this is the container layout of
 *  src/pybindings/stream/stack.rs:149-166 -- little-endian u32 words, one offset per message.) */
size_t cst_compact_scratch_bytes(size_t n_streams);
cst_status cst_compact_words(const uint32_t *d_words, size_t stride_words, const uint32_t *d_n_words,
                             size_t n_streams, uint64_t *d_offsets, uint32_t *d_packed,
                             size_t packed_capacity, void *d_scratch, void *stream);
/* The same for slabs of PACKED 16-bit words (CST_FLAG_PACKED_W16): stride, counts, offsets and capacity in 16-bit words; the
 * packed buffer is the concatenation of every stream's Vec<u16>.  Two kernels (the scan of cst_compact_words + a halfword
 * gather), same scratch. */
cst_status cst_compact_words16(const uint16_t *d_words16, size_t stride_words, const uint32_t *d_n_words,
                               size_t n_streams, uint64_t *d_offsets, uint16_t *d_packed16,
                               size_t packed_capacity, void *d_scratch, void *stream);

/* cst_ans_encode_batch with CST_FLAG_PACKED_W16 + a jump point in front of every ckpt_interval symbols (ABI 5, round 6):
 * `AnsCoder::pos()` (src/stream/stack.rs:1107-1139) of the (16,32) preset whose words lie as the reference holds them, a
 * Vec<u16> -- d_ckpt_pos[s * n_chunks + j] = 16-bit words in the bulk in front of chunk j, d_ckpt_state[...] = the coder state
 * there (its low 32 bits; n_chunks = n_per_stream / ckpt_interval).  The packed encoder notes them on its way at the plain call's
 * speed; the words are the plain call's.  Stream-major, shared table, 8 <= P <= 12, chunks of whole 32-symbol tiles that divide
 * the rows -- other shapes: CST_ERR_INVALID_ARGUMENT (note the points with cst_ans_encode_batch_ckpt into a scratch slab
 * instead).  Decode from the points: cst_ans_decode_batch on the n_streams * n_chunks chunks as streams of their own --
 * d_offsets[v] = s * stride_words (16-bit words), d_n_words[v] = pos, d_state = A COPY of the states (CST_FLAG_RAW_STATE makes
 * that array in AND out), flags CST_FLAG_RAW_STATE | CST_FLAG_PACKED_W16; symbols as the matrix [n_streams * n_chunks][interval]. */
cst_status cst_ans_encode_batch_ckpt_packed16(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                              size_t n_streams, size_t n_per_stream, uint16_t *d_words16,
                                              size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                              uint32_t *d_ckpt_pos, uint64_t *d_ckpt_state, int32_t *d_status,
                                              void *stream);

/* Every stream's words in REVERSED order: out[s][i] = in[s][n_words[s] - 1 - i].  The reference reads an ANS stream from
 * its END (a stack); `AnsCoder::from_reversed_compressed` (src/stream/stack.rs:734-748) and `Cursor::into_reversed`
 * (src/backends.rs:1424-1448; docs :774-803) are its coders over words stored last-written-first, the order in which a decoder
 * consumes them -- what a file or socket that is decoded while it arrives holds.  This entry point converts a batch between the
 * two orders (it is its own inverse); the decoders of this library take the reference's default order.
 *   d_offsets_in / d_offsets_out   packed layouts (the n_streams + 1 offsets of cst_compact_words: offsets[s] = first word of
 *                                  stream s), or NULL for slabs `stride` words apart
 * In place (same buffer, same layout on both sides) is allowed.  One asynchronous kernel, a wave per stream.  A stream whose
 * count exceeds its slab (stride) or its slice of a packed buffer (offsets[s + 1] - offsets[s]) is left untouched -- counts and
 * offsets are caller data, and the decoders would report such a stream as CST_STREAM_INVALID_DATA. */
cst_status cst_words_reverse(const uint32_t *d_words_in, const uint64_t *d_offsets_in, size_t stride_in,
                             const uint32_t *d_n_words, size_t n_streams, uint32_t *d_words_out,
                             const uint64_t *d_offsets_out, size_t stride_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * multi-GPU: gather of the packed compressed words of every rank to one root over RCCL / xGMI (BASELINE config C5).
 * One process per GPU; streams shard in contiguous blocks and no collective touches the coding path; this is the only
 * exchange step.  The library opens librccl at first use (no link-time dependency); `comm` is an ncclComm_t -- the
 * caller's own, or one made with the two helpers below from an id that rank 0 creates and the caller's launcher
 * distributes (128 bytes).  (No reference counterpart: its coders are single-threaded host objects.)
 * ---------------------------------------------------------------------------------------- */
cst_status cst_rccl_get_unique_id(void *h_id /* 128 bytes out */);
cst_status cst_rccl_comm_init(const void *h_id, int32_t n_ranks, int32_t rank, void **out_comm); /* on the current device */
cst_status cst_rccl_comm_destroy(void *comm);

/* Step 1 (every rank, asynchronous on `stream`): d_sizes[2 * n_ranks] (device, uint64) receives (n_streams, total_words)
 * of every rank, in rank order; d_offsets is the rank's own offsets[n_streams_local + 1] from cst_compact_words. */
cst_status cst_gather_sizes_rccl(void *comm, int32_t n_ranks, int32_t rank, const uint64_t *d_offsets,
                                 size_t n_streams_local, uint64_t *d_sizes, void *stream);

/* Step 2 (every rank): h_sizes = host copy of d_sizes.  Root: d_all_packed (capacity >= sum of words) receives the packed
 * words of all ranks in rank order, d_all_offsets[sum of streams + 1] their global offsets; other ranks pass NULL for
 * both.  Grouped point-to-point transfers straight into their final positions, asynchronous on `stream` on every
 * rank.  A failing transfer never leaves an RCCL group open: the group is closed first, then the error is returned. */
cst_status cst_gather_rccl(void *comm, int32_t n_ranks, int32_t rank, int32_t root, const uint32_t *d_packed,
                           const uint64_t *d_offsets, const uint64_t *h_sizes, uint32_t *d_all_packed,
                           uint64_t *d_all_offsets, void *stream);

/* The inverse (decoding on the ranks what one rank holds): the root passes the packed words of all ranks'
 * streams in rank order and their global offsets[sum of streams + 1] (NULL on the other ranks); every rank receives its
 * own words in d_packed (capacity >= h_sizes[2 * rank + 1]) and d_offsets[n_streams_local + 1] rebased to start at 0 --
 * what the `d_offsets` form of cst_ans_decode_batch / cst_range_decode_batch takes.  h_sizes as above, on every rank. */
cst_status cst_scatter_rccl(void *comm, int32_t n_ranks, int32_t rank, int32_t root, const uint32_t *d_all_packed,
                            const uint64_t *d_all_offsets, const uint64_t *h_sizes, uint32_t *d_packed,
                            uint64_t *d_offsets, void *stream);

/* ------------------------------------------------------------------------------------------
 * float32 parameters.  Every call below that takes per-symbol parameter arrays as `const double *d_means, *d_stds`
 * (`d_a`, `d_b`) has a twin NAME_f32 whose arrays hold float32 -- what a hyperprior or context model emits.  The twins take
 * them as `const void *` (the Categorical calls' convention for matrices whose element type the call names) and differ
 * from their originals in nothing else: same arguments, same refusals, same scratch-size helpers; each is declared right
 * behind its original.  A C compiler cannot check the element type behind a `const void *`: pass arrays of `float`, never of
 * `double`, to a NAME_f32.  The kernels read the
 * floats themselves and widen them in registers (exactly: subnormals and signed zeros included), so every word, count,
 * status and jump-table entry is bit-identical to NAME on the arrays widened to double -- which is what the reference
 * computes for float32 callers (src/pybindings/mod.rs:187-214) -- without the widened copy.  cst_last_kernel_name()
 * reports the original's name with `f32` added to its tag list ("ans_encode_gaussian_fused_kernel<f32>",
 * "range_decode_gaussian_ragged_kernel<jump, f32>").  The chain coder's calls take doubles only.
 * ---------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------
 * per-symbol quantized Gaussians: the reference's flagship Python call
 *     coder.encode_reverse(symbols, QuantizedGaussian(min, max), means, stds)
 *     coder.decode(QuantizedGaussian(min, max), means, stds)
 * (src/pybindings/stream/stack.rs:567-588, 733-751; src/pybindings/stream/model/internals.rs:188-249)
 * d_means / d_stds have the same shape and layout as d_symbols (f64; f32 callers widen first,
 * src/pybindings/mod.rs:211-216).  std <= 0 or a non-finite parameter yields
 * CST_STREAM_IMPOSSIBLE_SYMBOL for that stream (the reference panics: pybindings/stream/model.rs:654-657).
 * ---------------------------------------------------------------------------------------- */
cst_status cst_ans_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                         const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                         size_t n_streams, size_t n_per_stream, cst_layout layout,
                                         uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                         uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_ans_encode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                             const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                             size_t n_streams, size_t n_per_stream, cst_layout layout,
                                             uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                             uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_ans_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                         const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                         const uint32_t *d_n_words, const double *d_means, const double *d_stds,
                                         int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                         cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                         int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_ans_decode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                             const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                             const uint32_t *d_n_words, const void *d_means, const void *d_stds,
                                             int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                             cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                             int32_t *d_status, uint32_t flags, void *stream);

/* QuantizedLaplace / QuantizedCauchy with per-symbol parameters (src/pybindings/stream/model.rs:736-900): the Gaussian calls
 * above over another CDF -- the same kernels, routes, slabs, offsets, words_capacity, CST_FLAG_RAW_STATE and layouts; no jump
 * points.  family: CST_FAMILY_LAPLACE (d_a = means, d_b = scales) or CST_FAMILY_CAUCHY (d_a = locs, d_b = scales); d_a / d_b are
 * f64 matrices of the symbols' shape and layout.  A scale <= 0 or a non-finite parameter, and a symbol outside
 * [min_symbol, max_symbol], yield CST_STREAM_IMPOSSIBLE_SYMBOL for that stream.  The words are those of the tabulated route
 * (cst_family_cdf_rows + cst_*_encode_cp_batch / cst_*_decode_rows_batch), without the n_symbols + 1 words of table per symbol.
 * Any other family, a NULL matrix / words / counts / status pointer and max_symbol <= min_symbol return
 * CST_ERR_INVALID_ARGUMENT before the device is touched. */
cst_status cst_ans_encode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                       const int32_t *d_symbols, const double *d_a, const double *d_b,
                                       size_t n_streams, size_t n_per_stream, cst_layout layout,
                                       uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                       uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_ans_encode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                           const int32_t *d_symbols, const void *d_a, const void *d_b,
                                           size_t n_streams, size_t n_per_stream, cst_layout layout,
                                           uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                           uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_ans_decode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                       const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                       const uint32_t *d_n_words, const double *d_a, const double *d_b,
                                       int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                       cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                       int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_ans_decode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                           const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                           const uint32_t *d_n_words, const void *d_a, const void *d_b,
                                           int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                           int32_t *d_status, uint32_t flags, void *stream);

/* Categorical models with per-symbol probability vectors (Categorical(perfect=False) / Categorical(lazy=True) with a rank-2 array of
 * probabilities, src/pybindings/stream/model/internals.rs:399-514): symbol (s, t) is coded with the "fast" quantisation
 * (src/stream/model/categorical.rs:16-54 = LazyContiguousCategoricalEntropyModel, lazy_contiguous.rs:131-331) of row (s, t) of
 * d_probs, a float (prob_bytes = 4) or double (prob_bytes = 8) matrix of the symbol matrix's shape and layout with the n_symbols
 * entries of a row innermost.  The arithmetic is done in the type of the matrix -- float stays float -- by one sequential sum per
 * row; symbols are 0 .. n_symbols - 1.  The same slabs, offsets, words_capacity, CST_FLAG_RAW_STATE and layouts as the Gaussian
 * calls; no jump points.
 * Before the device is touched: a NULL symbols / probabilities / words / counts / status pointer and prob_bytes outside {4, 8}
 * return CST_ERR_INVALID_ARGUMENT, n_symbols < 2 or n_symbols >= 2^precision - 1 returns CST_ERR_MODEL.
 * Per stream: a row whose sum is not a positive normal number or that holds a negative or NaN entry, a symbol outside
 * [0, n_symbols) and a symbol whose interval comes out empty (an f32 row can end in one) yield CST_STREAM_IMPOSSIBLE_SYMBOL.
 * CST_CATEGORICAL_ROUTE=fused|rows (debug switch) forces the decoders' route: one lane per stream walking its rows (default
 * from 64 streams on), or rows tabulated in pieces and looked up by one wave per stream. */
cst_status cst_ans_encode_categorical_batch(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                            int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                            uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                            uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_ans_decode_categorical_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                            size_t words_capacity, const uint32_t *d_n_words, const void *d_probs, int32_t prob_bytes,
                                            int32_t n_symbols, int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                            cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                            int32_t *d_status, uint32_t flags, void *stream);

/* The quantised rows themselves: d_rows[r][0 .. n_symbols] = left cumulatives of row r of d_probs [n_rows][n_symbols], then
 * 2^precision (1 <= precision <= 31).  A bad row (see above) is written as 0xffffffff followed by 2^precision, and d_bad[r]
 * (optional) is 1 for it, else 0.  cst_categorical_fast_cdf_host is the same row walk on the CPU over host buffers. */
cst_status cst_categorical_fast_cdf_rows(int32_t precision, const void *d_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                         uint32_t *d_rows, int32_t *d_bad, void *stream);
cst_status cst_categorical_fast_cdf_host(int32_t precision, const void *h_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                         uint32_t *h_rows, int32_t *h_bad);

/* Categorical(perfect=True) / Bernoulli(perfect=True) with per-symbol probability vectors, quantised ON THE DEVICE: one wave runs
 * `perfectly_quantized_probabilities` (src/stream/model/categorical.rs:56-177; f32 rows are widened to f64 first) for one row --
 * the words of cst_categorical_perfect_cdf, row by row.  2 <= n_symbols <= CST_CATEGORICAL_PERFECT_MAX_K.
 *
 * cst_categorical_perfect_cdf_rows: the rows in the format of cst_categorical_fast_cdf_rows (1 <= precision <= 31).  d_bad[r]
 * (optional): 0 a good row, 1 a bad one (the host function's CST_ERR_MODEL: a sum that is not a positive normal number, a negative
 * or NaN entry, a share beyond the weight that is left), 2 a row whose search had not ended after 16 * n_symbols + 1024 unit
 * moves (a safety stop; no input is known to come near it).  Rows with a nonzero code are written as 0xffffffff followed by
 * 2^precision.  d_moves[r] (optional): the unit moves of the row's search.  cst_categorical_perfect_cdf_host is the same
 * formulation (ranks instead of a sorted vector, the same stop) on the CPU over host buffers.
 *
 * cst_{ans,range}_{encode,decode}_categorical_perfect_batch: the argument lists, layouts, slabs, offsets, words_capacity and
 * CST_FLAG_RAW_STATE of cst_*_categorical_batch.  The encoders quantise a row and keep only the entry of its symbol; the decoders
 * tabulate rows in pieces of at most 64 MiB and look them up with one wave per stream.  A row with a nonzero code and a symbol
 * outside [0, n_symbols) yield CST_STREAM_IMPOSSIBLE_SYMBOL for their stream only.
 * Before the device is touched: NULL pointers and prob_bytes outside {4, 8} return CST_ERR_INVALID_ARGUMENT; n_symbols < 2,
 * n_symbols > CST_CATEGORICAL_PERFECT_MAX_K and n_symbols > 2^precision return CST_ERR_MODEL. */
#define CST_CATEGORICAL_PERFECT_MAX_K 1024
cst_status cst_categorical_perfect_cdf_rows(int32_t precision, const void *d_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                            uint32_t *d_rows, int32_t *d_bad, uint32_t *d_moves, void *stream);
cst_status cst_categorical_perfect_cdf_host(int32_t precision, const void *h_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                            uint32_t *h_rows, int32_t *h_bad, uint32_t *h_moves);

/* Fitting table models to the data ON THE DEVICE (static two-pass coding: count, quantise, code).
 *
 * cst_count_symbols: histograms of n_total int32 symbols.  d_indices == NULL (n_tables must be 1): one histogram of the whole
 * array.  Otherwise symbol i counts into row d_indices[i] of d_counts [n_tables][n_symbols]; index_bytes is 1 (uint8) or 4
 * (int32) as in the indexed coders.  A symbol outside [min_symbol, min_symbol + n_symbols) or with an index outside [0, n_tables)
 * goes into no bin and adds one to *d_outside.  1 <= n_tables <= 256, 2 <= n_symbols <= 65536, n_total < 2^31.
 *
 * cst_count_symbols_per_stream: one histogram per stream, d_counts [n_streams][n_symbols], 2 <= n_symbols <= 1024.  The input is
 * stream-major with n_per_stream symbols per stream, or ragged with d_sym_offsets [n_streams + 1] (stream s is the flat range
 * [d_sym_offsets[s], d_sym_offsets[s + 1]), as in the ragged coders; n_per_stream is ignored then).  Fewer than 2^31 symbols in all.
 *
 * Both zero d_counts and *d_outside themselves on `stream`; n_total == 0 returns CST_OK with zeroed counts.  NULL pointers, a bad
 * index_bytes and sizes outside the limits return CST_ERR_INVALID_ARGUMENT before the device is touched.
 *
 * cst_fit_cdf_rows: row r of d_rows [n_rows][n_symbols + 1] is what Categorical(counts[r] as f64, perfect) tabulates: the counts
 * are widened to f64 (exact) and handed to cst_categorical_fast_cdf_rows, or with perfect != 0 to cst_categorical_perfect_cdf_rows
 * (n_symbols <= CST_CATEGORICAL_PERFECT_MAX_K), whose limits and error codes apply.  A row WITHOUT any count (an empty stream, an
 * index class nobody names) is quantised as if every count were 1, and d_empty[r] (optional) is 1 for it, else 0 -- the reference
 * refuses such a row; here one empty stream does not void a batch.  cst_fit_cdf_rows_host: the same over host buffers, no device.
 * The rows feed cst_model_create_tables_per_stream, or, read back, cst_model_create_table / cst_table_set_create. */
cst_status cst_count_symbols(const int32_t *d_symbols, size_t n_total, int32_t min_symbol, int32_t n_symbols,
                             const void *d_indices, int32_t index_bytes, int32_t n_tables,
                             uint32_t *d_counts, uint32_t *d_outside, void *stream);
cst_status cst_count_symbols_per_stream(const int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams, size_t n_per_stream,
                                        int32_t min_symbol, int32_t n_symbols, uint32_t *d_counts, uint32_t *d_outside, void *stream);
cst_status cst_fit_cdf_rows(int32_t precision, int32_t perfect, const uint32_t *d_counts, size_t n_rows, int32_t n_symbols,
                            uint32_t *d_rows, int32_t *d_empty, void *stream);
cst_status cst_fit_cdf_rows_host(int32_t precision, int32_t perfect, const uint32_t *h_counts, size_t n_rows, int32_t n_symbols,
                                 uint32_t *h_rows, int32_t *h_empty);

cst_status cst_ans_encode_categorical_perfect_batch(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                                    uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                                    uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_ans_decode_categorical_perfect_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t *d_n_words, const void *d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                                    cst_layout layout, uint64_t *d_state, uint32_t *d_n_words_out,
                                                    int32_t *d_status, uint32_t flags, void *stream);

/* Per-symbol models given explicitly (any model family with per-symbol parameters, e.g.
 * Categorical(perfect=False) with a probability matrix, src/pybindings/stream/model/internals.rs:188-249):
 *   encode: d_left / d_prob hold EncoderModel::left_cumulative_and_probability of every symbol
 *           (same shape/layout as the symbol matrix; prob == 0 marks an impossible symbol);
 *   decode: d_cdf_rows holds one cdf[n_symbols+1] row per coded symbol, row index = element index of the
 *           symbol matrix (s*n_per_stream + t, or t*n_streams + s for CST_LAYOUT_SYMBOL_MAJOR). */
cst_status cst_ans_encode_cp_batch(cst_coder_config cfg, const uint32_t *d_left, const uint32_t *d_prob,
                                   size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                   size_t stride_words, uint32_t *d_n_words, uint64_t *d_state, int32_t *d_status,
                                   uint32_t flags, void *stream);

cst_status cst_ans_decode_rows_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets,
                                     size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, const uint32_t *d_cdf_rows,
                                     int32_t n_symbols, int32_t min_symbol, int32_t *d_symbols, size_t n_streams,
                                     size_t n_per_stream, cst_layout layout, uint64_t *d_state,
                                     uint32_t *d_n_words_out, int32_t *d_status, uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * batched range coder (BASELINE config C4): one RangeEncoder / RangeDecoder per stream
 *   encode: RangeEncoder::encode_iid_symbols + get_compressed   src/stream/queue.rs:612-705, 458-523
 *   decode: RangeDecoder::from_compressed + decode_iid_symbols  src/stream/queue.rs:847-868, 968-1033
 * Symbols are coded in forward order (a queue).  Same slab/offset conventions as the ANS calls.
 * ---------------------------------------------------------------------------------------- */
/* Raw coder state of one range coder, for continuing a coder across calls (the single-coder drop-in):
 * RangeCoderState{lower, range} + EncoderSituation (queue.rs:60-71, 126-142) on the encoder side,
 * RangeCoderState + point + words consumed on the decoder side. */
typedef struct cst_range_state {
    uint64_t lower;
    uint64_t range;
    uint64_t point;        /* decoder only */
    uint32_t inverted_n;   /* encoder only: 0 = EncoderSituation::Normal */
    uint32_t inverted_first;
    uint64_t position;     /* decoder only: words consumed so far */
} cst_range_state;

/* d_rstate (may be NULL unless CST_FLAG_RAW_STATE) is in/out with CST_FLAG_RAW_STATE: the encoder then starts
 * from it and appends no seal words, the decoder does not re-read `point` and continues at ->position.
 * The model has one shared table, or one table per stream (cst_model_create_gaussian_per_stream /
 * cst_model_create_tables_per_stream: table s codes stream s; n_tables must equal n_streams, presets (32,64) and (16,32),
 * precision <= 16, either layout; "range_encode_ps_kernel" / "range_decode_ps_kernel": the stream's 16-bit cdf row sits in
 * LDS, a support too large for that is CST_ERR_INVALID_ARGUMENT).  With such a model CST_FLAG_RAW_STATE is refused
 * (CST_ERR_INVALID_ARGUMENT).  cst_jump_points_auto answers 0 for it. */
cst_status cst_range_encode_batch(const cst_model *model, cst_coder_config cfg, const int32_t *d_symbols,
                                  size_t n_streams, size_t n_per_stream, cst_layout layout,
                                  uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                  cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_decode_batch(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                  const uint64_t *d_offsets, size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                  int32_t *d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                  cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

/* ABI 5: NARROW symbol matrices for the range coder -- the reference's RangeEncoder / RangeDecoder are generic over the symbol type
 * (src/stream/queue.rs:612, 968; src/stream/model/quantize.rs:229-255).  The four calls below are cst_range_{en,de}code_batch[_ckpt] with
 * the matrix given as symbol_bytes = 1 (int8), 2 (int16) or 4 (int32: the plain call); words, counts, status and jump points are
 * those of the int32 call on the widened values.  An int8 matrix of stream-major rows of whole 32-symbol tiles at (32,64),
 * 8 <= P <= 24, is read by the hand-scheduled encoder itself ("range_encode_n8_kernel" / "range_encode_ckpt_n8_kernel": a quarter of the
 * symbol bytes, one more instruction per symbol) and written by the sub-lane decoder itself ("range_decode_n8_kernel" /
 * "range_decode_sub_n8_kernel": its byte tiles hold the symbols); every other shape converts next to the int32 call
 * (cst_symbols_widen / cst_symbols_narrow), models with one table per stream among them.  The decoders want a support that fits the type.
 * d_scratch: cst_range_sym_scratch_bytes(n_streams, n_per_stream, ckpt_interval or 0, symbol_bytes) bytes, contents irrelevant. */
size_t cst_range_sym_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval, int32_t symbol_bytes);
cst_status cst_range_encode_batch_sym(const cst_model *model, cst_coder_config cfg, const void *d_symbols, int32_t symbol_bytes,
                                      size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                      size_t stride_words, uint32_t *d_n_words, cst_range_state *d_rstate, int32_t *d_status,
                                      uint32_t flags, void *d_scratch, void *stream);
cst_status cst_range_decode_batch_sym(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                      const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                      const uint32_t *d_n_words, void *d_symbols, int32_t symbol_bytes, size_t n_streams,
                                      size_t n_per_stream, cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                      uint32_t flags, void *d_scratch, void *stream);
cst_status cst_range_encode_batch_ckpt_sym(const cst_model *model, cst_coder_config cfg, const void *d_symbols, int32_t symbol_bytes,
                                           size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                           size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval, uint32_t *d_ckpt_pos,
                                           uint64_t *d_ckpt_lower, uint64_t *d_ckpt_range, int32_t *d_status, void *d_scratch,
                                           void *stream);
cst_status cst_range_decode_batch_ckpt_sym(const cst_model *model, cst_coder_config cfg, const uint32_t *d_words,
                                           const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                           const uint32_t *d_n_words, size_t ckpt_interval, const uint32_t *d_ckpt_pos,
                                           const uint64_t *d_ckpt_lower, const uint64_t *d_ckpt_range, void *d_symbols,
                                           int32_t symbol_bytes, size_t n_streams, size_t n_per_stream, void *d_scratch,
                                           int32_t *d_status, void *stream);


/* Per-symbol-model variants of the range coder (same argument meaning as the cst_ans_* twins). */
cst_status cst_range_encode_cp_batch(cst_coder_config cfg, const uint32_t *d_left, const uint32_t *d_prob,
                                     size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                     size_t stride_words, uint32_t *d_n_words, cst_range_state *d_rstate,
                                     int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                           const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                           size_t n_streams, size_t n_per_stream, cst_layout layout,
                                           uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                           cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_range_encode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                               const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                               size_t n_streams, size_t n_per_stream, cst_layout layout,
                                               uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                               cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                           const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                           const uint32_t *d_n_words, const double *d_means, const double *d_stds,
                                           int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                           uint32_t flags, void *stream);
cst_status cst_range_decode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                               const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                               const uint32_t *d_n_words, const void *d_means, const void *d_stds,
                                               int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                               cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                               uint32_t flags, void *stream);

/* ... and over QuantizedLaplace / QuantizedCauchy (see cst_ans_encode_family_batch) */
cst_status cst_range_encode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                         const int32_t *d_symbols, const double *d_a, const double *d_b,
                                         size_t n_streams, size_t n_per_stream, cst_layout layout,
                                         uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                         cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_range_encode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                             const int32_t *d_symbols, const void *d_a, const void *d_b,
                                             size_t n_streams, size_t n_per_stream, cst_layout layout,
                                             uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                             cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_decode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                         const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                         const uint32_t *d_n_words, const double *d_a, const double *d_b,
                                         int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                         cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                         uint32_t flags, void *stream);
cst_status cst_range_decode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                             const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                             const uint32_t *d_n_words, const void *d_a, const void *d_b,
                                             int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                             cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                             uint32_t flags, void *stream);

/* ... and over Categorical probability matrices (see cst_ans_encode_categorical_batch) */
cst_status cst_range_encode_categorical_batch(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                              int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                              uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                              cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_decode_categorical_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                              size_t words_capacity, const uint32_t *d_n_words, const void *d_probs, int32_t prob_bytes,
                                              int32_t n_symbols, int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                              cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                              uint32_t flags, void *stream);

/* ... and with the perfect quantisation (see cst_ans_encode_categorical_perfect_batch) */
cst_status cst_range_encode_categorical_perfect_batch(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                      int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                                      uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                                      cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);

cst_status cst_range_decode_categorical_perfect_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                                      size_t words_capacity, const uint32_t *d_n_words, const void *d_probs, int32_t prob_bytes,
                                                      int32_t n_symbols, int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                                      cst_layout layout, cst_range_state *d_rstate, int32_t *d_status,
                                                      uint32_t flags, void *stream);

/* Categorical probability matrices for streams of DIFFERENT lengths (the fast quantisation of cst_*_categorical_batch: Categorical(perfect=False) /
 * Categorical(lazy=True)), plain and with jump points, both coders, both presets.  Stream s owns rows [d_sym_offsets[s], d_sym_offsets[s + 1])
 * of the flat matrix d_probs [n_total][n_symbols] (float: prob_bytes = 4, double: 8) and of the flat d_symbols [n_total].  Every stream's
 * words, word count and status are those of cst_{ans,range}_{encode,decode}_categorical_batch for that stream alone, bit for bit.
 *   - d_order, d_word_offsets / stride_words / words_capacity, the slabs and empty streams (no words, CST_STREAM_OK): as in
 *     cst_{ans,range}_{encode,decode}_gaussian_ragged.
 *   - n_total: the rows of d_probs and the elements of d_symbols.  Pass 1 of the encoders is sized by it (no read-back of d_sym_offsets), and
 *     the device bounds every row index by it: a stream that reaches beyond n_total reports CST_STREAM_INVALID_DATA and nothing is coded for
 *     it; one whose symbol range runs backwards or exceeds 2^32 - 1 reports CST_STREAM_CAPACITY.  The other streams are unaffected.
 *   - A bad row (see cst_ans_encode_categorical_batch), a symbol outside [0, n_symbols) and an empty interval yield
 *     CST_STREAM_IMPOSSIBLE_SYMBOL for their stream only.
 *   - *_jump: the plain call's arguments (the decoders' WITHOUT d_order), then jump_interval, d_chunk_offsets and the table -- argument order,
 *     table layout and semantics exactly those of cst_{ans,range}_{encode,decode}_gaussian_ragged_jump; the decoders' d_scratch holds
 *     cst_persymbol_ragged_jump_scratch_bytes(n_chunks_total) bytes.  jump_interval: a positive multiple of 16, at most 2^31 - 1.
 *   - Before the device is touched: a NULL pointer (d_order and d_word_offsets may be NULL, the latter with stride_words > 0), prob_bytes
 *     outside {4, 8}, an unsupported cfg, n_streams > 2^31 - 1, n_total > 64 (2^31 - 1) (encoders) and every refusal of the Gaussian jump
 *     calls return CST_ERR_INVALID_ARGUMENT; then n_symbols < 2 or n_symbols >= 2^precision - 1 returns CST_ERR_MODEL.  n_streams == 0:
 *     CST_OK, nothing is launched.
 *   - One route for every batch size: built for many streams; a few are coded correctly, but slowly.  Not here: the perfect quantisation (the
 *     cst_*_categorical_perfect_ragged calls below),
 *     the symbol-major layout (a ragged batch has none), a count_until, intervals that are no multiple of 16.
 * cst_last_kernel_name(): {ans,range}_encode_categorical_ragged_two_pass, {ans,range}_decode_categorical_ragged_kernel, and the same names
 * followed by <jump>. */
cst_status cst_ans_encode_categorical_ragged(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                             int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                             const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                             size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_categorical_ragged(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                             size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, const void *d_probs,
                                             int32_t prob_bytes, int32_t n_symbols, size_t n_total, int32_t *d_symbols,
                                             const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order, int32_t *d_status,
                                             void *stream);
cst_status cst_range_encode_categorical_ragged(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                               int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                               const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                               size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_ragged(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                               size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, const void *d_probs,
                                               int32_t prob_bytes, int32_t n_symbols, size_t n_total, int32_t *d_symbols,
                                               const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order, int32_t *d_status,
                                               void *stream);
cst_status cst_ans_encode_categorical_ragged_jump(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                  int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                                  const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                                  size_t stride_words, uint32_t *d_n_words, size_t jump_interval,
                                                  const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos, uint64_t *d_jump_state,
                                                  int32_t *d_status, void *stream);
cst_status cst_ans_decode_categorical_ragged_jump(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                  size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                  const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                  int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                  size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                  const uint32_t *d_jump_pos, const uint64_t *d_jump_state, void *d_scratch,
                                                  int32_t *d_status, void *stream);
cst_status cst_range_encode_categorical_ragged_jump(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                                    const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                                    size_t stride_words, uint32_t *d_n_words, size_t jump_interval,
                                                    const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos, uint64_t *d_jump_lower,
                                                    uint64_t *d_jump_range, int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_ragged_jump(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                    size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                    const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                    int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                    size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                    const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                    const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status, void *stream);

/* ... and with the perfect quantisation: Categorical(perfect=True), the reference's default, for streams of DIFFERENT lengths, plain and with
 * jump points (ABI 5).  The argument lists are those of cst_*_categorical_ragged[_jump] with ONE exception: the two plain
 * decoders take max_len directly after n_total.  Stream s owns rows [d_sym_offsets[s], d_sym_offsets[s + 1]) of d_probs [n_total][n_symbols]
 * and of the flat d_symbols; its words, word count and status are those of cst_{ans,range}_{encode,decode}_categorical_perfect_batch for
 * that stream alone, bit for bit.  d_order, the slabs, empty streams, the refusals against n_total (CST_STREAM_CAPACITY /
 * CST_STREAM_INVALID_DATA), the jump table, its layout and d_scratch (cst_persymbol_ragged_jump_scratch_bytes) are exactly those of
 * cst_*_categorical_ragged[_jump].
 *   - max_len (plain decoders): an upper bound of the longest stream.  The decoders tabulate the rows of a piece of positions of a group of
 *     streams, then look the symbols up, piece after piece up to max_len, without reading d_sym_offsets back.  A stream longer than max_len
 *     reports CST_STREAM_CAPACITY and decodes nothing.  The jump decoders need none: a chunk has at most jump_interval symbols.
 *   - The rows of one step stay within 64 MiB (CST_PERFECT_RAGGED_BUDGET, a debug switch, gives the budget in 32-bit words).
 *   - A bad or non-converged row (codes 1 and 2 of cst_categorical_perfect_cdf_rows) and a symbol outside [0, n_symbols) yield
 *     CST_STREAM_IMPOSSIBLE_SYMBOL for their stream only.
 *   - Before the device is touched: the refusals of cst_*_categorical_ragged[_jump], with the model limits of the perfect quantisation --
 *     n_symbols < 2, n_symbols > CST_CATEGORICAL_PERFECT_MAX_K or n_symbols > 2^precision return CST_ERR_MODEL -- and, encoders,
 *     n_total > 2^31 - 1 returns CST_ERR_INVALID_ARGUMENT (one quantiser workgroup per row).  n_streams == 0: CST_OK, nothing is launched.
 * cst_last_kernel_name(): {ans,range}_encode_categorical_perfect_ragged_two_pass, {ans,range}_decode_categorical_perfect_ragged_by_rows, and the
 * same names followed by <jump>. */
cst_status cst_ans_encode_categorical_perfect_ragged(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                     int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                                     const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                                     size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_categorical_perfect_ragged(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                     size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                     const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                     size_t max_len, int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                     const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_range_encode_categorical_perfect_ragged(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs, int32_t prob_bytes,
                                                       int32_t n_symbols, size_t n_total, const uint64_t *d_sym_offsets, size_t n_streams,
                                                       const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                                       size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_perfect_ragged(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                       size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                       const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                       size_t max_len, int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                       const uint32_t *d_order, int32_t *d_status, void *stream);
cst_status cst_ans_encode_categorical_perfect_ragged_jump(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs,
                                                          int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                          const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                          uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                          uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                          uint32_t *d_jump_pos, uint64_t *d_jump_state, int32_t *d_status, void *stream);
cst_status cst_ans_decode_categorical_perfect_ragged_jump(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                          size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                          const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                          int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                          size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                          const uint32_t *d_jump_pos, const uint64_t *d_jump_state, void *d_scratch,
                                                          int32_t *d_status, void *stream);
cst_status cst_range_encode_categorical_perfect_ragged_jump(cst_coder_config cfg, const int32_t *d_symbols, const void *d_probs,
                                                            int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                            const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                                            uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                                            uint32_t *d_n_words, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                                            uint32_t *d_jump_pos, uint64_t *d_jump_lower, uint64_t *d_jump_range,
                                                            int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_perfect_ragged_jump(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                            size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                            const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                            int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                            size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                            const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                            const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status, void *stream);

/* Random access into a ragged per-symbol Categorical batch, both quantisers: cst_{ans,range}_decode_gaussian_ragged_select (above) with
 * "parameters" read as "rows".  The arguments follow those calls block by block: cfg (no min_symbol / max_symbol); the words block; the
 * model arguments of cst_*_decode_categorical_ragged -- d_probs, prob_bytes, n_symbols, n_total: the batch's FULL [n_total][K] matrix,
 * laid out as the plain decode call takes it; the perfect pair only: max_piece_len; d_sym_offsets, n_streams; the table block (all
 * zero / NULL: no table); the query block and the tail, unchanged.
 *   - Piece j of a query reads rows from row d_sym_offsets[s] + (first / jump_interval + j) * jump_interval on (d_sym_offsets[s] without
 *     a table), decodes and drops its first symbols with THEIR rows and stores the rest at its place in the ragged output.  ONLY rows
 *     [that first row, d_sym_offsets[s] + first + count) of a query can influence any result or status: everything else in d_probs may
 *     hold anything (NaN included).
 *   - max_piece_len (the perfect pair): an upper bound of (symbols dropped + symbols stored) over all pieces -- with a table at most
 *     jump_interval (larger values are clamped to it), without one max(first + count) -- the role max_len has in
 *     cst_*_decode_categorical_perfect_ragged: the host loop runs without a read-back.  A piece longer than max_piece_len makes its
 *     query report CST_STREAM_CAPACITY and write nothing.  The rows are tabulated for groups of pieces within the 64 MiB of the plain
 *     perfect decoders (CST_PERFECT_RAGGED_BUDGET).
 *   - Statuses, one per QUERY.  Refused before decoding, nothing written: CST_STREAM_INVALID_DATA for every query
 *     cst_{ans,range}_decode_ragged_select refuse, and for a query whose stream's rows reach beyond n_total.  Failing while decoding: a
 *     query that meets a bad row or an impossible quantile, in its dropped part too, reports CST_STREAM_IMPOSSIBLE_SYMBOL and may leave
 *     anything inside its own output slice, nothing outside it.  The other queries are unaffected either way.
 *   - d_scratch: cst_persymbol_ragged_select_scratch_bytes(n_pieces_total) bytes, for all four.
 *   - CST_ERR_INVALID_ARGUMENT, then CST_ERR_MODEL, before the device is touched: every refusal of the plain Categorical ragged decode
 *     call of the same quantiser (d_symbols_out in the place of d_symbols; prob_bytes outside {4, 8}; its limits of K); with a table,
 *     every refusal of the _jump decoders; table arrays without an interval; n_pieces_total > 2^32 - 1; exactly one of d_query_first /
 *     d_query_count NULL; with n_queries > 0 a NULL d_query_stream, d_piece_offsets, d_out_offsets or d_scratch.  n_queries == 0
 *     returns CST_OK and launches nothing.
 * cst_last_kernel_name(): {ans,range}_decode_categorical_ragged_kernel<select>,
 * {ans,range}_decode_categorical_perfect_ragged_by_rows<select>. */
cst_status cst_ans_decode_categorical_ragged_select(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                    size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                    const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                    const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                    const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                    const uint64_t *d_jump_state, const uint32_t *d_query_stream,
                                                    const uint64_t *d_query_first, const uint64_t *d_query_count, size_t n_queries,
                                                    const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                    const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_ragged_select(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                      size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                      const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                      const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                      const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                      const uint64_t *d_jump_lower, const uint64_t *d_jump_range,
                                                      const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                      const uint64_t *d_query_count, size_t n_queries, const uint64_t *d_piece_offsets,
                                                      size_t n_pieces_total, int32_t *d_symbols_out, const uint64_t *d_out_offsets,
                                                      void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_ans_decode_categorical_perfect_ragged_select(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                                            size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                                            const void *d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                            size_t max_piece_len, const uint64_t *d_sym_offsets, size_t n_streams,
                                                            size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                            const uint32_t *d_jump_pos, const uint64_t *d_jump_state,
                                                            const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                            const uint64_t *d_query_count, size_t n_queries,
                                                            const uint64_t *d_piece_offsets, size_t n_pieces_total,
                                                            int32_t *d_symbols_out, const uint64_t *d_out_offsets, void *d_scratch,
                                                            int32_t *d_status, void *stream);
cst_status cst_range_decode_categorical_perfect_ragged_select(cst_coder_config cfg, const uint32_t *d_words,
                                                              const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                                              const uint32_t *d_n_words, const void *d_probs, int32_t prob_bytes,
                                                              int32_t n_symbols, size_t n_total, size_t max_piece_len,
                                                              const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                              const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                              const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                              const uint64_t *d_jump_range, const uint32_t *d_query_stream,
                                                              const uint64_t *d_query_first, const uint64_t *d_query_count,
                                                              size_t n_queries, const uint64_t *d_piece_offsets, size_t n_pieces_total,
                                                              int32_t *d_symbols_out, const uint64_t *d_out_offsets, void *d_scratch,
                                                              int32_t *d_status, void *stream);

/* ABI 5: jump points for the per-symbol Gaussian calls of the RANGE coder (RangeEncoder::pos / RangeDecoder::seek, src/stream/queue.rs:172-196,
 * 900-926), as cst_ans_{encode,decode}_gaussian_batch_ckpt are for ANS: the fused encoder notes (words emitted including held-back ones,
 * lower, range) in front of every chunk of ckpt_interval symbols (a multiple of 16 that divides n_per_stream; stream-major), the decoder
 * runs every (stream, chunk) pair as a decoder of its own -- chunk j of stream s codes row s * n_chunks + j of the three matrices viewed
 * as [n_streams * n_chunks][interval] -- and writes n_streams * n_chunks status entries.  The words are those of
 * cst_range_encode_gaussian_batch.  d_scratch: cst_range_gaussian_ckpt_scratch_bytes(...). */
cst_status cst_range_encode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                                size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                                size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                                uint32_t *d_ckpt_pos, uint64_t *d_ckpt_lower, uint64_t *d_ckpt_range,
                                                int32_t *d_status, void *stream);
cst_status cst_range_encode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                    const int32_t *d_symbols, const void *d_means, const void *d_stds,
                                                    size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t *d_words,
                                                    size_t stride_words, uint32_t *d_n_words, size_t ckpt_interval,
                                                    uint32_t *d_ckpt_pos, uint64_t *d_ckpt_lower, uint64_t *d_ckpt_range,
                                                    int32_t *d_status, void *stream);
size_t cst_range_gaussian_ckpt_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval);
cst_status cst_range_decode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                                size_t words_capacity, const uint32_t *d_n_words, size_t ckpt_interval,
                                                const uint32_t *d_ckpt_pos, const uint64_t *d_ckpt_lower,
                                                const uint64_t *d_ckpt_range, const double *d_means, const double *d_stds,
                                                int32_t *d_symbols, size_t n_streams, size_t n_per_stream, void *d_scratch,
                                                int32_t *d_status, void *stream);
cst_status cst_range_decode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol,
                                                    const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t *d_n_words, size_t ckpt_interval,
                                                    const uint32_t *d_ckpt_pos, const uint64_t *d_ckpt_lower,
                                                    const uint64_t *d_ckpt_range, const void *d_means, const void *d_stds,
                                                    int32_t *d_symbols, size_t n_streams, size_t n_per_stream, void *d_scratch,
                                                    int32_t *d_status, void *stream);

cst_status cst_range_decode_rows_batch(cst_coder_config cfg, const uint32_t *d_words, const uint64_t *d_offsets,
                                       size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, const uint32_t *d_cdf_rows,
                                       int32_t n_symbols, int32_t min_symbol, int32_t *d_symbols, size_t n_streams,
                                       size_t n_per_stream, cst_layout layout, cst_range_state *d_rstate,
                                       int32_t *d_status, uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * ChainCoder (src/stream/chain.rs:231-246; DefaultChainCoder = <u32, u64, 24>, SmallChainCoder = <u16, u32, 12>)
 *
 * A chain coder holds two word stacks, `compressed` and `remainders`, and two heads (chain.rs:248-258):
 *   compressed_head   the bits of the last compressed word that are not consumed yet, below a leading 1 bit
 *   remainders_head   2^(S-W-P) <= head < 2^(S-P) between calls
 * Decoding (decode_symbol, chain.rs:1044-1122) POPS P bits per symbol from `compressed` -- whatever the model -- and
 * PUSHES what the symbol did not use onto `remainders`; encoding (encode_symbol, chain.rs:1140-1209; symbols last to
 * first) pops from `remainders` and pushes P bits per symbol onto `compressed`.  The constructors and terminators
 * (from_binary / from_compressed / from_remainders, into_remainders / into_compressed / into_binary: a handful of
 * words each) are host code in the binding (constriction_amd/stream/chain.py); these entry points are the symbol loops.
 *
 *   d_pop_words / d_pop_offsets / pop_stride / d_n_pop   the stack that is popped, laid out like d_words of the ANS
 *             decoder (stream s: d_pop_words[off(s) .. off(s) + d_n_pop[s]), consumed from the END); d_n_pop is updated;
 *             d_pop_words must be a valid device pointer (at least one word) even if every d_n_pop[s] is 0
 *   d_push_words / push_stride / d_n_push                the words pushed, in push order, stream s at s * push_stride;
 *             at most one word per symbol; d_n_push[s] = their number
 *   d_heads   in / out, one per stream
 * d_status: CST_STREAM_OUT_OF_DATA if the popped stack ran empty (the reference returns an error; the stream stops
 * there), IMPOSSIBLE_SYMBOL / CAPACITY as for the other coders.
 * ---------------------------------------------------------------------------------------- */
typedef struct cst_chain_heads {
    uint64_t remainders_head;
    uint32_t compressed_head;
    uint32_t reserved;
} cst_chain_heads;

cst_status cst_chain_encode_cp_batch(cst_coder_config cfg, const uint32_t *d_left, const uint32_t *d_prob, size_t n_streams,
                                     size_t n_per_stream, cst_layout layout, const uint32_t *d_pop_words,
                                     const uint64_t *d_pop_offsets, size_t pop_stride, uint32_t *d_n_pop, uint32_t *d_push_words,
                                     size_t push_stride, uint32_t *d_n_push, cst_chain_heads *d_heads, int32_t *d_status,
                                     void *stream);
cst_status cst_chain_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t *d_symbols,
                                           const double *d_means, const double *d_stds, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, const uint32_t *d_pop_words, const uint64_t *d_pop_offsets,
                                           size_t pop_stride, uint32_t *d_n_pop, uint32_t *d_push_words, size_t push_stride,
                                           uint32_t *d_n_push, cst_chain_heads *d_heads, int32_t *d_status, void *stream);
cst_status cst_chain_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t *d_pop_words,
                                           const uint64_t *d_pop_offsets, size_t pop_stride, uint32_t *d_n_pop, const double *d_means,
                                           const double *d_stds, int32_t *d_symbols, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, uint32_t *d_push_words, size_t push_stride, uint32_t *d_n_push,
                                           cst_chain_heads *d_heads, int32_t *d_status, void *stream);
/* explicit cdf rows [n_symbols + 1] per coded symbol; row_stride = n_symbols + 1, or 0 for ONE row shared by every
 * symbol (a concrete model: decode_iid_symbols) */
cst_status cst_chain_decode_rows_batch(cst_coder_config cfg, const uint32_t *d_pop_words, const uint64_t *d_pop_offsets,
                                       size_t pop_stride, uint32_t *d_n_pop, const uint32_t *d_cdf_rows, size_t row_stride,
                                       int32_t n_symbols, int32_t min_symbol, int32_t *d_symbols, size_t n_streams,
                                       size_t n_per_stream, cst_layout layout, uint32_t *d_push_words, size_t push_stride,
                                       uint32_t *d_n_push, cst_chain_heads *d_heads, int32_t *d_status, void *stream);

/* The per-symbol entry points above take their scratch (16 B per symbol for encoding; 1 KiB per symbol of cdf rows, at
 * most 64 MiB at a time, for decoding fewer than 64 streams) from a stream-ordered memory pool that the LIBRARY owns (one
 * per device, created at first use; the device's default pool is never touched) and that keeps freed memory
 * (re-allocating 4 GiB per call cost more than coding them).  This hands it back: synchronises the device and trims the
 * library's pool. */
cst_status cst_release_scratch(void);

/* ------------------------------------------------------------------------------------------
 * Huffman symbol codes: constriction.symbol (src/symbol/mod.rs, src/symbol/huffman.rs, src/pybindings/symbol/)
 *
 * The reference's StackCoder / QueueEncoder / QueueDecoder with huffman.EncoderHuffmanTree / DecoderHuffmanTree codebooks,
 * one independent bit container per stream and ONE codebook shared by the batch.  Bits go into u32 words from bit 0
 * upwards (mod.rs:376-393, 600-617).  A stack (CST_HUFFMAN_STACK) writes each codeword leaf to root (huffman.rs:128-155),
 * consumes a stream's symbols BACK TO FRONT, ends with one seal bit `1` and is read from the last written bit downwards
 * (mod.rs:642-655); row s then decodes to symbols[s, 0..n) in order, the convention of cst_ans_encode_batch.  A queue
 * (CST_HUFFMAN_QUEUE) writes root to leaf (mod.rs:722-737), front to back, without a seal, and is read from bit 0 upwards
 * (mod.rs:438-455).
 * ---------------------------------------------------------------------------------------- */
#define CST_HUFFMAN_STACK 0
#define CST_HUFFMAN_QUEUE 1
/* largest alphabet a codebook takes (cst_huffman_codebook_create: CST_ERR_INVALID_ARGUMENT beyond) */
#define CST_HUFFMAN_MAX_SYMBOLS 65536

/* HOST function: the reference's tree (huffman.rs:62-116, 200-230) for n probabilities: pop the two smallest
 * (probability, index) pairs -- ties on the smaller index; the first popped becomes bit 0 -- and push their sum as inner
 * node n, n+1, ... .  Writes h_nodes[2n - 1], the encoder representation: node i holds parent << 1 | bit, 0 marks the root.
 * f32_sums != 0: probabilities are f32 values and every sum is an f32 addition (the reference adds in the input's float
 * type, which changes trees).  CST_ERR_MODEL for n == 0 and for NaN, negative or infinite probabilities. */
cst_status cst_huffman_tree(const double *h_probs, size_t n, int32_t f32_sums, uint64_t *h_nodes);

/* Device codebook from h_nodes[2n - 1] (cst_huffman_tree), 1 <= n <= CST_HUFFMAN_MAX_SYMBOLS: codewords in both bit orders
 * (codewords of more than 32 bits -- up to ~3000 for f64 probabilities -- in a bit pool the encoder reads out of line), the
 * decode table of the first 12 bits and the inner nodes the decoder walks past it.  *out is an opaque handle (void *), for
 * the coder calls below and cst_huffman_codebook_destroy.  CST_ERR_MODEL if h_nodes is not such a tree; synchronises
 * `stream`. */
cst_status cst_huffman_codebook_create(const uint64_t *h_nodes, size_t n, void *stream, void **out);
cst_status cst_huffman_codebook_destroy(void *codebook);

/* Slab stride (in words) that holds any stream of n_per_stream symbols: every codeword at the codebook's longest, the up to
 * 31 bits a continued call (d_cont) starts with and the seal, rounded up to whole 64-byte units.  0 for a bad argument. */
size_t cst_huffman_max_words(const void *codebook, size_t n_per_stream, int32_t semantics);

/* Replaces, for every stream s:
 *     coder = StackCoder(); for x in reversed(symbols[s]): coder.encode_symbol(x, tree)     (semantics CST_HUFFMAN_STACK)
 *     coder = QueueEncoder(); for x in symbols[s]: coder.encode_symbol(x, tree)             (CST_HUFFMAN_QUEUE)
 *     d_words[s*stride_words ..], d_n_bits[s] = coder.get_compressed_and_bitrate()           (pybindings/symbol/mod.rs:207-221)
 * d_symbols    stream-major [n_streams][n_per_stream], int32 (symbol_bytes 4) or uint8 (1)
 * d_n_bits     out (may be NULL): the bitrate, the written bits without the seal (mod.rs:205-220)
 * d_cont       in/out (may be NULL): the container's partial word, partial | nbits << 32 with nbits < 32.  Given, the call
 *              continues from it and neither seals nor flushes the partial word: d_words gets the completed words only and
 *              d_cont the new partial word (what the single-coder drop-in keeps between calls).
 * d_status     a symbol < 0 or >= n: CST_STREAM_IMPOSSIBLE_SYMBOL (huffman.rs:134-137); a slab too small: CST_STREAM_CAPACITY.
 *              Either way n_words (and n_bits) are 0 and d_cont is left as it was.
 * cst_last_kernel_name: "huffman_encode_kernel", or "huffman_encode_long_kernel" for a codebook with codewords of more than
 * 32 bits. */
cst_status cst_huffman_encode_batch(const void *codebook, int32_t semantics, const void *d_symbols, int32_t symbol_bytes,
                                    size_t n_streams, size_t n_per_stream, uint32_t *d_words, size_t stride_words,
                                    uint32_t *d_n_words, uint64_t *d_n_bits, uint64_t *d_cont, int32_t *d_status, void *stream);

/* Replaces, for every stream s, StackCoder(words[s]) resp. QueueDecoder(words[s]) and n_per_stream decode_symbol calls.  The
 * words of stream s are d_words[off(s) .. off(s) + d_n_words[s]) with off(s) = d_offsets ? d_offsets[s] : s * stride_words,
 * and words_capacity bounds them as for cst_ans_decode_batch.  symbol_bytes 1 needs n <= 256.
 * A stack stream is found by its seal, the HIGHEST set bit of its last word (the reference's from_compressed
 * looks at the lowest); no words or a zero last word: CST_STREAM_INVALID_DATA.  Running out of bits inside a codeword:
 * CST_STREAM_OUT_OF_DATA ("Ran out of bits in compressed data.", pybindings/symbol/mod.rs:386-395); the symbols from there on
 * read 0 and, as in the reference, every bit counts as read.
 * d_cont       in/out (may be NULL).  Queue: the read position in bits.  Stack: the partial word on top of the d_n_words[s]
 *              full words, partial | nbits << 32 (nbits < 32), instead of the seal search.  Out: the same after decoding.
 * d_n_words_out out (may be NULL).  Stack: the full words left below the partial word; queue: the words begun.
 * cst_last_kernel_name: "huffman_decode_kernel", or "huffman_decode_long_kernel" for codewords of more than 12 bits. */
cst_status cst_huffman_decode_batch(const void *codebook, int32_t semantics, const uint32_t *d_words, const uint64_t *d_offsets,
                                    size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, void *d_symbols,
                                    int32_t symbol_bytes, size_t n_streams, size_t n_per_stream, uint64_t *d_cont,
                                    uint32_t *d_n_words_out, int32_t *d_status, void *stream);

/* d_n_bits[s] (uint64 [n_streams]) = the exact bits of stream s under the codebook, without a stack's seal: what the encoders report
 * as d_n_bits, and what sizes exact slabs for them (a stack needs one bit more).  d_sym_offsets (uint64 [n_streams + 1]) as in the
 * ragged calls below, or NULL for a matrix [n_streams][n_per_stream].  A symbol outside 0 .. n-1 counts 0 bits (the encoder is what
 * reports it) and so does a range that runs backwards; the sums are 64-bit (a codeword can have ~3000 bits).
 * cst_last_kernel_name: "huffman_count_bits_kernel". */
cst_status cst_huffman_count_bits(const void *codebook, const void *d_symbols, int32_t symbol_bytes, const uint64_t *d_sym_offsets,
                                  size_t n_streams, size_t n_per_stream, uint64_t *d_n_bits, void *stream);

/* Streams of different lengths, the layout of cst_exp_golomb_encode_ragged / cst_exp_golomb_decode_ragged with a codebook:
 *     symbols of stream s = d_symbols[d_sym_offsets[s] .. d_sym_offsets[s + 1])      (flat, int32 or uint8: symbol_bytes 4 or 1)
 *     slab of stream s    = d_words[d_word_offsets[s] .. d_word_offsets[s + 1])      or, with d_word_offsets = NULL,
 *                           d_words[s * stride_words .. + stride_words)
 * One lane codes one stream, and the words of stream s are exactly what cst_huffman_encode_batch writes for it as a one-row batch
 * (the reference's StackCoder, symbols back to front and sealed, or QueueEncoder).  Statuses are those of the rectangular calls:
 * CST_STREAM_IMPOSSIBLE_SYMBOL and CST_STREAM_CAPACITY with 0 words and 0 bits, CST_STREAM_OUT_OF_DATA with the symbols from there
 * on 0, CST_STREAM_INVALID_DATA for a stack without its seal and for offsets or counts beyond words_capacity.  A stream of length 0
 * yields 0 words (a stack: its seal, 1 word) and CST_STREAM_OK.  A symbol range that runs backwards or exceeds 2^32 - 1 symbols:
 * CST_STREAM_CAPACITY from the encoder; a backwards one is CST_STREAM_INVALID_DATA (nothing written) from the decoder.  Word offsets
 * that run backwards are a slab of no words.  The decoder reads d_word_offsets[s] and d_n_words[s] only.  symbol_bytes 1 needs
 * n <= 256 to decode.  cst_last_kernel_name: "huffman_encode_ragged_kernel" / "huffman_decode_ragged_kernel", and
 * "huffman_encode_ragged_long_kernel" / "huffman_decode_ragged_long_kernel" for codewords of more than 32 / 12 bits. */
cst_status cst_huffman_encode_ragged(const void *codebook, int32_t semantics, const void *d_symbols, int32_t symbol_bytes,
                                     const uint64_t *d_sym_offsets, size_t n_streams, uint32_t *d_words, const uint64_t *d_word_offsets,
                                     size_t stride_words, uint32_t *d_n_words, uint64_t *d_n_bits, int32_t *d_status, void *stream);
cst_status cst_huffman_decode_ragged(const void *codebook, int32_t semantics, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                     size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, void *d_symbols,
                                     int32_t symbol_bytes, const uint64_t *d_sym_offsets, size_t n_streams, int32_t *d_status,
                                     void *stream);

/* Jump points for the ragged Huffman calls.  The reference has none for symbol codes ("Pos and Seek for SymbolCoder and for
 * QueueDecoder" is a to-do at the top of src/symbol/mod.rs): the table is this library's own, the words are those of
 * cst_huffman_encode_ragged bit for bit, and a reader that ignores the table loses only speed.
 *   - A jump point of a prefix code is one bit index and no coder state.  jump_interval (I) is a positive multiple of 32, at most
 *     2^31 - 32; d_chunk_offsets[n_streams + 1] is the exclusive prefix sum of ceil(length / I), the layout of
 *     cst_ans_{encode,decode}_ragged_jump; entry d_chunk_offsets[s] + j of d_jump_bits (uint64) is the bit index in stream s's
 *     container at which a reader starts chunk j, i.e. symbols [j I, min((j + 1) I, length)):
 *         queue   the first bit of the chunk's first codeword = the bits of symbols[: j I]; read upwards;
 *         stack   one past the highest bit of the chunk's first codeword = the bits of symbols[j I :]; read downwards; entry 0 is
 *                 d_n_bits[s], where the seal sits.
 *     Either is the container's bit length when the encoder crosses that boundary.  The entries of a stream whose status is not
 *     CST_STREAM_OK are unspecified; the encoder writes no entry outside [d_chunk_offsets[s], d_chunk_offsets[s + 1]).
 *   - The decoder runs one lane per chunk (n_chunks_total: the entries of d_jump_bits, at least d_chunk_offsets[n_streams]) and
 *     writes one status per STREAM: the largest of its chunks' status values, i.e. CST_STREAM_OUT_OF_DATA before
 *     CST_STREAM_INVALID_DATA before CST_STREAM_OK -- the precedence of cst_ans_decode_ragged_jump, which also takes the maximum.
 *   - A table entry beyond its stream's bits -- above 32 * d_n_words[s] for a queue, above the position of the seal for a stack --
 *     is CST_STREAM_INVALID_DATA for that stream and touches no other; it is judged before any word at that position is read.  A
 *     chunk that fails leaves zeros from the failure to its own end; the other chunks of its stream keep their symbols.  A table
 *     that does not describe its stream (chunks != ceil(length / I), offsets that run backwards or beyond n_chunks_total) is
 *     CST_STREAM_INVALID_DATA and nothing is written for that stream.
 * cst_last_kernel_name: "huffman_encode_ragged_kernel" / "huffman_decode_ragged_jump_kernel" and their "_long_kernel" forms
 * ("huffman_encode_ragged_long_kernel", "huffman_decode_ragged_jump_long_kernel").
 * All five calls return CST_ERR_INVALID_ARGUMENT (NULL pointers, symbol_bytes outside {1, 4}, unknown semantics, a handle that is no
 * codebook, an interval that is not allowed) before any device call. */
cst_status cst_huffman_encode_ragged_jump(const void *codebook, int32_t semantics, const void *d_symbols, int32_t symbol_bytes,
                                          const uint64_t *d_sym_offsets, size_t n_streams, uint32_t *d_words,
                                          const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words, uint64_t *d_n_bits,
                                          size_t jump_interval, const uint64_t *d_chunk_offsets, uint64_t *d_jump_bits,
                                          int32_t *d_status, void *stream);
cst_status cst_huffman_decode_ragged_jump(const void *codebook, int32_t semantics, const uint32_t *d_words,
                                          const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                          const uint32_t *d_n_words, void *d_symbols, int32_t symbol_bytes,
                                          const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                          const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint64_t *d_jump_bits,
                                          int32_t *d_status, void *stream);

/* Random access into a ragged Huffman batch: selected documents, or ranges of documents.  The contract is that of
 * cst_ans_decode_ragged_select -- queries (stream, first, count) in any order, repeats, overlaps and count 0 allowed, both of
 * d_query_first / d_query_count NULL for whole documents; a ragged output (query q owns d_symbols_out[d_out_offsets[q] ..
 * d_out_offsets[q + 1]), symbols of symbol_bytes 1 or 4) and one status per QUERY; d_piece_offsets[n_queries + 1] the exclusive
 * prefix sum of the pieces per query (with a table one per chunk touched, ceil((first % I + count) / I); without one 1; none for
 * count 0), n_pieces_total an upper bound of them; d_scratch of cst_ragged_select_scratch_bytes(n_pieces_total) bytes -- with the
 * table of cst_huffman_encode_ragged_jump (d_chunk_offsets, d_jump_bits), or without one (jump_interval 0, both pointers NULL).
 *   - With a table the first piece of a query seeks to entry first / I and decodes and drops first % I symbols.  Without one a query
 *     is one piece that starts where its document starts (a queue at bit 0, a stack at its seal) and drops `first` symbols.
 *   - A refused query reports CST_STREAM_INVALID_DATA and WRITES NOTHING: no such stream, a range beyond its document (no 64-bit
 *     wrap), a slice of d_out_offsets or d_piece_offsets that is not its own, words that leave words_capacity, a slice of the table
 *     that does not describe the stream, a stack without a seal, or ANY TABLE ENTRY IT TOUCHES BEYOND ITS STREAM'S BITS (above
 *     32 * d_n_words[s] for a queue, above the seal for a stack; judged before any word at the entry is read).  A document longer than
 *     2^32 - 1 symbols is CST_STREAM_CAPACITY.  Otherwise a query's status is the largest of its pieces' (CST_STREAM_OUT_OF_DATA
 *     before CST_STREAM_INVALID_DATA); a piece that fails writes zeros from the failure to its own end, all of them if it fails inside
 *     the symbols it drops.
 *   - CST_ERR_INVALID_ARGUMENT before the device is touched: what cst_huffman_decode_ragged refuses, an interval that is neither 0 nor
 *     a multiple of 32, a table given in part, n_chunks_total or n_pieces_total above 2^32 - 1, exactly one of d_query_first /
 *     d_query_count NULL, and with n_queries > 0 a NULL among the query, output, scratch or status pointers.  n_queries == 0 returns
 *     CST_OK and launches nothing.
 * Every piece is a lane of the SELECT form of the jump decoder.  cst_last_kernel_name: "huffman_decode_ragged_jump_kernel<select>" /
 * "huffman_decode_ragged_jump_long_kernel<select>". */
cst_status cst_huffman_decode_ragged_select(const void *codebook, int32_t semantics, const uint32_t *d_words,
                                            const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                            const uint32_t *d_n_words, const uint64_t *d_sym_offsets, size_t n_streams,
                                            size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                            const uint64_t *d_jump_bits, const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                            const uint64_t *d_query_count, size_t n_queries, const uint64_t *d_piece_offsets,
                                            size_t n_pieces_total, void *d_symbols_out, int32_t symbol_bytes,
                                            const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Exponential-Golomb symbol codes: ExpGolomb<N> of src/symbol/exp_golomb.rs in the bit containers above
 *
 * A universal code for unsigned integers, with no codebook to build or ship.  symbol_bytes selects N: 1 = u8 (uint8), 2 = u16 (the
 * bit pattern of int16), 4 = u32 (the bit pattern of int32: -1 is u32::MAX).  With m = symbol + 1 and len = floor(log2 m) the
 * codeword is, in prefix order, len zeros and then the len + 1 bits of m from the most significant down: 2 len + 1 bits.  N::MAX
 * wraps to m == 0 in the reference and codes as B zeros, a one, B zeros (B the bits of N: 17 / 33 / 65 bits).  A queue
 * (CST_SYMBOL_QUEUE) writes prefix order, a stream's symbols front to back, without a seal, its last partial word zero-padded; a
 * stack (CST_SYMBOL_STACK) writes every codeword in suffix order (prefix order reversed), a stream's symbols BACK TO FRONT, and one
 * seal bit, so that row s decodes to symbols[s, 0..n) in order: the conventions of the Huffman calls.
 * Every value of N has a codeword: an encoder reports CST_STREAM_OK or CST_STREAM_CAPACITY (n_words and n_bits 0, d_cont untouched).
 * A decoder reports CST_STREAM_INVALID_DATA for an invalid codeword (exp_golomb.rs:135-171): the bits run out inside the zero run,
 * the run is longer than B, the bits run out inside the len value bits, or len == B with value bits that are not all zero.  Running
 * out of bits is an invalid codeword here and not CST_STREAM_OUT_OF_DATA: a queue read past its last symbol walks into the zero
 * padding and ends this way.  A stack without words or with a zero last word is CST_STREAM_INVALID_DATA too.  The symbols from the
 * failing one on read 0, and the stream's d_cont / d_n_words_out are left as they came in (the reference leaves the bits consumed up
 * to the failure: DESIGN.md 7).
 * CST_ERR_INVALID_ARGUMENT (NULL pointers, symbol_bytes outside {1, 2, 4}, unknown semantics) is returned before any device call.
 * ---------------------------------------------------------------------------------------- */
#define CST_SYMBOL_STACK CST_HUFFMAN_STACK
#define CST_SYMBOL_QUEUE CST_HUFFMAN_QUEUE

/* HOST function, needs no device.  Slab stride (in words) that holds any stream of n_per_stream symbols: every codeword 2 B + 1 bits,
 * the up to 31 bits a continued call (d_cont) starts with and the seal, rounded up to whole 64-byte units.  0 for a bad argument. */
size_t cst_exp_golomb_max_words(size_t n_per_stream, int32_t symbol_bytes, int32_t semantics);

/* d_n_bits[s] (uint64 [n_streams]) = the exact bits of stream s, without a seal: what the encoders below report as d_n_bits, and
 * what sizes exact slabs for them (a stack needs one bit more).  d_sym_offsets (uint64 [n_streams + 1]) as in the ragged calls, or
 * NULL for a matrix [n_streams][n_per_stream]; a range that runs backwards counts 0.  cst_last_kernel_name:
 * "exp_golomb_count_bits_kernel". */
cst_status cst_exp_golomb_count_bits(const void *d_symbols, int32_t symbol_bytes, const uint64_t *d_sym_offsets, size_t n_streams,
                                     size_t n_per_stream, uint64_t *d_n_bits, void *stream);

/* cst_huffman_encode_batch / cst_huffman_decode_batch without a codebook: the same slabs or packed words (d_offsets), words_capacity,
 * d_n_bits, d_cont (partial | nbits << 32; for the queue decoder the read position in bits) and d_n_words_out.
 * cst_last_kernel_name: "exp_golomb_encode_kernel" / "exp_golomb_decode_kernel". */
cst_status cst_exp_golomb_encode_batch(int32_t semantics, const void *d_symbols, int32_t symbol_bytes, size_t n_streams,
                                       size_t n_per_stream, uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                       uint64_t *d_n_bits, uint64_t *d_cont, int32_t *d_status, void *stream);
cst_status cst_exp_golomb_decode_batch(int32_t semantics, const uint32_t *d_words, const uint64_t *d_offsets, size_t stride_words,
                                       size_t words_capacity, const uint32_t *d_n_words, void *d_symbols, int32_t symbol_bytes,
                                       size_t n_streams, size_t n_per_stream, uint64_t *d_cont, uint32_t *d_n_words_out,
                                       int32_t *d_status, void *stream);

/* Streams of different lengths, the layout of cst_ans_encode_ragged / cst_ans_decode_ragged without a model:
 *     symbols of stream s = d_symbols[d_sym_offsets[s] .. d_sym_offsets[s + 1])      (flat, of symbol_bytes each)
 *     slab of stream s    = d_words[d_word_offsets[s] .. d_word_offsets[s + 1])      or, with d_word_offsets = NULL,
 *                           d_words[s * stride_words .. + stride_words)
 * One lane codes one stream; a wave of 64 consecutive streams runs as long as its longest one.  d_n_bits (may be NULL) as above.  A
 * stream of length 0 yields 0 words (a stack: its seal, 1 word) and CST_STREAM_OK.  A symbol range that runs backwards or exceeds
 * 2^32 - 1 symbols: CST_STREAM_CAPACITY from the encoder, CST_STREAM_INVALID_DATA (nothing written) from the decoder; word offsets
 * that run backwards are a slab of no words.  The decoder reads d_word_offsets[s] and d_n_words[s] only and checks them against
 * words_capacity as cst_ans_decode_batch does.  cst_last_kernel_name: "exp_golomb_encode_ragged_kernel" /
 * "exp_golomb_decode_ragged_kernel". */
cst_status cst_exp_golomb_encode_ragged(int32_t semantics, const void *d_symbols, int32_t symbol_bytes, const uint64_t *d_sym_offsets,
                                        size_t n_streams, uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                        uint32_t *d_n_words, uint64_t *d_n_bits, int32_t *d_status, void *stream);
cst_status cst_exp_golomb_decode_ragged(int32_t semantics, const uint32_t *d_words, const uint64_t *d_word_offsets, size_t stride_words,
                                        size_t words_capacity, const uint32_t *d_n_words, void *d_symbols, int32_t symbol_bytes,
                                        const uint64_t *d_sym_offsets, size_t n_streams, int32_t *d_status, void *stream);

/* Jump points for the ragged Exp-Golomb calls: the table of cst_huffman_encode_ragged_jump with Exp-Golomb codeword lengths.
 * jump_interval (I) is a positive multiple of 32, at most 2^31 - 32; d_chunk_offsets[n_streams + 1] is the exclusive prefix sum of
 * ceil(length / I); entry d_chunk_offsets[s] + j of d_jump_bits (uint64) is the bit index at which a reader starts chunk j -- a queue
 * the bits of symbols[: j I], read upwards; a stack the bits of symbols[j I :], read downwards, entry 0 being d_n_bits[s], where the
 * seal sits.  The words are those of cst_exp_golomb_encode_ragged bit for bit.  The encoder adds one 8-byte store per chunk, always
 * between two whole codewords (a u32 symbol from 2^17 - 1 on is put in two pieces; no entry lies between them), and writes no entry
 * outside [d_chunk_offsets[s], d_chunk_offsets[s + 1]); the entries of a stream whose status is not CST_STREAM_OK are unspecified.
 * The decoder runs one lane per chunk (n_chunks_total: the entries of d_jump_bits) and writes one status per STREAM, the largest of its
 * chunks'.  There is no CST_STREAM_OUT_OF_DATA: a chunk that runs out of bits or meets an invalid codeword is
 * CST_STREAM_INVALID_DATA and leaves zeros from the failure to its own end, while the other chunks keep their symbols.  A table entry
 * beyond its stream's bits (above 32 * d_n_words[s] for a queue, above the seal for a stack; judged before any word at the entry is
 * read) and a stack without words or with a zero last word are CST_STREAM_INVALID_DATA for that stream only.  A table that does not
 * describe its stream (chunks != ceil(length / I), offsets that run backwards or beyond n_chunks_total) is CST_STREAM_INVALID_DATA
 * and nothing is written for that stream.  CST_ERR_INVALID_ARGUMENT (NULL pointers, symbol_bytes outside {1, 2, 4}, unknown
 * semantics, an interval that is 0, no multiple of 32 or too large) is returned before any device call.
 * cst_last_kernel_name: "exp_golomb_encode_ragged_jump_kernel" / "exp_golomb_decode_ragged_jump_kernel". */
cst_status cst_exp_golomb_encode_ragged_jump(int32_t semantics, const void *d_symbols, int32_t symbol_bytes,
                                             const uint64_t *d_sym_offsets, size_t n_streams, uint32_t *d_words,
                                             const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                             uint64_t *d_n_bits, size_t jump_interval, const uint64_t *d_chunk_offsets,
                                             uint64_t *d_jump_bits, int32_t *d_status, void *stream);
cst_status cst_exp_golomb_decode_ragged_jump(int32_t semantics, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                             size_t stride_words, size_t words_capacity, const uint32_t *d_n_words, void *d_symbols,
                                             int32_t symbol_bytes, const uint64_t *d_sym_offsets, size_t n_streams,
                                             size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                             const uint64_t *d_jump_bits, int32_t *d_status, void *stream);

/* cst_huffman_decode_ragged_select without a codebook: the same queries, pieces, refusals and argument errors (symbol_bytes in
 * {1, 2, 4}), with the table of cst_exp_golomb_encode_ragged_jump or without one.  A piece that fails is CST_STREAM_INVALID_DATA.
 * cst_last_kernel_name: "exp_golomb_decode_ragged_jump_kernel<select>". */
cst_status cst_exp_golomb_decode_ragged_select(int32_t semantics, const uint32_t *d_words, const uint64_t *d_word_offsets,
                                               size_t stride_words, size_t words_capacity, const uint32_t *d_n_words,
                                               const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                               const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint64_t *d_jump_bits,
                                               const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                               const uint64_t *d_query_count, size_t n_queries, const uint64_t *d_piece_offsets,
                                               size_t n_pieces_total, void *d_symbols_out, int32_t symbol_bytes,
                                               const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------------------------------
 * indexed table coding: every symbol names one of K tabulated models
 *
 * The common way to drive an entropy coder from a learned codec: a hyperprior or context model predicts one scale (or class)
 * per latent, the prediction is quantised to one of K levels, and the coder uses that level's pre-tabulated model:
 *     coder.encode_symbols_reverse(symbols.zip(indices.map(|k| &tables[k])))      src/stream/stack.rs:784-849
 *     encoder.encode_symbols(symbols.zip(indices.map(|k| &tables[k])))            src/stream/queue.rs:612-705
 * with every tables[k] a ContiguousCategoricalEntropyModel (src/stream/model/categorical/contiguous.rs:673-700).  Only K distinct
 * models ever exist, so they live in LDS and a symbol costs its index (1 or 4 bytes) of side traffic.
 *
 * A cst_table_set is K cdfs that share a support [min_symbol, min_symbol + n_symbols) and a precision: an opaque handle of its
 * own, passed as void * like the Huffman codebook (*out of cst_table_set_create; valid for the calls below and
 * cst_table_set_destroy; the getters answer 0 for anything else).  It is NOT a cst_model: a cst_model with several tables means
 * "one table per stream" to every other entry point.
 * Limits: 1 <= n_tables <= 256 and 1 <= precision <= 24 (else CST_ERR_INVALID_ARGUMENT); n_symbols >= 2, and the set's LDS image
 * must fit beside the coder's rings and tiles: n_tables * (n_symbols + 1) * E bytes of rows, rounded up to 16, E = 2 for
 * precision <= 16 and 4 above, plus at least n_tables * 2 * B bytes of bucket index, rounded up to 16, B = 1 for n_symbols <= 256
 * and 2 above, in 90 KiB (92 160 bytes) -- else CST_ERR_MODEL.  64 tables of 255 symbols fit at every precision, 256 tables of
 * 64 symbols at precision <= 16.  Every row h_cdfs[k][0 .. n_symbols] is validated as cst_model_create_table validates its one
 * row (0 = cdf[0] < cdf[1] < ... < cdf[n_symbols] = 2^precision); a bad row: CST_ERR_MODEL.  Argument errors are reported
 * before the device is touched; without a device: CST_ERR_NO_DEVICE.  The device image is built once, here. */
cst_status cst_table_set_create(int32_t precision, int32_t min_symbol, int32_t n_symbols, int32_t n_tables, const uint32_t *h_cdfs,
                                void **out);
cst_status cst_table_set_destroy(void *tables);
int32_t cst_table_set_precision(const void *tables);
int32_t cst_table_set_min_symbol(const void *tables);
int32_t cst_table_set_n_symbols(const void *tables);
int32_t cst_table_set_n_tables(const void *tables);

/* cst_ans_encode_batch / cst_ans_decode_batch / cst_range_encode_batch / cst_range_decode_batch with the table set in the model's
 * place and two more arguments: d_indices, of the symbol matrix's shape and layout, and index_bytes = 1 (uint8) or 4 (int32).
 * Symbol t of stream s is coded with table d_indices[s][t]; every stream's words, count and final state are those of the reference
 * coder fed that sequence of models (the ANS coder walks a row last symbol first, as encode_symbols_reverse does), in the slab /
 * offset / words_capacity conventions of the plain calls.
 * Scope: cfg = (32, 64, precision of the set), int32 symbols, CST_LAYOUT_STREAM_MAJOR, flags = CST_FLAG_NONE, any number of streams
 * and symbols per stream.  Anything else, a NULL pointer (d_state, d_rstate and d_n_words_out excepted) or a handle that is not a
 * live table set: CST_ERR_INVALID_ARGUMENT before any device call.
 * Optional outputs (NULL = discard): the encoders leave the coder state in front of its seal in d_state[s] (the ANS state whose
 * words end the stream) resp. d_rstate[s] (lower, range, inverted_n, inverted_first); the decoders leave what remains of the coder
 * in d_state[s] and d_n_words_out[s] (words not consumed) resp. d_rstate[s] (lower, range, point, position = words consumed).
 * Per-stream status: a symbol outside the support, or an encoder index >= n_tables (no table gives that symbol a probability):
 * CST_STREAM_IMPOSSIBLE_SYMBOL; a slab too small: CST_STREAM_CAPACITY -- d_n_words[s] is then 0, the slab's content and the optional
 * state are unspecified, as after cst_ans_encode_batch.  A decoder index >= n_tables: CST_STREAM_INVALID_DATA, and that stream's
 * symbols from there on, its state and counts are unspecified (the index is clamped before any table is read).  A failing stream
 * never disturbs its neighbours and writes nothing outside its own row and slab.  Decoding past the end of the words and corrupt
 * counts or offsets behave as in cst_ans_decode_batch / cst_range_decode_batch.
 * cst_last_kernel_name: "ans_encode_indexed_kernel", "ans_decode_indexed_kernel", "range_encode_indexed_kernel",
 * "range_decode_indexed_kernel". */
cst_status cst_ans_encode_indexed_batch(const void *tables, cst_coder_config cfg, const int32_t *d_symbols,
                                        const void *d_indices, int32_t index_bytes, size_t n_streams, size_t n_per_stream,
                                        cst_layout layout, uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                        uint64_t *d_state, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_ans_decode_indexed_batch(const void *tables, cst_coder_config cfg, const uint32_t *d_words,
                                        const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                        const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes, int32_t *d_symbols,
                                        size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t *d_state,
                                        uint32_t *d_n_words_out, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_range_encode_indexed_batch(const void *tables, cst_coder_config cfg, const int32_t *d_symbols,
                                          const void *d_indices, int32_t index_bytes, size_t n_streams, size_t n_per_stream,
                                          cst_layout layout, uint32_t *d_words, size_t stride_words, uint32_t *d_n_words,
                                          cst_range_state *d_rstate, int32_t *d_status, uint32_t flags, void *stream);
cst_status cst_range_decode_indexed_batch(const void *tables, cst_coder_config cfg, const uint32_t *d_words,
                                          const uint64_t *d_offsets, size_t stride_words, size_t words_capacity,
                                          const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes, int32_t *d_symbols,
                                          size_t n_streams, size_t n_per_stream, cst_layout layout, cst_range_state *d_rstate,
                                          int32_t *d_status, uint32_t flags, void *stream);

/* Indexed table coding for streams of DIFFERENT lengths, plain and with jump points: the per-symbol ragged calls
 * (cst_{ans,range}_{encode,decode}_gaussian_ragged[_jump] above) with the table set and the index array in the model's place.
 * Stream s owns elements [d_sym_offsets[s], d_sym_offsets[s + 1]) of the flat d_symbols (int32) and d_indices (index_bytes = 1: uint8,
 * 4: int32; the same element numbering); symbol t of a stream is coded with table d_indices[that element].  The ANS coder codes a
 * stream last symbol first, the range coder first symbol first.  Every stream's words, count and status are those of
 * cst_{ans,range}_encode_indexed_batch for that stream alone, and those of the reference coder fed that sequence of models.
 *   - Slabs: d_word_offsets[n_streams + 1] (slab of stream s = [off[s], off[s + 1])), or NULL with stride_words > 0 (s * stride_words).
 *     A stream of n symbols fills at most min(n, ceil(n P / 32)) + 2 words under either coder (the two words of the ANS state, resp.
 *     the two words that seal a range coder).  d_order: NULL, or [n_streams] lane slot -> stream (cst_ans_encode_ragged's schedule; an
 *     entry that is not a stream codes nothing); results are indexed by stream whatever the order.
 *   - Jump points: layout and semantics of the table are those of cst_{ans,range}_encode_gaussian_ragged_jump -- jump_interval a
 *     positive multiple of 16; chunk j of stream s is entry d_chunk_offsets[s] + j; ANS notes (words in the bulk, state) AFTER the
 *     chunk's first symbol has been coded, the range coder (words emitted including held-back ones, lower, range) BEFORE it; no chunk
 *     starts at the end of a stream.  The words are bit-identical to the plain call's.  The jump decoders take no d_order and
 *     d_scratch of cst_persymbol_ragged_jump_scratch_bytes(n_chunks_total) bytes; they run every table entry as a coder of its own.
 *   - Per-stream status.  Encode: a symbol outside the support or an index >= n_tables: CST_STREAM_IMPOSSIBLE_SYMBOL with d_n_words[s]
 *     = 0, for that stream alone; a slab too small, or offsets that run backwards: CST_STREAM_CAPACITY; a stream of length 0: 0 words,
 *     CST_STREAM_OK.  Decode: an index >= n_tables is clamped before any table is read and its stream reports
 *     CST_STREAM_INVALID_DATA (the worst of its chunks' statuses in the jump form); a slice that leaves words_capacity:
 *     CST_STREAM_INVALID_DATA; a jump table that does not describe its stream, or a d_jump_pos beyond d_n_words:
 *     CST_STREAM_INVALID_DATA for that stream -- the others decode, and nothing outside words_capacity or the stream's own symbols is
 *     touched.  No index byte outside [d_indices, d_indices + index_bytes * d_sym_offsets[n_streams]) is read: a uint8 row may start at
 *     any byte, an int32 row at any 4-byte boundary.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: a NULL `tables` or a handle that is not a live table set; a NULL
 *     d_symbols / d_indices / d_sym_offsets / d_words / d_n_words / d_status; index_bytes not 1 or 4; a preset other than (32, 64);
 *     cfg.precision not the set's; d_word_offsets == NULL with stride_words == 0; n_streams > 2^32 - 1; in the jump forms also
 *     jump_interval 0, not a multiple of 16 or > 2^31 - 1, a NULL d_chunk_offsets or table array, n_chunks_total > 2^32 - 1, a NULL
 *     d_scratch.  n_streams == 0 (with arguments that pass): CST_OK, nothing is launched.
 * cst_last_kernel_name(): {ans,range}_{encode,decode}_indexed_ragged_kernel, with <jump> appended for the jump forms. */
cst_status cst_ans_encode_indexed_ragged(cst_coder_config cfg, const void *tables, const int32_t *d_symbols, const void *d_indices,
                                         int32_t index_bytes, const uint64_t *d_sym_offsets, size_t n_streams,
                                         const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                         size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_range_encode_indexed_ragged(cst_coder_config cfg, const void *tables, const int32_t *d_symbols, const void *d_indices,
                                           int32_t index_bytes, const uint64_t *d_sym_offsets, size_t n_streams,
                                           const uint32_t *d_order, uint32_t *d_words, const uint64_t *d_word_offsets,
                                           size_t stride_words, uint32_t *d_n_words, int32_t *d_status, void *stream);
cst_status cst_ans_decode_indexed_ragged(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                         const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                         const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes, int32_t *d_symbols,
                                         const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                         int32_t *d_status, void *stream);
cst_status cst_range_decode_indexed_ragged(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                           const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                           const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes, int32_t *d_symbols,
                                           const uint64_t *d_sym_offsets, size_t n_streams, const uint32_t *d_order,
                                           int32_t *d_status, void *stream);
cst_status cst_ans_encode_indexed_ragged_jump(cst_coder_config cfg, const void *tables, const int32_t *d_symbols,
                                              const void *d_indices, int32_t index_bytes, const uint64_t *d_sym_offsets,
                                              size_t n_streams, const uint32_t *d_order, uint32_t *d_words,
                                              const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                              size_t jump_interval, const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos,
                                              uint64_t *d_jump_state, int32_t *d_status, void *stream);
cst_status cst_range_encode_indexed_ragged_jump(cst_coder_config cfg, const void *tables, const int32_t *d_symbols,
                                                const void *d_indices, int32_t index_bytes, const uint64_t *d_sym_offsets,
                                                size_t n_streams, const uint32_t *d_order, uint32_t *d_words,
                                                const uint64_t *d_word_offsets, size_t stride_words, uint32_t *d_n_words,
                                                size_t jump_interval, const uint64_t *d_chunk_offsets, uint32_t *d_jump_pos,
                                                uint64_t *d_jump_lower, uint64_t *d_jump_range, int32_t *d_status, void *stream);
cst_status cst_ans_decode_indexed_ragged_jump(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                              const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                              const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes,
                                              int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                              size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                              const uint32_t *d_jump_pos, const uint64_t *d_jump_state, void *d_scratch,
                                              int32_t *d_status, void *stream);
cst_status cst_range_decode_indexed_ragged_jump(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                                const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                                const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes,
                                                int32_t *d_symbols, const uint64_t *d_sym_offsets, size_t n_streams,
                                                size_t jump_interval, const uint64_t *d_chunk_offsets, size_t n_chunks_total,
                                                const uint32_t *d_jump_pos, const uint64_t *d_jump_lower,
                                                const uint64_t *d_jump_range, void *d_scratch, int32_t *d_status, void *stream);

/* Random access into a ragged indexed batch: cst_{ans,range}_decode_ragged_select (where queries, pieces,
 * d_out_offsets, d_piece_offsets and the per-query statuses are described) for the indexed ragged decoders above.  The arguments are
 * the model block of cst_{ans,range}_decode_indexed_ragged_jump (cfg, tables, the words block, d_indices / index_bytes -- the batch's
 * FULL index array, laid out exactly as the plain decode call takes it -- d_sym_offsets, n_streams), then the table block and the query
 * block of cst_{ans,range}_decode_gaussian_ragged_select with the same conventions: jump_interval 0 and every table pointer NULL is no
 * table; both of d_query_first / d_query_count NULL is whole streams; d_status has one entry per QUERY; n_queries == 0 returns CST_OK
 * and launches nothing.
 *   - A piece reads its indices from the element of its jump point on: element d_sym_offsets[s] + (first / jump_interval + j) *
 *     jump_interval for piece j of a query, d_sym_offsets[s] without a table.  The symbols in front of `first` are decoded with their
 *     own tables and dropped.  No index byte outside [that first element, d_sym_offsets[s] + first + count) of a piece is read (a uint8
 *     piece may start at any byte, an int32 piece at any 4-byte boundary), so ONLY those indices can influence any result or status:
 *     everything else in d_indices may hold anything, the indices behind a query's end in the same chunk included.
 *   - Statuses, one per QUERY: CST_STREAM_INVALID_DATA (nothing is written) for every query cst_{ans,range}_decode_ragged_select
 *     refuse.  An index >= n_tables inside a query's decoded range, the dropped symbols included, is clamped before any table is read
 *     and the query reports CST_STREAM_INVALID_DATA; it may leave anything inside its own output slice, nothing outside it; the other
 *     queries are unaffected.
 *   - d_scratch: cst_persymbol_ragged_select_scratch_bytes(n_pieces_total) bytes.
 *   - CST_ERR_INVALID_ARGUMENT, before the device is touched: every refusal of the plain indexed ragged decode (d_symbols_out in the
 *     place of d_symbols; d_order does not exist here); with a table, every refusal of the _jump decoders (jump_interval not a
 *     multiple of 16 or > 2^31 - 1, a NULL d_chunk_offsets or table array, n_chunks_total > 2^32 - 1); table arrays without an interval;
 *     n_pieces_total > 2^32 - 1; exactly one of d_query_first / d_query_count NULL; with n_queries > 0 a NULL d_query_stream,
 *     d_piece_offsets, d_out_offsets or d_scratch.
 * Four launches: the queries kernel, the per-symbol piece builder, the decoder (a lane per piece), the status kernel.
 * cst_last_kernel_name(): {ans,range}_decode_indexed_ragged_kernel<select>. */
cst_status cst_ans_decode_indexed_ragged_select(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                                const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                                const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes,
                                                const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                const uint64_t *d_jump_state, const uint32_t *d_query_stream,
                                                const uint64_t *d_query_first, const uint64_t *d_query_count, size_t n_queries,
                                                const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);
cst_status cst_range_decode_indexed_ragged_select(cst_coder_config cfg, const void *tables, const uint32_t *d_words,
                                                  const uint64_t *d_word_offsets, size_t stride_words, size_t words_capacity,
                                                  const uint32_t *d_n_words, const void *d_indices, int32_t index_bytes,
                                                  const uint64_t *d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                  const uint64_t *d_chunk_offsets, size_t n_chunks_total, const uint32_t *d_jump_pos,
                                                  const uint64_t *d_jump_lower, const uint64_t *d_jump_range,
                                                  const uint32_t *d_query_stream, const uint64_t *d_query_first,
                                                  const uint64_t *d_query_count, size_t n_queries,
                                                  const uint64_t *d_piece_offsets, size_t n_pieces_total, int32_t *d_symbols_out,
                                                  const uint64_t *d_out_offsets, void *d_scratch, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------------------------------
 * bit-exact f64 special functions on device (test hooks for the model kernels)
 * out[i] = erf(x[i]) resp. Gaussian cdf, evaluated by the same device code the table kernels use.
 * ---------------------------------------------------------------------------------------- */
cst_status cst_debug_erf(const double *d_x, double *d_out, size_t n, void *stream);
/* the same erf as the per-symbol kernels evaluate it (one Horner recurrence over per-lane coefficients from LDS) */
cst_status cst_debug_erf_tab(const double *d_x, double *d_out, size_t n, void *stream);
/* The per-symbol kernels evaluate the Gaussian left cumulative through a FAST erf and fall back to the bit-exact one
 * wherever free_weight * cdf lies so close to an integer that the difference could change the truncation (cst_math.hpp);
 * the integer is the reference's in every case.  Hooks: which = 0: out[i] = fast erf(x[i]); 1: |fast - exact|. */
cst_status cst_debug_erf_fast(int32_t which, const double *d_x, double *d_out, size_t n, void *stream);
/* left cumulative of symbol index d_index[i] (0 .. n_symbols) under Gaussian(d_means[i], d_stds[i]) both ways:
 * d_counts[0] += results that differ (must stay 0), d_counts[1] += exact fallbacks taken (caller zeroes d_counts). */
cst_status cst_debug_gaussian_left_quick(int32_t precision, int32_t min_symbol, int32_t max_symbol, const int32_t *d_index,
                                         const double *d_means, const double *d_stds, size_t n, uint64_t *d_counts,
                                         void *stream);
cst_status cst_debug_gaussian_lcp(int32_t precision, int32_t prob_bits, int32_t min_symbol, int32_t max_symbol,
                                  const int32_t *d_symbols, const double *d_means, const double *d_stds,
                                  uint32_t *d_left, uint32_t *d_prob, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONSTRICTION_AMD_H */
