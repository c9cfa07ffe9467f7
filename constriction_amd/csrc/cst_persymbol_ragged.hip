// cst_persymbol_ragged.hip -- per-symbol Gaussian, Laplace and Cauchy models for streams of DIFFERENT lengths (cst_persymbol.hpp has the
// map of the per-symbol files): the plain forms of encode_gaussian_ragged_kernel and decode_gaussian_ragged_kernel
// (cst_persymbol_ragged.hpp) and their eight entry points.  Their forms with jump points: cst_persymbol_ragged_jump.hip.
#include "cst_persymbol_ragged.hpp"

namespace cst {

// ---- host side: one route whatever the batch ----
template <int KIND, class FAM, class PT>
static cst_status launch_encode_ragged(cst_coder_config cfg, const GaussianRaggedEncodeArgs& a, hipStream_t hs) {
    const size_t per_block = (size_t)(kFuBlock / kWave) * kFuStreams;
    const size_t blocks = (a.n_streams + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    const size_t lds = (FAM::kErfTab ? kFuTabBytes : 0) + (size_t)(kFuBlock / kWave) * kRgEncWaveBytes;
    return dispatch_word_size(cfg, [&](auto W, auto S) { return launch_with_lds(encode_gaussian_ragged_kernel<W, S, KIND, FAM, false, PT>, blocks, kFuBlock, lds, a, hs); });
}

template <int KIND, class FAM, class PT>
static cst_status launch_decode_ragged(cst_coder_config cfg, const GaussianRaggedDecodeArgs& a, hipStream_t hs) {
    const size_t blocks = (a.p.n_streams + kRgDecThreads - 1) / kRgDecThreads;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    const size_t lds = FAM::kErfTab ? kRgDecLdsBytes : kRgDecLdsBytesNoTab;
    return dispatch_word_size(cfg, [&](auto W, auto S) { return launch_with_lds(decode_gaussian_ragged_kernel<W, S, KIND, FAM, kRgPlain, PT>, blocks, kRgDecThreads, lds, a, hs); });
}

// the checks, the arguments and the launch of every (coder, family) ragged encode call; d_a / d_b are the family's two parameters
template <int KIND, class FAM, class PT>
static cst_status encode_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols, const PT* d_a,
                                const PT* d_b, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, uint32_t* d_words,
                                const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, int32_t* d_status, hipStream_t hs) {
    if (cst_status st = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                   stride_words, d_n_words, d_status, d_order, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    GaussianRaggedEncodeArgs a{};
    a.symbols = d_symbols; a.means = d_a; a.stds = d_b; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.order = d_order;
    a.precision = cfg.precision; a.lo = min_symbol; a.hi = max_symbol;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words = d_n_words; a.status = d_status;
    return note_kernel(FamilyNames<FAM, PT>::ragged[KIND == kRange][0], launch_encode_ragged<KIND, FAM, PT>(cfg, a, hs));
}

template <int KIND, class FAM, class PT>
static cst_status decode_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                const PT* d_a, const PT* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                const uint32_t* d_order, int32_t* d_status, hipStream_t hs) {
    if (cst_status st = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                   stride_words, d_n_words, d_status, d_order, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    GaussianRaggedDecodeArgs a{};
    a.p.words = d_words; a.p.offsets = d_word_offsets; a.p.stride_words = stride_words; a.p.n_words = d_n_words; a.p.words_capacity = words_capacity;
    a.p.symbols = d_symbols; a.p.n_streams = n_streams; a.p.precision = cfg.precision;
    a.p.min_symbol = min_symbol; a.p.n_symbols = (int32_t)((int64_t)max_symbol - min_symbol + 1);
    a.p.means = d_a; a.p.stds = d_b; a.p.status = d_status;
    a.sym_offsets = d_sym_offsets; a.order = d_order;
    return note_kernel(FamilyNames<FAM, PT>::ragged[KIND == kRange][1], launch_decode_ragged<KIND, FAM, PT>(cfg, a, hs));
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_ans_encode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                          const double* d_means, const double* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                          const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                          uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_ragged<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, d_sym_offsets, n_streams, d_order, d_words,
                                               d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                          const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                          const double* d_means, const double* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                          size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_ragged<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_means,
                                               d_stds, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                            const double* d_means, const double* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                            const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                            uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_ragged<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, d_sym_offsets, n_streams, d_order, d_words,
                                                 d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                            const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                            const double* d_means, const double* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                            size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_ragged<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_means,
                                                 d_stds, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_ans_encode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                        const double* d_a, const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                        const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                        uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged, kAns, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                        const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                        const double* d_a, const double* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                        size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_a,
                             d_b, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                          const double* d_a, const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                          const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                          uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged, kRange, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                          const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                          const double* d_a, const double* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                          size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_a,
                             d_b, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

// ---- the float32 twins (the header's "float32 parameters"): the originals' arguments with the arrays untyped, the same host templates ----

cst_status cst_ans_encode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                              const void* d_means, const void* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                              const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                              uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_ragged<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), d_sym_offsets, n_streams, d_order, d_words,
                                               d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_ans_encode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                            const void* d_a, const void* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                            const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                            uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged, kAns, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                              const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                              const void* d_means, const void* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                              size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_ragged<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_means),
                                               f32(d_stds), d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                            const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                            const void* d_a, const void* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                            size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_a),
                             f32(d_b), d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                const void* d_means, const void* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_ragged<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), d_sym_offsets, n_streams, d_order, d_words,
                                                 d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                              const void* d_a, const void* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                              const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                              uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged, kRange, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                const void* d_means, const void* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_ragged<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_means),
                                                 f32(d_stds), d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                              const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                              const void* d_a, const void* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                              size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_a),
                             f32(d_b), d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

} // extern "C"
