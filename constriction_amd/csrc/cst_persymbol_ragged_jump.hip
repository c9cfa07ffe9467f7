// cst_persymbol_ragged_jump.hip -- jump points (the reference's Pos / Seek) for the per-symbol coders of cst_persymbol_ragged.hip: the
// JUMP forms of encode_gaussian_ragged_kernel and decode_gaussian_ragged_kernel, launched between the kernels that turn a jump table
// into chunks and chunk statuses into stream statuses (all in cst_persymbol_ragged.hpp), and the eight entry points.  A unit of its
// own: twenty-four more instantiations of the two kernels would have doubled the build's longest compile.
#include "cst_persymbol_ragged.hpp"

namespace cst {

template <int KIND, class FAM>
static cst_status encode_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols, const double* d_a,
                                     const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, uint32_t* d_words,
                                     const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, size_t jump_interval,
                                     const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_a, uint64_t* d_jump_b,
                                     int32_t* d_status, hipStream_t hs) {
    if (jump_interval_bad(jump_interval) || !d_chunk_offsets || !d_jump_pos || !d_jump_a || (KIND == kRange && !d_jump_b)) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                   stride_words, d_n_words, d_status, d_order, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    GaussianRaggedEncodeJumpArgs a{};
    a.symbols = d_symbols; a.means = d_a; a.stds = d_b; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.order = d_order;
    a.precision = cfg.precision; a.lo = min_symbol; a.hi = max_symbol;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words = d_n_words; a.status = d_status;
    a.jump_tiles = (uint32_t)(jump_interval / kFuTile); a.jump_chunk_offsets = d_chunk_offsets; a.jump_pos = d_jump_pos; a.jump_a = d_jump_a;
    a.jump_b = d_jump_b;
    const size_t per_block = (size_t)(kFuBlock / kWave) * kFuStreams;
    const size_t blocks = (n_streams + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    const size_t lds = (FAM::kErfTab ? kFuTabBytes : 0) + (size_t)(kFuBlock / kWave) * kRgEncWaveBytes;
    return note_kernel(FamilyNames<FAM>::ragged_jump[KIND == kRange][0], dispatch_word_size(cfg, [&](auto W, auto S) {
        return launch_with_lds(encode_gaussian_ragged_kernel<W, S, KIND, FAM, true>, blocks, kFuBlock, lds, a, hs);
    }));
}

// d_jump_a / d_jump_b: the state (ANS, d_jump_b unused), or lower / range (the range coder)
template <int KIND, class FAM>
static cst_status decode_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                     const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                     const double* d_a, const double* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                     size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                     const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    if (jump_interval_bad(jump_interval) || n_chunks_total > 0xffffffffull || !d_chunk_offsets || !d_jump_pos || !d_jump_a ||
        (KIND == kRange && !d_jump_b) || !d_scratch) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                   stride_words, d_n_words, d_status, nullptr, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    if (n_streams > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    const uint32_t interval = (uint32_t)jump_interval;
    // (slab form without a capacity: all the slabs, as the ragged table coders' jump decoders take it)
    const uint64_t capacity = words_capacity ? words_capacity : (d_word_offsets ? 0 : (uint64_t)n_streams * stride_words);
    const PerSymbolJumpScratch v(d_scratch, n_chunks_total);
    if (n_chunks_total > 0) {
        const unsigned grid = (unsigned)((n_chunks_total + 255) / 256);
        dispatch_word_size(cfg, [&](auto W, auto S) {
            hipLaunchKernelGGL((persymbol_jump_chunks_kernel<W, S, KIND>), dim3(grid), dim3(256), 0, hs, d_words, d_sym_offsets, d_word_offsets, stride_words,
                               capacity, d_n_words, d_chunk_offsets, n_streams, n_chunks_total, interval, d_jump_pos, d_jump_a, d_jump_b, v);
            return 0;
        });
        CST_HIP_TRY(hipGetLastError());
        // (the slices handed on are absolute offsets that passed the check, or empty: `capacity` bounds them once more)
        GaussianRaggedChunkArgs a{};
        a.p.words = d_words; a.p.offsets = v.word_off; a.p.stride_words = 0; a.p.n_words = v.n_words; a.p.words_capacity = capacity;
        a.p.symbols = d_symbols; a.p.n_streams = n_chunks_total; a.p.precision = cfg.precision;
        a.p.min_symbol = min_symbol; a.p.n_symbols = (int32_t)((int64_t)max_symbol - min_symbol + 1);
        a.p.means = d_a; a.p.stds = d_b; a.p.status = v.status; a.p.state = v.state; a.p.rstate = v.rstate;
        a.sym_lo = v.sym_lo; a.len = v.len;
        const size_t blocks = (n_chunks_total + kRgDecThreads - 1) / kRgDecThreads;
        const size_t lds = FAM::kErfTab ? kRgDecLdsBytes : kRgDecLdsBytesNoTab;
        const cst_status rc = dispatch_word_size(cfg, [&](auto W, auto S) {
            return launch_with_lds(decode_gaussian_ragged_kernel<W, S, KIND, FAM, true>, blocks, kRgDecThreads, lds, a, hs);
        });
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(persymbol_jump_status_kernel<>, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, hs, v, d_sym_offsets, d_word_offsets,
                       stride_words, capacity, d_chunk_offsets, d_jump_pos, d_n_words, n_streams, n_chunks_total, interval, d_status);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(FamilyNames<FAM>::ragged_jump[KIND == kRange][1], CST_OK);
}

} // namespace cst

using namespace cst;

extern "C" {

// ---- jump points: the plain calls' arguments, then the interval and the table ----

size_t cst_persymbol_ragged_jump_scratch_bytes(size_t n_chunks_total) { return 80 * n_chunks_total + 128; }

cst_status cst_ans_encode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                               const double* d_means, const double* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                               const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                               uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                               uint64_t* d_jump_state, int32_t* d_status, void* stream) {
    return encode_ragged_jump<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, d_sym_offsets, n_streams, d_order, d_words,
                                                    d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state,
                                                    nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                               const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                               const double* d_means, const double* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                               size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                               const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status,
                                               void* stream) {
    return decode_ragged_jump<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_means,
                                                    d_stds, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                    d_jump_pos, d_jump_state, nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                 const double* d_means, const double* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                 const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                 uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                 uint64_t* d_jump_lower, uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return encode_ragged_jump<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, d_sym_offsets, n_streams, d_order, d_words,
                                                      d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower,
                                                      d_jump_range, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                 const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                 const double* d_means, const double* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                 size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                 void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_jump<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                      d_means, d_stds, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                      d_jump_pos, d_jump_lower, d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_ans_encode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                             const double* d_a, const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                             const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                             uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                             uint64_t* d_jump_state, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged_jump, kAns, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state, nullptr, d_status,
                             (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                             const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                             const double* d_a, const double* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                             size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                             const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status,
                                             void* stream) {
    return CST_FAMILY_CALL(decode_ragged_jump, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_a,
                             d_b, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_state,
                             nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                               const double* d_a, const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                               const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                               uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                               uint64_t* d_jump_lower, uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged_jump, kRange, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower, d_jump_range, d_status,
                             (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged_jump(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                               const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                               const double* d_a, const double* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                               size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                               const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                               void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_jump, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_a,
                             d_b, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_lower,
                             d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

} // extern "C"
