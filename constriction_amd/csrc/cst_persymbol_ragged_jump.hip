// cst_persymbol_ragged_jump.hip -- jump points (the reference's Pos / Seek) for the per-symbol coders of cst_persymbol_ragged.hip: the
// JUMP forms of encode_gaussian_ragged_kernel and decode_gaussian_ragged_kernel, launched between the kernels that turn a jump table
// into chunks and chunk statuses into stream statuses (all in cst_persymbol_ragged.hpp), and the eight entry points.  A unit of its
// own: twenty-four more instantiations of the two kernels would have doubled the build's longest compile.
#include "cst_persymbol_ragged.hpp"

namespace cst {

template <int KIND, class FAM, class PT>
static cst_status encode_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols, const PT* d_a,
                                     const PT* d_b, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, uint32_t* d_words,
                                     const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, size_t jump_interval,
                                     const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_a, uint64_t* d_jump_b,
                                     int32_t* d_status, hipStream_t hs) {
    if (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b)) return CST_ERR_INVALID_ARGUMENT;
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
    return note_kernel(FamilyNames<FAM, PT>::ragged_jump[KIND == kRange][0], dispatch_word_size(cfg, [&](auto W, auto S) {
        return launch_with_lds(encode_gaussian_ragged_kernel<W, S, KIND, FAM, true, PT>, blocks, kFuBlock, lds, a, hs);
    }));
}

// (the table kernels around decode_gaussian_ragged_kernel<JUMP>: decode_jump_chunks, cst_persymbol_ragged.hpp)
template <int KIND, class FAM, class PT>
static cst_status decode_ragged_jump(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                     const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                     const PT* d_a, const PT* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                     size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                     const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    const cst_status plain = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                        stride_words, d_n_words, d_status, nullptr, n_streams);
    return decode_jump_chunks<KIND>(cfg, plain, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams,
                                    jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_a, d_jump_b, d_scratch, d_status,
                                    FamilyNames<FAM, PT>::ragged_jump[KIND == kRange][1], hs,
                                    [&](const PerSymbolDecodeArgs& p, const PerSymbolJumpScratch& v) {
        GaussianRaggedChunkArgs a{};
        a.p = p; a.p.min_symbol = min_symbol; a.p.n_symbols = (int32_t)((int64_t)max_symbol - min_symbol + 1); a.p.means = d_a; a.p.stds = d_b;
        a.sym_lo = v.sym_lo; a.len = v.len;
        const size_t blocks = (p.n_streams + kRgDecThreads - 1) / kRgDecThreads;
        const size_t lds = FAM::kErfTab ? kRgDecLdsBytes : kRgDecLdsBytesNoTab;
        return dispatch_word_size(cfg, [&](auto W, auto S) {
            return launch_with_lds(decode_gaussian_ragged_kernel<W, S, KIND, FAM, kRgJump, PT>, blocks, kRgDecThreads, lds, a, hs);
        });
    });
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

// ---- the float32 twins (the header's "float32 parameters"): the originals' arguments with the arrays untyped, the same host templates ----

cst_status cst_ans_encode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                   const void* d_means, const void* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                   const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                   uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                   uint64_t* d_jump_state, int32_t* d_status, void* stream) {
    return encode_ragged_jump<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), d_sym_offsets, n_streams, d_order, d_words,
                                                    d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state,
                                                    nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_ans_encode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                 const void* d_a, const void* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                                 const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                 uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                 uint64_t* d_jump_state, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged_jump, kAns, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state, nullptr, d_status,
                             (hipStream_t)stream);
}

cst_status cst_ans_decode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                   const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                   const void* d_means, const void* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                   const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status,
                                                   void* stream) {
    return decode_ragged_jump<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_means),
                                                    f32(d_stds), d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                    d_jump_pos, d_jump_state, nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                 const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                 const void* d_a, const void* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                 size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status,
                                                 void* stream) {
    return CST_FAMILY_CALL(decode_ragged_jump, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_a),
                             f32(d_b), d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_state,
                             nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                     const void* d_means, const void* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                     const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                     uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                     uint64_t* d_jump_lower, uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return encode_ragged_jump<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), d_sym_offsets, n_streams, d_order, d_words,
                                                      d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower,
                                                      d_jump_range, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                   const void* d_a, const void* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                                   const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                   uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                   uint64_t* d_jump_lower, uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(encode_ragged_jump, kRange, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), d_sym_offsets, n_streams, d_order, d_words,
                             d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower, d_jump_range, d_status,
                             (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged_jump_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                     const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                     const void* d_means, const void* d_stds, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                     size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                     void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_jump<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                      f32(d_means), f32(d_stds), d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                      d_jump_pos, d_jump_lower, d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged_jump_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                   const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                   const void* d_a, const void* d_b, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                   const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                   void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_jump, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, f32(d_a),
                             f32(d_b), d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_lower,
                             d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

} // extern "C"
