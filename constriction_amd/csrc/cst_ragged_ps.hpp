// cst_ragged_ps.hpp -- streams of DIFFERENT lengths, ONE TABLE PER STREAM (cst_ragged_ps.hip): what the ragged entry points of
// cst_api.hip and the jump decoders of cst_ans_ragged.hip / cst_range_ragged.hip call for a model with `per_stream` set.
#pragma once
#include "cst_common.hpp"

namespace cst {

// what every ragged call asks of a per-stream model: table s belongs to stream s, 16-bit rows (P <= 16), a preset of these kernels
// (`need_recip`: the ANS encoder's reciprocal table)
inline bool ragged_ps_model_ok(const cst_model* model, cst_coder_config cfg, size_t n_streams, bool need_recip) {
    return model->per_stream && model->n_tables == n_streams && n_streams <= 0xfffffffeull && model->d_cdf16 && model->precision <= 16 &&
           (!need_recip || model->d_recip) &&
           ((cfg.word_bits == 32 && cfg.state_bits == 64) || (cfg.word_bits == 16 && cfg.state_bits == 32));
}

// interval == 0: plain; otherwise AnsCoder::pos() in front of every chunk goes to d_jump_pos / d_jump_state
cst_status ans_encode_ragged_ps(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                int32_t* d_status, const uint32_t* d_order, uint32_t interval, const uint64_t* d_chunk_offsets,
                                uint32_t* d_jump_pos, uint64_t* d_jump_state, hipStream_t hs);
cst_status ans_decode_ragged_ps(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, const uint32_t* d_order, hipStream_t hs);
// one lane per table entry (chunk); d_chunk_status [n_chunks_total]: an entry no stream owns reports CST_STREAM_INVALID_DATA
cst_status ans_decode_ragged_ps_chunks(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                       size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                       const uint64_t* d_sym_offsets, size_t n_streams, uint32_t interval, const uint64_t* d_chunk_offsets,
                                       size_t n_chunks_total, const uint32_t* d_jump_pos, const uint64_t* d_jump_state,
                                       int32_t* d_chunk_status, hipStream_t hs);

// interval == 0: plain; otherwise RangeEncoder::pos() in front of every chunk goes to d_jump_pos / d_jump_lower / d_jump_range
cst_status range_encode_ragged_ps(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                  size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                  int32_t* d_status, const uint32_t* d_order, uint32_t interval, const uint64_t* d_chunk_offsets,
                                  uint32_t* d_jump_pos, uint64_t* d_jump_lower, uint64_t* d_jump_range, hipStream_t hs);
cst_status range_decode_ragged_ps(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                  size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                  const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, const uint32_t* d_order, hipStream_t hs);
// one lane per chunk as rr_chunks_kernel (cst_range_ragged.hip) describes them: symbol range, the owner's checked slice of the words, the
// owner itself (0xffffffff: none)
cst_status range_decode_ragged_ps_chunks(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, size_t words_capacity,
                                         int32_t* d_symbols, size_t n_chunks_total, const uint64_t* d_chunk_sym_lo, const uint32_t* d_chunk_len,
                                         const uint64_t* d_chunk_word_off, const uint32_t* d_chunk_n_words, const uint32_t* d_chunk_owner,
                                         const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                         int32_t* d_chunk_status, hipStream_t hs);

} // namespace cst
