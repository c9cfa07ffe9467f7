// cst_persymbol_ragged_select.hip -- random access into the ragged per-symbol batches of cst_persymbol_ragged.hip: the
// SELECT form of decode_gaussian_ragged_kernel, one lane per PIECE of a query (cst_ragged_select.hpp's cut), between that header's
// queries and status kernels and the per-symbol piece builder (cst_persymbol_ragged_select.hpp, shared with the Categorical select
// calls of cst_persymbol_categorical_ragged.hip), and the four entry points.  A unit of its own: twelve more
// instantiations of the decoding kernel belong on no other unit's compile time.
#include "cst_persymbol_ragged_select.hpp"

namespace cst {

template <int KIND, class FAM, class PT>
static cst_status decode_ragged_select(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                       const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                       const PT* d_a, const PT* d_b, const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                       const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos, const uint64_t* d_jump_a,
                                       const uint64_t* d_jump_b, const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                       const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total,
                                       int32_t* d_symbols_out, const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    // a table is an interval and ALL its arrays (jump_table_bad: the jump decoders' rule, whole tiles of 16 included), or nothing at all
    const bool table = jump_interval != 0 || d_chunk_offsets || d_jump_pos || d_jump_a || d_jump_b;
    if (table && (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b) || n_chunks_total > 0xffffffffull))
        return CST_ERR_INVALID_ARGUMENT;
    if (n_pieces_total > 0xffffffffull || (d_query_first == nullptr) != (d_query_count == nullptr)) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_ragged_gaussian_args(cfg, min_symbol, max_symbol, d_symbols_out, d_a, d_b, d_sym_offsets, d_words, d_word_offsets,
                                                   stride_words, d_n_words, d_status, nullptr, n_streams)) return st;
    if (n_queries > 0 && (!d_query_stream || !d_piece_offsets || !d_out_offsets || !d_scratch)) return CST_ERR_INVALID_ARGUMENT;
    if (n_queries == 0) return CST_OK;
    if (n_queries > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    RaggedSelect b{};
    b.sym_offsets = d_sym_offsets; b.word_offsets = d_word_offsets; b.stride_words = stride_words; b.n_words = d_n_words; b.n_streams = n_streams;
    // (slab form without a capacity: the slabs themselves bound every slice, as in the jump decoders)
    b.words_capacity = words_capacity ? words_capacity : (d_word_offsets ? 0 : (uint64_t)n_streams * stride_words);
    b.interval = (uint32_t)jump_interval; b.chunk_offsets = d_chunk_offsets; b.n_chunks_total = n_chunks_total; b.jump_pos = d_jump_pos;
    b.query_stream = d_query_stream; b.query_first = d_query_first; b.query_count = d_query_count; b.n_queries = n_queries;
    b.piece_offsets = d_piece_offsets; b.n_pieces_total = n_pieces_total; b.out_offsets = d_out_offsets;
    const PerSymbolSelectPieces v(d_scratch, n_pieces_total);
    const unsigned q_grid = (unsigned)((n_queries + 255) / 256);
    hipLaunchKernelGGL(ragged_select_queries_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, d_status);
    CST_HIP_TRY(hipGetLastError());
    if (n_pieces_total > 0) {
        const unsigned p_grid = (unsigned)((n_pieces_total + 255) / 256);
        dispatch_word_size(cfg, [&](auto W, auto S) {
            hipLaunchKernelGGL((persymbol_select_pieces_kernel<W, S, KIND>), dim3(p_grid), dim3(256), 0, hs, b, d_words, d_jump_a, d_jump_b, d_status, v);
            return 0;
        });
        CST_HIP_TRY(hipGetLastError());
        // (the slices handed on are absolute offsets that passed the check, or empty: the capacity bounds them once more)
        GaussianRaggedSelectArgs a{};
        a.p.words = d_words; a.p.offsets = v.word_off; a.p.stride_words = 0; a.p.n_words = v.n_words; a.p.words_capacity = b.words_capacity;
        a.p.symbols = d_symbols_out; a.p.n_streams = n_pieces_total; a.p.precision = cfg.precision;
        a.p.min_symbol = min_symbol; a.p.n_symbols = (int32_t)((int64_t)max_symbol - min_symbol + 1); a.p.means = d_a; a.p.stds = d_b;
        a.p.status = v.status; a.p.state = v.state; a.p.rstate = v.rstate;
        a.par_lo = v.par_lo; a.out_lo = v.out_lo; a.skip = v.skip; a.len = v.len; a.raw = jump_interval != 0;
        const size_t blocks = (n_pieces_total + kRgDecThreads - 1) / kRgDecThreads;
        const size_t lds = FAM::kErfTab ? kRgDecLdsBytes : kRgDecLdsBytesNoTab;
        const cst_status rc = dispatch_word_size(cfg, [&](auto W, auto S) {
            return launch_with_lds(decode_gaussian_ragged_kernel<W, S, KIND, FAM, kRgSelect, PT>, blocks, kRgDecThreads, lds, a, hs);
        });
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(ragged_select_status_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, v.folded(), d_status);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(FamilyNames<FAM, PT>::ragged_select[KIND == kRange], CST_OK);
}

} // namespace cst

using namespace cst;

extern "C" {

size_t cst_persymbol_ragged_select_scratch_bytes(size_t n_pieces_total) { return kPsSelectPieceBytes * n_pieces_total + 128; }

cst_status cst_ans_decode_gaussian_ragged_select(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                 const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                 const double* d_means, const double* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                 size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                                 const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                 const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                 const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_select<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                      d_means, d_stds, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                      d_jump_pos, d_jump_state, nullptr, d_query_stream, d_query_first, d_query_count, n_queries,
                                                      d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status,
                                                      (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged_select(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                   const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity,
                                                   const uint32_t* d_n_words, const double* d_means, const double* d_stds,
                                                   const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                   const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                                   const uint64_t* d_jump_lower, const uint64_t* d_jump_range, const uint32_t* d_query_stream,
                                                   const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                   const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                   const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_select<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                        d_means, d_stds, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                        d_jump_pos, d_jump_lower, d_jump_range, d_query_stream, d_query_first, d_query_count,
                                                        n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch,
                                                        d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged_select(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                               const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                               const double* d_a, const double* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                               size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                               const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                               const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                               const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                               const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_select, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                             d_a, d_b, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_state, nullptr,
                             d_query_stream, d_query_first, d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets,
                             d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged_select(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                 const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity,
                                                 const uint32_t* d_n_words, const double* d_a, const double* d_b, const uint64_t* d_sym_offsets,
                                                 size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                 const uint32_t* d_query_stream, const uint64_t* d_query_first, const uint64_t* d_query_count,
                                                 size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                 const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_select, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                             d_a, d_b, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_lower,
                             d_jump_range, d_query_stream, d_query_first, d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out,
                             d_out_offsets, d_scratch, d_status, (hipStream_t)stream);
}

// ---- the float32 twins (the header's "float32 parameters"): the originals' arguments with the arrays untyped, the same host templates ----

cst_status cst_ans_decode_gaussian_ragged_select_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                     const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                     const void* d_means, const void* d_stds, const uint64_t* d_sym_offsets, size_t n_streams,
                                                     size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                                     const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                     const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                     const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_select<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                      f32(d_means), f32(d_stds), d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                      d_jump_pos, d_jump_state, nullptr, d_query_stream, d_query_first, d_query_count, n_queries,
                                                      d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status,
                                                      (hipStream_t)stream);
}

cst_status cst_ans_decode_family_ragged_select_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                   const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                   const void* d_a, const void* d_b, const uint64_t* d_sym_offsets, size_t n_streams,
                                                   size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                   const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                                   const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                   const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                   const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_select, kAns, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                             f32(d_a), f32(d_b), d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_state, nullptr,
                             d_query_stream, d_query_first, d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets,
                             d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_gaussian_ragged_select_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                       const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity,
                                                       const uint32_t* d_n_words, const void* d_means, const void* d_stds,
                                                       const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                       const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                                       const uint64_t* d_jump_lower, const uint64_t* d_jump_range, const uint32_t* d_query_stream,
                                                       const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                       const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                       const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_ragged_select<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                        f32(d_means), f32(d_stds), d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                        d_jump_pos, d_jump_lower, d_jump_range, d_query_stream, d_query_first, d_query_count,
                                                        n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch,
                                                        d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_family_ragged_select_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol,
                                                     const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity,
                                                     const uint32_t* d_n_words, const void* d_a, const void* d_b, const uint64_t* d_sym_offsets,
                                                     size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                     const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                     const uint32_t* d_query_stream, const uint64_t* d_query_first, const uint64_t* d_query_count,
                                                     size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                     const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return CST_FAMILY_CALL(decode_ragged_select, kRange, cfg, min_symbol, max_symbol, d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                             f32(d_a), f32(d_b), d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_lower,
                             d_jump_range, d_query_stream, d_query_first, d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out,
                             d_out_offsets, d_scratch, d_status, (hipStream_t)stream);
}

} // extern "C"
