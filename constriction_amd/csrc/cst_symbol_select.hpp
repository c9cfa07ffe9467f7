// cst_symbol_select.hpp -- random access into a ragged batch of a symbol code (Huffman, Exp-Golomb): what
// cst_{huffman,exp_golomb}_decode_ragged_select share.
//
// The queries, pieces and statuses are those of cst_ragged_select.hpp; only the table differs.  A jump point of a prefix code is one
// bit index (d_jump_bits, 64 bits wide) and no coder state, so the queries kernel here judges every entry a query touches against its
// stream's BIT limit -- 32 n_words for a queue, the position of the seal for a stack -- before any word at the entry is read, and a
// stack without a seal is refused whether there is a table or not.  The pieces kernel is ragged_select_pieces_kernel<false> (it
// reads no table), the status kernel ragged_select_status_kernel.
#pragma once
#include "cst_ragged_select.hpp"

namespace cst {

// the highest bit index a reader of the container may start at.  A stack's is the position of its seal, the HIGHEST set bit of its
// last word.  false: a stack without words or with a zero last word
template <bool STACK>
__device__ __forceinline__ bool symbol_bit_limit(const uint32_t* words, size_t n_words, uint64_t& bits) {
    if (!STACK) { bits = 32ull * n_words; return true; }
    if (n_words == 0) return false;
    const uint32_t last = words[n_words - 1];
    if (last == 0u) return false;
    bits = 32ull * (n_words - 1) + (31u - (uint32_t)__clz((int)last));
    return true;
}

// what a lane of the SELECT form of a chunk-lane decoder reads: its piece's record, the caller's table by `entry`, and where its
// status goes
struct SymbolSelectLanes {
    const uint64_t *out_lo, *word_off;
    const uint32_t *entry, *skip, *len, *n_words;
    const uint64_t* jump_bits;
    int32_t* status;
    size_t n_pieces;
};
inline SymbolSelectLanes symbol_select_lanes(const RaggedSelectPieces& v, const uint64_t* jump_bits, size_t n_pieces) {
    return SymbolSelectLanes{v.out_lo, v.word_off, v.entry, v.skip, v.len, v.n_words, jump_bits, v.status, n_pieces};
}

template <bool STACK>
__global__ void symbol_select_queries_kernel(const RaggedSelect b, const uint32_t* __restrict__ words, const uint64_t* __restrict__ jump_bits,
                                             int32_t* __restrict__ status) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= b.n_queries) return;
    SelectQuery r = select_query(b, q);
    if (r.status == CST_STREAM_OK) {
        const uint64_t p0 = b.piece_offsets[q], p1 = b.piece_offsets[q + 1];
        if (p1 < p0 || p1 > b.n_pieces_total || p1 - p0 != r.n_pieces) r.status = CST_STREAM_INVALID_DATA;
    }
    uint64_t bits = 0;
    if (r.status == CST_STREAM_OK) {
        const WordSlice ws = word_slice(b.word_offsets, b.stride_words, b.n_words, r.s, b.words_capacity);
        // (the last word of a checked slice: the only word read here)
        if (ws.bad || !symbol_bit_limit<STACK>(words + ws.off, ws.n, bits)) r.status = CST_STREAM_INVALID_DATA;
    }
    if (r.status == CST_STREAM_OK && b.interval != 0) {
        // the stream's slice of the table is ceil(len / I) entries inside the table, and no entry the query touches lies beyond
        // the stream's bits
        const uint64_t c0 = b.chunk_offsets[r.s], c1 = b.chunk_offsets[r.s + 1];
        if (c1 < c0 || c1 > b.n_chunks_total || c1 - c0 != (r.doc_len + b.interval - 1) / b.interval) r.status = CST_STREAM_INVALID_DATA;
        else {
            const uint64_t e0 = c0 + r.first / b.interval;          // (n_pieces > 0 implies first / I + n_pieces <= ceil(len / I))
            for (uint64_t j = 0; j < r.n_pieces; ++j)
                if (jump_bits[e0 + j] > bits) r.status = CST_STREAM_INVALID_DATA;
        }
    }
    status[q] = r.status;
}

// what the two select calls refuse alike before the device is touched; `table` = how many of the table's two pointers are given
inline bool symbol_select_args_ok(size_t jump_interval, int table, size_t n_chunks_total, const void* d_query_first, const void* d_query_count,
                                  size_t n_pieces_total) {
    if (jump_interval != 0 && (jump_interval % 32 != 0 || jump_interval > 0x7fffffffull)) return false;
    if (table != 0 && table != 2) return false;                 // a table is an interval and BOTH its arrays, or nothing at all
    if ((jump_interval != 0) != (table != 0)) return false;
    if ((table != 0 && n_chunks_total > 0xffffffffull) || n_pieces_total > 0xffffffffull) return false;
    return (d_query_first == nullptr) == (d_query_count == nullptr);
}

inline RaggedSelect symbol_select_batch(const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                        const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets,
                                        size_t n_chunks_total, const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                        const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total,
                                        const uint64_t* d_out_offsets) {
    RaggedSelect b{};
    b.sym_offsets = d_sym_offsets; b.word_offsets = d_word_offsets; b.stride_words = stride_words; b.n_words = d_n_words; b.n_streams = n_streams;
    // (slab form without a capacity: the slabs themselves bound every slice, as in the jump decoders)
    b.words_capacity = words_capacity ? words_capacity : (d_word_offsets ? 0 : n_streams * stride_words);
    b.interval = (uint32_t)jump_interval; b.chunk_offsets = d_chunk_offsets; b.n_chunks_total = n_chunks_total; b.jump_pos = nullptr;
    b.query_stream = d_query_stream; b.query_first = d_query_first; b.query_count = d_query_count; b.n_queries = n_queries;
    b.piece_offsets = d_piece_offsets; b.n_pieces_total = n_pieces_total; b.out_offsets = d_out_offsets;
    return b;
}

// the three launches around the decoding kernel; `decode` launches it over n_pieces_total lanes
template <class Decode>
static cst_status symbol_select_run(bool stack, const RaggedSelect& b, const uint32_t* d_words, const uint64_t* d_jump_bits,
                                    const RaggedSelectPieces& v, int32_t* d_status, hipStream_t hs, Decode decode) {
    const unsigned q_grid = (unsigned)((b.n_queries + 255) / 256);
    if (stack) hipLaunchKernelGGL(symbol_select_queries_kernel<true>, dim3(q_grid), dim3(256), 0, hs, b, d_words, d_jump_bits, d_status);
    else hipLaunchKernelGGL(symbol_select_queries_kernel<false>, dim3(q_grid), dim3(256), 0, hs, b, d_words, d_jump_bits, d_status);
    CST_HIP_TRY(hipGetLastError());
    if (b.n_pieces_total > 0) {
        hipLaunchKernelGGL(ragged_select_pieces_kernel<false>, dim3((unsigned)((b.n_pieces_total + 255) / 256)), dim3(256), 0, hs, b, d_status, v);
        CST_HIP_TRY(hipGetLastError());
        const cst_status rc = decode();
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(ragged_select_status_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, v, d_status);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

} // namespace cst
