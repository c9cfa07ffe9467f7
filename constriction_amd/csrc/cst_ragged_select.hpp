// cst_ragged_select.hpp -- random access into a ragged batch: what cst_{ans,range}_decode_ragged_select share.
//
// A query (stream, first, count) asks for symbols [first, first + count) of one document.  With a jump table of interval I it is cut
// into PIECES, one per chunk it touches: piece 0 starts at jump point first / I and decodes first % I symbols it does not store, the
// others are whole chunks or a chunk's head.  Without a table a query is one piece from the start of its document.  Every piece is a
// lane of the SELECT form of the coder's ragged decoding kernel.  Around that kernel, the same three small ones for both coders:
//   1. ragged_select_queries_kernel   one thread per query: everything the caller says about it is checked (all of it is caller data)
//                                     -> d_status[q] = OK or the refusal; a refused query gets no piece and writes nothing;
//   2. ragged_select_pieces_kernel    one thread per piece: its query by bisection in d_piece_offsets (rr_chunks_kernel's scheme), then
//                                     table entry, skip, length, output position and its stream's checked slice of the words -> scratch;
//   3. ragged_select_status_kernel    one thread per query: the worst of its pieces' statuses.
// The kernels are templates so that each translation unit that launches them carries its own copy (no relocatable device code):
// cst_ans_ragged.hip, cst_range_ragged.hip, cst_persymbol_ragged_select.hip, cst_persymbol_categorical_ragged.hip and
// cst_indexed_ragged.hip, whose pieces carry more (their own piece builder, cst_persymbol_ragged_select.hpp), and cst_huffman_ragged.hip and cst_exp_golomb.hip, whose
// tables hold bit indices (their own queries kernel, cst_symbol_select.hpp).
#pragma once
#include "cst_common.hpp"

namespace cst {

constexpr uint32_t kSelectNoEntry = 0xffffffffu;      // a piece that starts where its document starts (no table), or belongs to no query

// the scratch of a call: one record per piece (structure of arrays)
struct RaggedSelectPieces {
    uint64_t *out_lo, *word_off;     // first symbol of the piece in the output; the words of its stream (checked, or the empty slice)
    uint32_t *entry, *skip, *len;    // table entry (kSelectNoEntry: none); symbols decoded and dropped, then symbols stored
    uint32_t *n_words, *owner;       // words the piece's coder may read; the query it belongs to (kSelectNoEntry: none)
    int32_t* status;                 // written by the decoding kernel
    RaggedSelectPieces(void* d_scratch, size_t n) {
        unsigned char* b = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(d_scratch) + 15) & ~(uintptr_t)15);
        out_lo = reinterpret_cast<uint64_t*>(b); word_off = out_lo + n;
        entry = reinterpret_cast<uint32_t*>(word_off + n); skip = entry + n; len = skip + n; n_words = len + n; owner = n_words + n;
        status = reinterpret_cast<int32_t*>(owner + n);
    }
};
static_assert(kRaggedSelectPieceBytes == 2 * 8 + 6 * 4, "a piece record is two 64-bit and six 32-bit fields");

// what a lane of the SELECT form of a decoding kernel reads: its piece's record, and the caller's table by `entry`
struct RaggedSelectLanes {
    const uint64_t *out_lo, *word_off;
    const uint32_t *entry, *skip, *len, *n_words;
    const uint32_t* jump_pos;        // range coder: words in front of the jump point
    const uint64_t* jump_a;          // ANS: the coder state there; range coder: lower
    const uint64_t* jump_b;          // range coder: range
};
inline RaggedSelectLanes select_lanes(const RaggedSelectPieces& v, const uint32_t* jump_pos, const uint64_t* jump_a, const uint64_t* jump_b) {
    return RaggedSelectLanes{v.out_lo, v.word_off, v.entry, v.skip, v.len, v.n_words, jump_pos, jump_a, jump_b};
}

// what a query asks for, once it has been read (every index checked before it is used)
struct SelectQuery {
    int32_t status;                  // CST_STREAM_OK, or why the query decodes nothing
    size_t s;
    uint64_t first, count, doc_len;
    uint64_t n_pieces;
};

// pieces of a query: one per chunk it touches; without a table one, from the start of the document
__device__ __forceinline__ uint64_t select_piece_count(uint64_t first, uint64_t count, uint32_t interval) {
    if (count == 0) return 0;
    if (interval == 0) return 1;
    return (first % interval + count + interval - 1) / interval;         // (count <= 2^32 - 1 here: no wrap)
}

// stream, range and output slice of query q (its piece offsets, words and table entries: ragged_select_queries_kernel)
__device__ __forceinline__ SelectQuery select_query(const RaggedSelect& b, size_t q) {
    SelectQuery r{CST_STREAM_INVALID_DATA, 0, 0, 0, 0, 0};
    r.s = b.query_stream[q];
    if (r.s >= b.n_streams) return r;
    const uint64_t lo = b.sym_offsets[r.s], end = b.sym_offsets[r.s + 1];
    if (end < lo || end - lo > 0xffffffffull) { r.status = CST_STREAM_CAPACITY; return r; }       // as the plain decoders say it
    r.doc_len = end - lo;
    r.first = b.query_first ? b.query_first[q] : 0;
    r.count = b.query_count ? b.query_count[q] : r.doc_len;
    if (r.first > r.doc_len || r.count > r.doc_len - r.first) return r;                             // (first + count may wrap: not formed)
    const uint64_t o0 = b.out_offsets[q], o1 = b.out_offsets[q + 1];
    if (o1 < o0 || o1 - o0 != r.count) return r;                                                    // the slice the query owns is `count` long
    r.n_pieces = select_piece_count(r.first, r.count, b.interval);
    r.status = CST_STREAM_OK;
    return r;
}

template <int UNUSED = 0>
__global__ void ragged_select_queries_kernel(const RaggedSelect b, int32_t* __restrict__ status) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= b.n_queries) return;
    SelectQuery r = select_query(b, q);
    if (r.status == CST_STREAM_OK) {
        const uint64_t p0 = b.piece_offsets[q], p1 = b.piece_offsets[q + 1];
        if (p1 < p0 || p1 > b.n_pieces_total || p1 - p0 != r.n_pieces) r.status = CST_STREAM_INVALID_DATA;
    }
    if (r.status == CST_STREAM_OK && word_slice(b.word_offsets, b.stride_words, b.n_words, r.s, b.words_capacity).bad)
        r.status = CST_STREAM_INVALID_DATA;
    if (r.status == CST_STREAM_OK && b.interval != 0) {
        // the stream's slice of the table is ceil(len / I) entries inside the table, and no entry the query touches claims more
        // words than the stream has
        const uint64_t c0 = b.chunk_offsets[r.s], c1 = b.chunk_offsets[r.s + 1];
        if (c1 < c0 || c1 > b.n_chunks_total || c1 - c0 != (r.doc_len + b.interval - 1) / b.interval) r.status = CST_STREAM_INVALID_DATA;
        else {
            const uint32_t nw = b.n_words[r.s];
            const uint64_t e0 = c0 + r.first / b.interval;          // (n_pieces > 0 implies first / I + n_pieces <= ceil(len / I))
            for (uint64_t j = 0; j < r.n_pieces; ++j)
                if (b.jump_pos[e0 + j] > nw) r.status = CST_STREAM_INVALID_DATA;
        }
    }
    status[q] = r.status;
}

// ANS: a piece's coder owns the words IN FRONT of its jump point (a stack reads downwards from there); the range coder's reads forward
// from it inside its stream's words
template <bool ANS>
__global__ void ragged_select_pieces_kernel(const RaggedSelect b, const int32_t* __restrict__ query_status, RaggedSelectPieces v) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= b.n_pieces_total) return;
    size_t q = 0, hi = b.n_queries;          // the last query with piece_offsets[q] <= p
    while (hi - q > 1) {
        const size_t mid = q + (hi - q) / 2;
        if (b.piece_offsets[mid] <= p) q = mid; else hi = mid;
    }
    const uint64_t p0 = b.piece_offsets[q], p1 = b.piece_offsets[q + 1];
    bool mine = query_status[q] == CST_STREAM_OK && p >= p0 && p < p1;
    uint64_t out_lo = 0, word_off = 0;
    uint32_t entry = kSelectNoEntry, skip = 0, len = 0, n_words = 0;
    if (mine) {
        const SelectQuery r = select_query(b, q);          // (passed once already: status OK, p1 - p0 == n_pieces)
        const uint64_t j = p - p0;
        const WordSlice ws = word_slice(b.word_offsets, b.stride_words, b.n_words, r.s, b.words_capacity);
        mine = r.status == CST_STREAM_OK && j < r.n_pieces && !ws.bad;
        if (mine) {
            word_off = ws.off; n_words = ws.n;
            if (b.interval == 0) {
                skip = (uint32_t)r.first; len = (uint32_t)r.count;          // (first + count <= the document's length <= 2^32 - 1)
                out_lo = b.out_offsets[q];
            } else {
                const uint64_t chunk = r.first / b.interval + j;
                const uint64_t start = j == 0 ? r.first : chunk * b.interval;
                const uint64_t stop = min((chunk + 1) * (uint64_t)b.interval, r.first + r.count);
                skip = j == 0 ? (uint32_t)(r.first % b.interval) : 0u;
                len = (uint32_t)(stop - start);
                out_lo = b.out_offsets[q] + (start - r.first);
                entry = (uint32_t)(b.chunk_offsets[r.s] + chunk);           // (< n_chunks_total <= 2^32 - 1)
                if constexpr (ANS) n_words = min(b.jump_pos[entry], ws.n);
            }
        }
    }
    v.out_lo[p] = out_lo; v.word_off[p] = word_off;
    v.entry[p] = entry; v.skip[p] = skip; v.len[p] = len; v.n_words[p] = n_words;
    v.owner[p] = mine ? (uint32_t)q : kSelectNoEntry;
}

// a query's status: its refusal, or the worst of its pieces' (a piece that the bisection gave to another query -- piece offsets that
// do not ascend -- is caller data gone wrong)
template <int UNUSED = 0>
__global__ void ragged_select_status_kernel(const RaggedSelect b, RaggedSelectPieces v, int32_t* __restrict__ status) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= b.n_queries) return;
    int32_t worst = status[q];
    if (worst != CST_STREAM_OK) return;
    const uint64_t p0 = b.piece_offsets[q], p1 = b.piece_offsets[q + 1];
    for (uint64_t p = p0; p < p1; ++p) {
        worst = max(worst, v.status[p]);
        if (v.owner[p] != (uint32_t)q) worst = CST_STREAM_INVALID_DATA;
    }
    status[q] = worst;
}

// the three launches around the decoding kernel; `decode` launches it over n_pieces_total lanes
template <bool ANS, class Decode>
static cst_status ragged_select_run(const RaggedSelect& b, const RaggedSelectPieces& v, int32_t* d_status, hipStream_t hs, Decode decode) {
    const unsigned q_grid = (unsigned)((b.n_queries + 255) / 256);
    hipLaunchKernelGGL(ragged_select_queries_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, d_status);
    CST_HIP_TRY(hipGetLastError());
    if (b.n_pieces_total > 0) {
        hipLaunchKernelGGL(ragged_select_pieces_kernel<ANS>, dim3((unsigned)((b.n_pieces_total + 255) / 256)), dim3(256), 0, hs, b, d_status, v);
        CST_HIP_TRY(hipGetLastError());
        const cst_status rc = decode();
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(ragged_select_status_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, v, d_status);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

} // namespace cst
