// cst_persymbol_ragged_select.hpp -- what the SELECT forms of the per-symbol ragged decoders share: the record of a
// piece and the kernel that builds it, for cst_persymbol_ragged_select.hip (Gaussian, Laplace, Cauchy),
// cst_persymbol_categorical_ragged.hip (Categorical, both quantisers) and cst_indexed_ragged.hip (indexed tables, DESIGN.md 4.31: the
// "parameters" are the indices).  A piece of a per-symbol batch needs what a piece of a
// shared-table batch does not: the element its PARAMETERS (or probability rows) start at -- the jump point's, not the first stored
// symbol's -- and the coder's raw state there, prepared as persymbol_jump_chunks_kernel prepares a chunk's.  Templates: each unit's
// code object carries its own copy (no relocatable device code).
#pragma once
#include "cst_persymbol_ragged.hpp"
#include "cst_ragged_select.hpp"

namespace cst {

// the scratch of a call: one record per piece (structure of arrays), 92 bytes; cst_persymbol_ragged_select_scratch_bytes rounds up
constexpr size_t kPsSelectPieceBytes = 96;
struct PerSymbolSelectPieces {
    cst_range_state* rstate;                          // the range coder at the jump point (with a table)
    uint64_t *par_lo, *out_lo, *word_off, *state;     // first parameter element; first stored symbol; the stream's words; ANS: the state
    uint32_t *skip, *len, *n_words, *owner;           // as RaggedSelectPieces
    int32_t* status;                                  // written by the decoding kernel
    PerSymbolSelectPieces(void* d_scratch, size_t n) {
        unsigned char* b = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(d_scratch) + 15) & ~(uintptr_t)15);
        rstate = reinterpret_cast<cst_range_state*>(b);
        par_lo = reinterpret_cast<uint64_t*>(rstate + n); out_lo = par_lo + n; word_off = out_lo + n; state = word_off + n;
        skip = reinterpret_cast<uint32_t*>(state + n); len = skip + n; n_words = len + n; owner = n_words + n;
        status = reinterpret_cast<int32_t*>(owner + n);
    }
    // what ragged_select_status_kernel reads of a piece: its owner and its status
    RaggedSelectPieces folded() const {
        RaggedSelectPieces r(nullptr, 0);
        r.owner = owner; r.status = status;
        return r;
    }
};
static_assert(sizeof(cst_range_state) + 4 * 8 + 5 * 4 <= kPsSelectPieceBytes, "a piece record");

// ragged_select_pieces_kernel for the per-symbol decoders: the same cut, and per piece also where its parameters start and the coder's
// raw state at its jump point --
//   ANS:    the first min(jump_pos[entry], n_words[s]) words of the stream and jump_a[entry] (AnsCoder::seek);
//   range:  lower / range from the table, the point re-read at the jump point clamped to the stream's words (RangeDecoder::seek), all
//           of the stream's words to read on in: persymbol_jump_chunks_kernel's lines.
// Without a table a piece is all of its stream's words from the document's first element; its coder starts as the plain decoder's.
template <int W, int S, int KIND>
__global__ void persymbol_select_pieces_kernel(const RaggedSelect b, const uint32_t* __restrict__ words, const uint64_t* __restrict__ jump_a,
                                               const uint64_t* __restrict__ jump_b, const int32_t* __restrict__ query_status,
                                               PerSymbolSelectPieces v) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= b.n_pieces_total) return;
    size_t q = 0, hi = b.n_queries;          // the last query with piece_offsets[q] <= p
    while (hi - q > 1) {
        const size_t mid = q + (hi - q) / 2;
        if (b.piece_offsets[mid] <= p) q = mid; else hi = mid;
    }
    const uint64_t p0 = b.piece_offsets[q], p1 = b.piece_offsets[q + 1];
    bool mine = query_status[q] == CST_STREAM_OK && p >= p0 && p < p1;
    uint64_t par_lo = 0, out_lo = 0, state = 0;
    WordSlice ws{0, 0u, false};
    uint32_t skip = 0, len = 0, n_words = 0;
    cst_range_state r{};
    if (mine) {
        const SelectQuery sq = select_query(b, q);         // (passed once already: status OK, p1 - p0 == n_pieces)
        const uint64_t j = p - p0;
        ws = word_slice(b.word_offsets, b.stride_words, b.n_words, sq.s, b.words_capacity);
        mine = sq.status == CST_STREAM_OK && j < sq.n_pieces && !ws.bad;
        if (!mine) ws = WordSlice{0, 0u, false};
        else if (b.interval == 0) {
            skip = (uint32_t)sq.first; len = (uint32_t)sq.count;        // (first + count <= the document's length <= 2^32 - 1)
            par_lo = b.sym_offsets[sq.s]; out_lo = b.out_offsets[q]; n_words = ws.n;
        } else {
            const uint64_t chunk = sq.first / b.interval + j;
            const uint64_t start = j == 0 ? sq.first : chunk * b.interval;
            const uint64_t stop = min((chunk + 1) * (uint64_t)b.interval, sq.first + sq.count);
            skip = j == 0 ? (uint32_t)(sq.first % b.interval) : 0u;
            len = (uint32_t)(stop - start);
            par_lo = b.sym_offsets[sq.s] + chunk * b.interval;
            out_lo = b.out_offsets[q] + (start - sq.first);
            const uint64_t entry = b.chunk_offsets[sq.s] + chunk;         // (< n_chunks_total: the queries kernel has looked)
            const uint32_t jp = b.jump_pos[entry];
            if constexpr (KIND == kAns) {
                n_words = min(jp, ws.n);
                state = jump_a[entry];
            } else {
                uint32_t pos = min(jp, ws.n);
                uint64_t pt = 0;
                int num_read = 0;
                const uint64_t mask = S == 64 ? ~0ull : ((1ull << (S % 64)) - 1ull);
                while (pos < ws.n) {                                      // read_point, queue.rs:847-868
                    pt = ((pt << (W % 64)) | (uint64_t)words[ws.off + pos++]) & mask;
                    if (++num_read == S / W) break;
                }
                if (num_read < S / W && num_read != 0) pt = (pt << (S - num_read * W)) & mask;
                r.lower = jump_a[entry] & mask; r.range = jump_b[entry] & mask; r.point = pt; r.position = pos;
                n_words = ws.n;
            }
        }
    }
    v.par_lo[p] = par_lo; v.out_lo[p] = out_lo; v.word_off[p] = ws.off; v.state[p] = state; v.rstate[p] = r;
    v.skip[p] = skip; v.len[p] = len; v.n_words[p] = n_words;
    v.owner[p] = mine ? (uint32_t)q : kSelectNoEntry;
}

} // namespace cst
