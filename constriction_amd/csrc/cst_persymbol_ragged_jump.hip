// cst_persymbol_ragged_jump.hip -- jump points (the reference's Pos / Seek) for the per-symbol coders of cst_persymbol_ragged.hip: the
// JUMP forms of encode_gaussian_ragged_kernel and decode_gaussian_ragged_kernel (cst_persymbol_ragged.hpp), the kernels that turn a jump
// table into chunks and chunk statuses into stream statuses, and the eight entry points.  A unit of its own: twenty-four more
// instantiations of the two kernels would have doubled the build's longest compile.
#include "cst_persymbol_ragged.hpp"

namespace cst {

// ------------------------------------------------------------------------------------------------
// jump points: the encoder's JUMP form notes the table; the decoder runs every table entry as a coder of its own
// ------------------------------------------------------------------------------------------------

// what the decoder keeps per table entry (d_scratch, cst_persymbol_ragged_jump_scratch_bytes): 80 bytes each
struct PerSymbolJumpScratch {
    uint64_t* sym_lo; uint64_t* word_off; uint64_t* state; cst_range_state* rstate;
    uint32_t* len; uint32_t* n_words; uint32_t* owner; int32_t* status;
    PerSymbolJumpScratch(void* d_scratch, size_t n) {
        unsigned char* b = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(d_scratch) + 15) & ~(uintptr_t)15);
        rstate = reinterpret_cast<cst_range_state*>(b);
        sym_lo = reinterpret_cast<uint64_t*>(rstate + n); word_off = sym_lo + n; state = word_off + n;
        len = reinterpret_cast<uint32_t*>(state + n); n_words = len + n; owner = n_words + n;
        status = reinterpret_cast<int32_t*>(owner + n);
    }
};
static_assert(sizeof(cst_range_state) == 40, "the scratch layout above");
constexpr uint32_t kPjNoOwner = 0xffffffffu;

// The chunks of a batch as coders of their own, one thread per table entry (rr_chunks_kernel's scheme, cst_range_ragged.hip): entry c
// belongs to the stream s with chunk_offsets[s] <= c < chunk_offsets[s + 1], found by bisection -- the table is caller data, and
// whatever it holds, every entry is written here and gets a symbol range inside ONE stream's symbols or none at all.  It decodes symbols
// [j I, min(j I + I, len)) of its stream, j = c - chunk_offsets[s]; entries that belong to no stream (behind the last chunk:
// n_chunks_total may be an upper bound) are empty.  The stream's slice of the words is checked HERE as the plain decoder checks it
// (per-slab bound included) and handed on as an absolute offset, or as the empty slice.
//   ANS:    the chunk's words are the first jump_pos[c] of its stream's (AnsCoder::seek, stack.rs:1107-1139) -- none where the jump
//           point lies beyond the stream's words -- and its state a copy of jump_state[c].
//   range:  RangeDecoder::seek (queue.rs:911-926) as gaussian_range_virtual_kernel does it: lower and range from the table, the point
//           re-read at the jump point, which is clamped to the stream's words; the chunk reads on from there, never past n_words[s].
template <int W, int S, int KIND>
__global__ void persymbol_jump_chunks_kernel(const uint32_t* __restrict__ words, const uint64_t* __restrict__ sym_offsets,
                                             const uint64_t* __restrict__ word_offsets, size_t stride_words, uint64_t words_capacity,
                                             const uint32_t* __restrict__ n_words, const uint64_t* __restrict__ chunk_offsets, size_t n_streams,
                                             size_t n_chunks_total, uint32_t interval, const uint32_t* __restrict__ jump_pos,
                                             const uint64_t* __restrict__ jump_a, const uint64_t* __restrict__ jump_b, PerSymbolJumpScratch v) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks_total) return;
    size_t s = 0, hi = n_streams;          // the last stream with chunk_offsets[s] <= c
    while (hi - s > 1) {
        const size_t mid = s + (hi - s) / 2;
        if (chunk_offsets[mid] <= c) s = mid; else hi = mid;
    }
    const uint64_t c0 = chunk_offsets[s], c1 = chunk_offsets[s + 1];
    const uint64_t lo = sym_offsets[s], end = sym_offsets[s + 1];
    const uint64_t start = (c - c0) * interval;
    const bool mine = c >= c0 && c < c1 && end >= lo && end - lo <= 0xffffffffull && start < end - lo;
    const WordSlice ws = mine ? word_slice(word_offsets, stride_words, n_words, s, words_capacity) : WordSlice{0, 0u, false};
    const uint64_t left = mine ? end - lo - start : 0;
    v.sym_lo[c] = mine ? lo + start : 0;
    v.len[c] = (uint32_t)(left < interval ? left : interval);
    v.word_off[c] = ws.off;
    v.owner[c] = mine ? (uint32_t)s : kPjNoOwner;
    const uint32_t jp = mine ? jump_pos[c] : 0u;
    if constexpr (KIND == kAns) {
        v.n_words[c] = jp <= ws.n ? jp : 0u;
        v.state[c] = mine ? jump_a[c] : 0;
    } else {
        uint32_t pos = jp < ws.n ? jp : ws.n;
        uint64_t pt = 0;
        int num_read = 0;
        const uint64_t mask = S == 64 ? ~0ull : ((1ull << (S % 64)) - 1ull);
        while (pos < ws.n) {                                          // read_point, queue.rs:847-868
            pt = ((pt << (W % 64)) | (uint64_t)words[ws.off + pos++]) & mask;
            if (++num_read == S / W) break;
        }
        if (num_read < S / W && num_read != 0) pt = (pt << (S - num_read * W)) & mask;
        cst_range_state r{};
        r.lower = mine ? jump_a[c] & mask : 0; r.range = mine ? jump_b[c] & mask : mask; r.point = pt; r.position = pos;
        v.rstate[c] = r;
        v.n_words[c] = ws.n;
    }
}

// a stream's status: the worst of its chunks'.  A table that does not describe the stream (chunks != ceil(len / I), entries beyond
// n_chunks_total or given to another stream), a jump point beyond the stream's words, or words that leave the buffer, are caller data
// gone wrong: CST_STREAM_INVALID_DATA.  (A stream too long for one coder: CST_STREAM_CAPACITY, as the plain decoder says.)
__global__ void persymbol_jump_status_kernel(PerSymbolJumpScratch v, const uint64_t* __restrict__ sym_offsets, const uint64_t* __restrict__ word_offsets,
                                             size_t stride_words, uint64_t words_capacity, const uint64_t* __restrict__ chunk_offsets,
                                             const uint32_t* __restrict__ jump_pos, const uint32_t* __restrict__ n_words, size_t n_streams,
                                             size_t n_chunks_total, uint32_t interval, int32_t* __restrict__ status) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const uint64_t lo = sym_offsets[s], end = sym_offsets[s + 1];
    const uint64_t c0 = chunk_offsets[s], c1 = chunk_offsets[s + 1];
    int32_t worst = CST_STREAM_OK;
    if (word_slice(word_offsets, stride_words, n_words, s, words_capacity).bad) worst = CST_STREAM_INVALID_DATA;
    else if (end < lo || end - lo > 0xffffffffull) worst = CST_STREAM_CAPACITY;
    else if (c1 < c0 || c1 > n_chunks_total || c1 - c0 != (end - lo + interval - 1) / interval) worst = CST_STREAM_INVALID_DATA;
    else
        for (uint64_t c = c0; c < c1; ++c) {
            worst = max(worst, v.status[c]);
            if (v.owner[c] != (uint32_t)s || jump_pos[c] > n_words[s]) worst = CST_STREAM_INVALID_DATA;
        }
    status[s] = worst;
}

// what the jump calls refuse on top of the plain calls' refusals
static bool jump_interval_bad(size_t jump_interval) { return jump_interval == 0 || jump_interval % kFuTile != 0 || jump_interval > 0x7fffffffull; }

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
    hipLaunchKernelGGL(persymbol_jump_status_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, hs, v, d_sym_offsets, d_word_offsets,
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
