// cst_range_ragged.hip -- the batched RANGE coder with one shared table for streams of DIFFERENT lengths: one queue per document.
//
// The reference's RangeEncoder / RangeDecoder (src/stream/queue.rs) used as cst_ans_ragged.hip uses its AnsCoder: thousands of short
// documents, one coder each, one launch for all of them (the layout of the symbols, the slabs and the schedule `order` are those of
// cst_ans_ragged.hip: read its header first).  One lane per stream, a wave runs as many steps as its longest stream; these batches are
// bound by the LATENCY of a step, so everything a step waits for stays inside the CU:
//   * tables in LDS whenever they fit in 64 KiB beside the rings (the encoder's 16-byte entries; the decoder's cdf + 16-byte bucket
//     entries with second-level tables, or cdf + 16-bit bucket index), read from HBM / L2 otherwise;
//   * a QUEUE: symbols are coded first to last.  The encoder takes whole groups of eight from two unaligned 16-byte loads per lane
//     requested one group ahead, then the (len mod 8) symbols at the END of the row one by one (requested before the first group);
//     the decoder collects eight symbols in registers and stores them as two 16-byte pieces;
//   * one memory point per group (a gfx9 wave has ONE counter for its loads and stores): the values requested a group ago are
//     consumed, this group's requests and stores are issued, then eight steps run out of LDS and registers.
// Encoder steps: quads of the branch-free step_inline; a quad in which some lane leaves an Inverted run of two or more held-back
// words is rolled back and repeated with the general step (as range_encode_kernel does), and behind every general step the lane
// makes room in its ring, so that a run of ANY length comes out exactly (a burst may fill the ring up to its brim otherwise).
// Decoder steps: RangeDecLane::step, whose quantile is an f64 quotient -- the cost of a range step over an ANS step.
// Every stream's words, count and status are those of cst_range_{encode,decode}_batch for that stream alone (queue.rs:612-705,
// 458-523, 847-868, 968-1033).
// Jump points (RangeEncoder::pos / RangeDecoder::seek, queue.rs:172-196, 900-926) are a form of their own of the two coding kernels
// (JUMP, a compile-time parameter of the shared bodies: the plain kernels keep their registers, LDS, occupancy and timings): see
// RangeRaggedJump and RangeRaggedChunks below.  Random access -- selected documents and ranges of documents -- is a third form of the
// decoder's body (its MODE: kRrPlain, kRrJump, kRrSelect), around it the kernels of cst_ragged_select.hpp.
#include "cst_range_kernels.hpp"
#include "cst_ragged_select.hpp"
#include "cst_ragged_ps.hpp"

namespace cst {

struct RangeRaggedArgs {
    const int32_t* symbols_in;
    int32_t* symbols_out;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    size_t n_streams;
    const EncEntry* enc;
    const uint32_t* cdf;
    const uint16_t* bucket;
    int32_t bucket_bits, n_symbols, min_symbol, precision;
    uint32_t* words_out;
    const uint32_t* words_in;
    const uint64_t* word_offsets;    // [n_streams + 1] (encode: slab of stream s = [off[s], off[s + 1])) or null
    size_t stride_words;
    uint32_t* n_words_out;
    const uint32_t* n_words_in;
    int32_t* status;
    uint64_t words_capacity;
    const uint32_t* order;           // null, or [n_streams]: lane slot i codes stream order[i]
};

// The jump form of the encoder notes RangeEncoder::pos() in front of every chunk of `interval` symbols of every stream: chunk j of
// stream s is entry chunk_offsets[s] + j of pos / lower / range, chunk_offsets the exclusive prefix sum of ceil(len / interval) (the
// layout of cst_ans_ragged.hip).  pos = words emitted so far INCLUDING held-back ones, (lower, range) the RangeCoderState there.
struct RangeRaggedJump {
    uint32_t interval;               // a multiple of kRrGroup
    const uint64_t* chunk_offsets;   // [n_streams + 1]
    uint32_t* pos;
    uint64_t* lower;
    uint64_t* range;
};

// The jump form of the decoder runs every chunk as a coder of its own, one lane per chunk (`n_streams` of its RangeRaggedArgs is
// the number of chunks, `status` one entry per chunk, `order` null).  A range chunk reads FORWARD from its jump point and may read on
// past its chunk, never past its stream: a chunk carries its own symbol range and its STREAM's slice of the words.
struct RangeRaggedChunks {
    const uint64_t* sym_lo;          // first symbol of the chunk in the flat output
    const uint32_t* len;             // symbols of the chunk (0: a table entry that belongs to no stream)
    const uint64_t* word_off;        // the chunk's stream: offset and number of its words (already checked once, see rr_chunks_kernel)
    const uint32_t* n_words;
    const uint32_t* pos;             // the jump table
    const uint64_t* lower;
    const uint64_t* range;
};

// lane slot -> stream: the slot itself, or order[slot] (an entry that is not a stream leaves its lane idle)
__device__ __forceinline__ size_t rr_stream(const RangeRaggedArgs& a, size_t slot, bool& active) {
    active = slot < a.n_streams;
    if (!active || !a.order) return slot;
    const size_t s = a.order[slot];
    active = s < a.n_streams;
    return s;
}

__device__ __forceinline__ uint32_t rr_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

typedef int32_t rr_v4i __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) rr_v4i_unaligned { rr_v4i v; };      // 16-byte access at a 4-byte boundary

// "the values requested a group ago are needed HERE": the compiler's wait goes in front of this, not behind the new group's requests
__device__ __forceinline__ void rr_consume(rr_v4i& a, rr_v4i& b) {
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
}

constexpr int kRrGroup = 8;                      // symbols per memory point
constexpr size_t kRrStageLimit = 64 * 1024;      // tables up to this size are staged in LDS
// Encoder ring: a group of step_inline pushes at most 16 words on top of an incomplete chunk (3), a memory point moves up to
// kMaxChunksPerPoint chunks (20 words) out: 32 slots hold that, and the general step's bursts make room for themselves (push_slow)
constexpr int kRrEncSlots = 32;
constexpr size_t kRrEncRingBytes = (size_t)(kBlock / kWave) * kRrEncSlots * kWave * 4;
// (behind a quad of general steps less than half the ring is pending -- `relieve` below -- and the group's other quad adds at most 8)
static_assert(3 + 2 * kRrGroup < kRrEncSlots && kRrEncSlots / 2 + kRrGroup < kRrEncSlots && kRrEncSlots / 2 - 1 + kRrGroup <= 3 + 4 * kMaxChunksPerPoint,
              "the encoder's ring must hold a group's words, and a memory point must be able to move them out");

// the encoder: JUMP = false is range_encode_ragged_kernel, JUMP = true the form that notes the jump points of `jp` on its way
template <int W, int S, bool STAGED, bool JUMP>
__device__ __forceinline__ void rr_encode(const RangeRaggedArgs& a, const RangeRaggedJump& jp, unsigned char* smem) {
    constexpr int G = kRrGroup;
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (kRrEncSlots * kWave);
    const EncEntry* table = a.enc;
    if constexpr (STAGED) {
        EncEntry* t = reinterpret_cast<EncEntry*>(smem + kRrEncRingBytes);
        for (int i = threadIdx.x; i < a.n_symbols; i += blockDim.x) t[i] = a.enc[i];
        table = t;
        __syncthreads();
    }
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot - lane >= a.n_streams) return;
    bool active;
    const size_t s = rr_stream(a, slot, active);
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols;
    const uint64_t sym_lo = active ? a.sym_offsets[s] : 0, sym_hi = active ? a.sym_offsets[s + 1] : 0;
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    const uint64_t slab_lo = !active ? 0 : (a.word_offsets ? a.word_offsets[s] : (uint64_t)s * a.stride_words);
    // (offsets that run backwards -- corrupt metadata -- give the stream a slab of NO words: CST_STREAM_CAPACITY, nothing written)
    const uint64_t slab_hi = !active ? 0 : (a.word_offsets ? a.word_offsets[s + 1] : 0);
    const uint64_t slab_n = !active ? 0 : (a.word_offsets ? (slab_hi >= slab_lo ? slab_hi - slab_lo : 0) : (uint64_t)a.stride_words);
    RangeEncLane<W, S, kRrEncSlots> L;
    L.init(a.words_out + slab_lo, (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n), ring, lane);
    const int32_t* row = a.symbols_in + sym_lo;
    auto entry = [&](int32_t v) { return table[enc_index(v, a.min_symbol, nsym, L.bad)]; };
    // behind a general step: whole chunks leave the ring until less than half of it is pending (a resolved run of held-back words
    // may have filled it up to four slots below its brim, and the steps that follow push without looking)
    auto relieve = [&]() { while (L.out.wr + L.out.shift - L.out.flushed >= (uint32_t)(kRrEncSlots / 2)) L.out.flush_chunks(); };
    auto quad = [&](const rr_v4i v) {
        const EncEntry e0 = entry(v.x), e1 = entry(v.y), e2 = entry(v.z), e3 = entry(v.w);
        const auto lower0 = L.lower, range0 = L.range;
        const uint32_t wr0 = L.out.wr, inv_n0 = L.inv_n, inv_first0 = L.inv_first;
        bool slow = false;
        L.step_inline(e0.c, e0.p, P, slow); L.step_inline(e1.c, e1.p, P, slow);
        L.step_inline(e2.c, e2.p, P, slow); L.step_inline(e3.c, e3.p, P, slow);
        if (__any(slow)) {           // (nothing of the quad has left the ring: no memory point lies inside it)
            L.lower = lower0; L.range = range0; L.out.wr = wr0; L.inv_n = inv_n0; L.inv_first = inv_first0;
            L.step(e0.c, e0.p, P); relieve(); L.step(e1.c, e1.p, P); relieve();
            L.step(e2.c, e2.p, P); relieve(); L.step(e3.c, e3.p, P); relieve();
        }
    };
    const uint32_t ng = len / G, pre = len & (uint32_t)(G - 1);       // whole groups, then the ragged end of the row
    const uint32_t mxg = rr_wave_max_u32(ng);
    // the (len mod 8) symbols at the end of the row: requested now, coded last (row + 8 ng + j < row + len: inside the row)
    int32_t tail[G - 1];
#pragma unroll
    for (int j = 0; j < G - 1; ++j) tail[j] = (uint32_t)j < pre ? row[(size_t)G * ng + (uint32_t)j] : 0;
    const rr_v4i_unaligned* g4 = reinterpret_cast<const rr_v4i_unaligned*>(row);      // group g = pieces 2 g, 2 g + 1
    rr_v4i nx0 = rr_v4i{0, 0, 0, 0}, nx1 = rr_v4i{0, 0, 0, 0};
    if (ng > 0) { nx0 = g4[0].v; nx1 = g4[1].v; }
    // RangeEncoder::pos() in front of every chunk (JUMP).  A queue codes first to last, so chunk j starts in front of group
    // j * interval / 8 and is known AT that group's memory point: it is stored there, next to the word chunks (one memory point per
    // group).  Between groups no quad is in flight, so a rolled-back quad never sees a jump point; pos counts the held-back words of an
    // Inverted run as cst_range.hip does.  No division in the loop: the lane counts groups down to its next chunk (`to_jump`).
    [[maybe_unused]] uint32_t to_jump = 0;
    [[maybe_unused]] uint64_t next_chunk = 0;
    [[maybe_unused]] bool jumps = false;
    if constexpr (JUMP) {
        jumps = active && len > 0;
        if (jumps) next_chunk = jp.chunk_offsets[s];
    }
    auto store_jump_point = [&]() {
        jp.pos[next_chunk] = L.out.wr + L.inv_n; jp.lower[next_chunk] = (uint64_t)L.lower; jp.range[next_chunk] = (uint64_t)L.range;
        ++next_chunk;
        to_jump = jp.interval / (uint32_t)G;
    };
    for (uint32_t g = 0; g < mxg; ++g) {
        rr_consume(nx0, nx1);                  // group g's symbols (requested a group ago) -- and every older store
        const rr_v4i c0 = nx0, c1 = nx1;
        if (g + 1 < ng) { nx0 = g4[2 * (size_t)(g + 1)].v; nx1 = g4[2 * (size_t)(g + 1) + 1].v; }      // (only a group that exists)
        L.out.flush_chunks();                  // complete 16-byte chunks of the words of earlier groups: ring -> slab (at most 5)
        if constexpr (JUMP) {
            if (jumps && g < ng) {
                if (to_jump == 0) store_jump_point();
                --to_jump;
            }
        }
        if (g < ng) { quad(c0); quad(c1); }
    }
    if constexpr (JUMP) {
        // a chunk that starts exactly at 8 ng, in front of the ragged end of the row (no chunk starts at len itself)
        if (jumps && pre != 0 && to_jump == 0) store_jump_point();
    }
    if (__any(pre != 0)) {
#pragma unroll
        for (int j = 0; j < G - 1; ++j)
            if ((uint32_t)j < pre) {
                const EncEntry e = entry(tail[j]);
                L.step(e.c, e.p, P);
                relieve();
            }
    }
    uint32_t n_words = 0;
    int32_t status = L.finish(nsym, n_words);
    if (too_long) status = CST_STREAM_CAPACITY;
    if (!active) return;
    a.n_words_out[s] = status == CST_STREAM_OK ? n_words : 0u;
    a.status[s] = status;
}

template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_encode_ragged_kernel(const RangeRaggedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rr_encode<W, S, STAGED, false>(a, RangeRaggedJump{}, smem);
}

template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_encode_ragged_jump_kernel(const RangeRaggedArgs a, const RangeRaggedJump jp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rr_encode<W, S, STAGED, true>(a, jp, smem);
}

// what both decoding kernels share: the tables (staged or not), the lane's coder on its slice of the words, its window primed.
// Small rings (32 slots, 24 words ahead): 8 KiB per wave, two workgroups per CU next to 42 KiB of tables.
constexpr int kRrDecSlots = 32, kRrDecAhead = 24;
constexpr size_t kRrDecRingBytes = (size_t)(kBlock / kWave) * kRrDecSlots * kWave * 4;
// a step consumes at most ONE word, and what a memory point requests lands at the next one: the words a group may read (kRrGroup
// consumed by the group before it, kRrGroup by itself) must lie inside what was requested two points ago
static_assert(2 * kRrGroup <= kRrDecAhead - 4, "a group may consume kRrGroup words before the chunks requested at its start land");
static_assert(kRrDecAhead + 4 <= kRrDecSlots, "the window (rounded up to a chunk) must fit the ring");
static_assert(kRrGroup + 3 <= 4 * kMaxChunksPerPoint, "a memory point must be able to request what a group consumed");

template <int W, int S, bool STAGED>
struct RangeRaggedDecoder {
    DecLut lut{};
    const uint32_t* cdf;
    const uint16_t* bucket;
    RangeDecLane<W, S, kRrDecSlots, kRrDecAhead> L;
    WordSlice ws;
    bool active;
    size_t s, slot;
    int lane;

    // every thread of the workgroup: the tables (the only barriers)
    __device__ __forceinline__ void stage(const RangeRaggedArgs& a, unsigned char* smem) {
        cdf = a.cdf; bucket = a.bucket;
        if constexpr (STAGED) {
            stage_decoder_tables<kDecBucket, true, true>(smem + kRrDecRingBytes, a.precision, nullptr, nullptr, a.cdf, a.bucket, a.bucket_bits,
                                                         a.n_symbols, lut, cdf, bucket);
            __syncthreads();
        }
        lane = threadIdx.x & (kWave - 1);
        slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        s = rr_stream(a, slot, active);
    }
    __device__ __forceinline__ bool wave_has_streams(const RangeRaggedArgs& a) const { return slot - lane < a.n_streams; }
    // from_compressed + read_point on the stream's (checked) slice of the words, window primed
    __device__ __forceinline__ void start(const RangeRaggedArgs& a, uint32_t* ring) {
        ws = active ? word_slice(a.word_offsets, a.stride_words, a.n_words_in, s, a.words_capacity) : WordSlice{0, 0u, false};
        L.init(a.words_in + ws.off, ws.n, ring, lane);
        L.in.prime();
        wave_lds_fence();
    }
    // a chunk (the lane's `s` is a chunk index): RangeDecoder::seek to its jump point on its STREAM's slice of the words -- checked as
    // start() checks it --, window primed at the read position.  init_at clamps a `pos` beyond the stream's words to their end.
    __device__ __forceinline__ void start_at(const RangeRaggedArgs& a, const RangeRaggedChunks& v, uint32_t* ring) {
        using st_t = typename StateT<S>::type;
        ws = active ? word_slice(v.word_off, 0, v.n_words, s, a.words_capacity) : WordSlice{0, 0u, false};
        L.init_at(a.words_in + ws.off, ws.n, active ? v.pos[s] : 0u, active ? (st_t)v.lower[s] : (st_t)0, active ? (st_t)v.range[s] : (st_t)0, ring, lane);
        L.in.prime();
        wave_lds_fence();
    }
    // a piece of a query (SELECT: the lane's `s` is a piece index): seek to its table entry -- or to the start of its document, which is
    // jump point (0, 0, all ones) -- on its STREAM's slice of the words, the one the piece builder checked, bounded once more here
    __device__ __forceinline__ void start_piece(const RangeRaggedArgs& a, const RaggedSelectLanes& v, uint32_t* ring) {
        using st_t = typename StateT<S>::type;
        ws = active ? word_slice(v.word_off, 0, v.n_words, s, a.words_capacity) : WordSlice{0, 0u, false};
        const uint32_t e = (active && !ws.bad) ? v.entry[s] : kSelectNoEntry;
        const bool at = e != kSelectNoEntry;
        L.init_at(a.words_in + ws.off, ws.n, at ? v.jump_pos[e] : 0u, at ? (st_t)v.jump_a[e] : (st_t)0, at ? (st_t)v.jump_b[e] : (st_t)~(st_t)0, ring, lane);
        L.in.prime();
        wave_lds_fence();
    }
    __device__ __forceinline__ uint32_t step(const RangeRaggedArgs& a) {
        return L.template step<kDecBucket>(lut, cdf, bucket, a.precision - a.bucket_bits, a.n_symbols, a.precision);
    }
};

// the decoder: MODE kRrPlain is range_decode_ragged_kernel (a lane per stream), kRrJump the form with a lane per chunk of `v`, kRrSelect
// the form with a lane per PIECE of a query (`q`, cst_ragged_select.hpp): a lane decodes `skip` symbols it does not store, then its
// piece's symbols into its own row of the output.  The skipped symbols go through the same groups of eight (advance_window, eight steps: one
// memory point per group), only their stores are left out; a wave runs as long as its longest skip + length.
constexpr int kRrPlain = 0, kRrJump = 1, kRrSelect = 2;
template <int W, int S, bool STAGED, int MODE>
__device__ __forceinline__ void rr_decode(const RangeRaggedArgs& a, const RangeRaggedChunks& v, const RaggedSelectLanes& q, unsigned char* smem) {
    constexpr int G = kRrGroup;
    constexpr bool SELECT = MODE == kRrSelect;
    RangeRaggedDecoder<W, S, STAGED> D;
    D.stage(a, smem);
    if (!D.wave_has_streams(a)) return;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (kRrDecSlots * kWave);
    uint64_t sym_lo = 0, sym_hi = 0;
    [[maybe_unused]] uint32_t skip = 0;
    if constexpr (SELECT) {
        D.start_piece(a, q, ring);
        if (D.active) { sym_lo = q.out_lo[D.s]; skip = q.skip[D.s]; sym_hi = sym_lo + skip + q.len[D.s]; }
    } else if constexpr (MODE == kRrJump) {
        D.start_at(a, v, ring);
        if (D.active) { sym_lo = v.sym_lo[D.s]; sym_hi = sym_lo + v.len[D.s]; }
    } else {
        D.start(a, ring);
        sym_lo = D.active ? a.sym_offsets[D.s] : 0; sym_hi = D.active ? a.sym_offsets[D.s + 1] : 0;
    }
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    // (SELECT: `len` counts the symbols the lane DECODES, the first `skip` of which it does not store: skip + the piece's length, at
    //  most 2^32 - 1 by the piece builder's bound; decoded symbol k >= skip is row[k - skip])
    int32_t* row = a.symbols_out + sym_lo;
    const uint32_t mx = rr_wave_max_u32(len);
    int32_t o[G];
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = 0;
    // symbols k0 - 8 .. k0 - 1 (decoded by the previous group) -> HBM: two 16-byte pieces, or one by one at the end of a row.
    // SELECT: a group wholly in front of `skip` stores nothing; the pieces are 16-byte stores at 4-byte boundaries, so a group wholly
    // behind it keeps them wherever in a group the first stored symbol fell; the group that holds that symbol goes one by one
    auto store_group = [&](uint32_t k0) {
        if (k0 < (uint32_t)G || k0 - G >= len) return;
        const uint32_t b = k0 - G;
        if constexpr (SELECT) {
            if (k0 <= skip) return;
            if (b >= skip && k0 <= len) {
                rr_v4i_unaligned* d = reinterpret_cast<rr_v4i_unaligned*>(row + (b - skip));
                d[0].v = rr_v4i{o[0], o[1], o[2], o[3]};
                d[1].v = rr_v4i{o[4], o[5], o[6], o[7]};
            } else {
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (b + (uint32_t)j >= skip && b + (uint32_t)j < len) row[b + (uint32_t)j - skip] = o[j];
            }
        } else {
            if (k0 <= len) {
                rr_v4i_unaligned* d = reinterpret_cast<rr_v4i_unaligned*>(row + b);
                d[0].v = rr_v4i{o[0], o[1], o[2], o[3]};
                d[1].v = rr_v4i{o[4], o[5], o[6], o[7]};
            } else {
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (b + (uint32_t)j < len) row[b + (uint32_t)j] = o[j];
            }
        }
    };
    for (uint32_t k0 = 0; k0 < mx; k0 += G) {
        D.L.in.advance_window();            // lands the chunks requested a group ago, requests this group's
        store_group(k0);
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (k0 + (uint32_t)j < len) o[j] = a.min_symbol + (int32_t)D.step(a);
    }
    store_group((mx + G - 1) / G * G);
    if (!D.active) return;
    a.status[D.s] = D.ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (too_long ? (int32_t)CST_STREAM_CAPACITY : D.L.status);
}

template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_decode_ragged_kernel(const RangeRaggedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rr_decode<W, S, STAGED, kRrPlain>(a, RangeRaggedChunks{}, RaggedSelectLanes{}, smem);
}

template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_decode_ragged_jump_kernel(const RangeRaggedArgs a, const RangeRaggedChunks v) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rr_decode<W, S, STAGED, kRrJump>(a, v, RaggedSelectLanes{}, smem);
}

template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_decode_ragged_select_kernel(const RangeRaggedArgs a, const RaggedSelectLanes q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rr_decode<W, S, STAGED, kRrSelect>(a, RangeRaggedChunks{}, q, smem);
}

// The reference's index stores no lengths: a document ends where its terminator is decoded, and a queue writes it LAST.  First pass of
// that: every stream is decoded until `eof_index` appears, nothing is stored but the count -- terminator included.  A RangeDecoder that
// has run out of words goes on decoding (it shifts in zeros, queue.rs:1025-1029), so `max_symbols` is the only stop for a stream
// without a terminator: CST_STREAM_CAPACITY (whatever such a stream decoded on its way, InvalidData included, says nothing).
template <int W, int S, bool STAGED>
__global__ __launch_bounds__(kBlock) void range_count_until_kernel(const RangeRaggedArgs a, uint32_t eof_index, uint64_t max_symbols, uint64_t* lengths) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RangeRaggedDecoder<W, S, STAGED> D;
    D.stage(a, smem);
    if (!D.wave_has_streams(a)) return;
    D.start(a, reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (kRrDecSlots * kWave));
    uint64_t n = 0;
    bool done = !D.active || D.ws.bad || max_symbols == 0;
    bool found = false;
    while (__any(!done)) {
        D.L.in.advance_window();
#pragma unroll
        for (int j = 0; j < kRrGroup; ++j) {
            if (!done) {
                const uint32_t idx = D.step(a);
                ++n;
                found = idx == eof_index;
                done = found || n >= max_symbols;
            }
        }
    }
    if (!D.active) return;
    lengths[D.s] = n;
    a.status[D.s] = D.ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (found ? D.L.status : (int32_t)CST_STREAM_CAPACITY);
}

static size_t rr_encode_table_bytes(const cst_model* m) { return (((size_t)m->n_symbols * sizeof(EncEntry)) + 15) & ~(size_t)15; }
static size_t rr_decode_table_bytes(const cst_model* m) {
    const size_t cdf = (((size_t)m->n_symbols + 1) * 4 + 15) & ~(size_t)15;
    return cdf + (bucket16_usable(m->n_symbols, m->precision) ? ((size_t)16 << m->bucket_bits) + kSubAreaBytes
                                                               : ((((size_t)2 << m->bucket_bits) + 15) & ~(size_t)15));
}

// largest dynamic LDS allocation of a workgroup on the current device (cached per process: the library targets one kind of GPU)
static size_t rr_device_lds_limit() {
    static const size_t limit = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
            return (size_t)64 * 1024;
        return (size_t)v;
    }();
    return limit;
}

template <typename K, typename... Extra>
static cst_status rr_launch(K kernel, const RangeRaggedArgs& a, size_t ring_bytes, size_t table_bytes, hipStream_t hs, Extra... extra) {
    const size_t blocks = (a.n_streams + kBlock - 1) / kBlock;
    if (blocks == 0) return CST_OK;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    const size_t lds = ring_bytes + table_bytes;
    if (lds > 64 * 1024)
        CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), lds, hs, a, extra...);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

// (W, S) by the preset, STAGED by the size of the tables: staged if they fit beside the rings in what THIS device gives a workgroup
#define CST_RANGE_RAGGED_DISPATCH(KERNEL, RING_BYTES, TABLE_BYTES, ...)                                                              \
    do {                                                                                                                             \
        const size_t tb_ = (TABLE_BYTES);                                                                                            \
        const bool staged_ = tb_ <= kRrStageLimit && (RING_BYTES) + tb_ <= rr_device_lds_limit();                                    \
        const size_t t_ = staged_ ? tb_ : 0;                                                                                         \
        if (cfg.word_bits != 32)                                                                                                     \
            return staged_ ? rr_launch(KERNEL<16, 32, true>, a, RING_BYTES, t_, hs, ##__VA_ARGS__)                                   \
                           : rr_launch(KERNEL<16, 32, false>, a, RING_BYTES, t_, hs, ##__VA_ARGS__);                                 \
        return staged_ ? rr_launch(KERNEL<32, 64, true>, a, RING_BYTES, t_, hs, ##__VA_ARGS__)                                       \
                       : rr_launch(KERNEL<32, 64, false>, a, RING_BYTES, t_, hs, ##__VA_ARGS__);                                     \
    } while (0)

cst_status range_encode_ragged(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                               size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                               uint32_t* d_n_words, int32_t* d_status, const uint32_t* d_order, hipStream_t hs) {
    RangeRaggedArgs a{};
    a.order = d_order;
    a.symbols_in = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.enc = model->d_enc;
    a.n_symbols = model->n_symbols; a.min_symbol = model->min_symbol; a.precision = model->precision;
    a.words_out = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words_out = d_n_words; a.status = d_status;
    CST_RANGE_RAGGED_DISPATCH(range_encode_ragged_kernel, kRrEncRingBytes, rr_encode_table_bytes(model));
}

static RangeRaggedArgs rr_decode_args(const cst_model* model, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                      size_t words_capacity, const uint32_t* d_n_words, size_t n_streams, int32_t* d_status, const uint32_t* d_order) {
    RangeRaggedArgs a{};
    a.order = d_order;
    a.n_streams = n_streams; a.cdf = model->d_cdf; a.bucket = model->d_bucket;
    a.bucket_bits = model->bucket_bits; a.n_symbols = model->n_symbols; a.min_symbol = model->min_symbol; a.precision = model->precision;
    a.words_in = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words_in = d_n_words; a.status = d_status;
    a.words_capacity = words_capacity;
    return a;
}

cst_status range_decode_ragged(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                               size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                               const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, const uint32_t* d_order, hipStream_t hs) {
    RangeRaggedArgs a = rr_decode_args(model, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, n_streams, d_status, d_order);
    a.symbols_out = d_symbols; a.sym_offsets = d_sym_offsets;
    CST_RANGE_RAGGED_DISPATCH(range_decode_ragged_kernel, kRrDecRingBytes, rr_decode_table_bytes(model));
}

cst_status range_count_until(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                             size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, size_t n_streams, int32_t eof_symbol,
                             size_t max_symbols, uint64_t* d_lengths, int32_t* d_status, const uint32_t* d_order, hipStream_t hs) {
    const RangeRaggedArgs a = rr_decode_args(model, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, n_streams, d_status, d_order);
    const uint32_t eof_index = (uint32_t)eof_symbol - (uint32_t)model->min_symbol;
    const uint64_t mx = (uint64_t)max_symbols;
    CST_RANGE_RAGGED_DISPATCH(range_count_until_kernel, kRrDecRingBytes, rr_decode_table_bytes(model), eof_index, mx, d_lengths);
}
// ---- jump points ----
cst_status range_encode_ragged_jump(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                    size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                    uint32_t* d_n_words, int32_t* d_status, const uint32_t* d_order, uint32_t interval,
                                    const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_lower, uint64_t* d_jump_range,
                                    hipStream_t hs) {
    RangeRaggedArgs a{};
    a.order = d_order;
    a.symbols_in = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.enc = model->d_enc;
    a.n_symbols = model->n_symbols; a.min_symbol = model->min_symbol; a.precision = model->precision;
    a.words_out = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words_out = d_n_words; a.status = d_status;
    const RangeRaggedJump jp{interval, d_chunk_offsets, d_jump_pos, d_jump_lower, d_jump_range};
    CST_RANGE_RAGGED_DISPATCH(range_encode_ragged_jump_kernel, kRrEncRingBytes, rr_encode_table_bytes(model), jp);
}

// The decoder's scratch: what RangeRaggedChunks points to, the stream every chunk belongs to, and one status per chunk.
struct RangeRaggedScratch {
    uint64_t *sym_lo, *word_off;
    uint32_t *len, *n_words, *owner;
    int32_t* status;
    explicit RangeRaggedScratch(void* d_scratch, size_t n) {
        unsigned char* b = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(d_scratch) + 15) & ~(uintptr_t)15);
        sym_lo = reinterpret_cast<uint64_t*>(b); word_off = sym_lo + n;
        len = reinterpret_cast<uint32_t*>(word_off + n); n_words = len + n; owner = n_words + n;
        status = reinterpret_cast<int32_t*>(owner + n);
    }
};
size_t range_ragged_jump_scratch_bytes(size_t n_chunks_total) { return 32 * n_chunks_total + 128; }
constexpr uint32_t kRrNoOwner = 0xffffffffu;

// The chunks of a batch as coders of their own, one thread per table entry: entry c belongs to the stream s with
// chunk_offsets[s] <= c < chunk_offsets[s + 1] (found by bisection: the table is caller data, and whatever it holds, an entry gets a
// symbol range inside ONE stream's symbols or none at all), and decodes symbols [j I, min(j I + I, len)) of it, j = c - chunk_offsets[s].
// Entries that belong to no stream (behind the last chunk: n_chunks_total may be an upper bound) are empty.  The stream's slice of
// the words is checked HERE as the plain decoder checks it (per-slab bound included); a bad one is handed on as the empty slice.
__global__ void rr_chunks_kernel(const uint64_t* __restrict__ sym_offsets, const uint64_t* __restrict__ word_offsets, size_t stride_words,
                                 uint64_t words_capacity, const uint32_t* __restrict__ n_words, const uint64_t* __restrict__ chunk_offsets,
                                 size_t n_streams, size_t n_chunks_total, uint32_t interval, RangeRaggedScratch v) {
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
    v.n_words[c] = ws.n;
    v.owner[c] = mine ? (uint32_t)s : kRrNoOwner;
}

// a stream's status: the worst of its chunks'.  A table that does not describe the stream (chunks != ceil(len / I), entries beyond
// n_chunks_total or given to another stream), a jump point beyond the stream's words, or words that leave the buffer, are caller data
// gone wrong: CST_STREAM_INVALID_DATA.  (A stream too long for one coder: CST_STREAM_CAPACITY, as the plain decoder says.)
__global__ void rr_chunk_status_kernel(RangeRaggedScratch v, const uint64_t* __restrict__ sym_offsets, const uint64_t* __restrict__ word_offsets,
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

static cst_status rr_decode_chunks(const cst_model* model, cst_coder_config cfg, const RangeRaggedArgs& a, const RangeRaggedChunks& v, hipStream_t hs) {
    CST_RANGE_RAGGED_DISPATCH(range_decode_ragged_jump_kernel, kRrDecRingBytes, rr_decode_table_bytes(model), v);
}

cst_status range_decode_ragged_jump(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                    size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                    const uint64_t* d_sym_offsets, size_t n_streams, uint32_t interval, const uint64_t* d_chunk_offsets,
                                    size_t n_chunks_total, const uint32_t* d_jump_pos, const uint64_t* d_jump_lower,
                                    const uint64_t* d_jump_range, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    if (n_streams > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    const RangeRaggedScratch v(d_scratch, n_chunks_total);
    if (n_chunks_total > 0) {
        hipLaunchKernelGGL(rr_chunks_kernel, dim3((unsigned)((n_chunks_total + 255) / 256)), dim3(256), 0, hs, d_sym_offsets, d_word_offsets,
                           stride_words, (uint64_t)words_capacity, d_n_words, d_chunk_offsets, n_streams, n_chunks_total, interval, v);
        CST_HIP_TRY(hipGetLastError());
        // (the slices handed on are absolute offsets that passed the check, or empty: `words_capacity` bounds them once more)
        RangeRaggedArgs a = rr_decode_args(model, d_words, nullptr, 0, words_capacity, nullptr, n_chunks_total, v.status, nullptr);
        a.symbols_out = d_symbols;
        const RangeRaggedChunks ch{v.sym_lo, v.len, v.word_off, v.n_words, d_jump_pos, d_jump_lower, d_jump_range};
        // (one table per stream: the chunk lanes of cst_ragged_ps.hip, each with a copy of its owner's row)
        const cst_status rc = model->per_stream ? range_decode_ragged_ps_chunks(model, cfg, d_words, words_capacity, d_symbols, n_chunks_total, v.sym_lo,
                                                                                v.len, v.word_off, v.n_words, v.owner, d_jump_pos, d_jump_lower,
                                                                                d_jump_range, v.status, hs)
                                                : rr_decode_chunks(model, cfg, a, ch, hs);
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(rr_chunk_status_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, hs, v, d_sym_offsets, d_word_offsets, stride_words,
                       (uint64_t)words_capacity, d_chunk_offsets, d_jump_pos, d_n_words, n_streams, n_chunks_total, interval, d_status);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

// ---- random access: selected documents and ranges (cst_ragged_select.hpp) ----
static cst_status rr_decode_select_lanes(const cst_model* model, cst_coder_config cfg, const RangeRaggedArgs& a, const RaggedSelectLanes& q, hipStream_t hs) {
    CST_RANGE_RAGGED_DISPATCH(range_decode_ragged_select_kernel, kRrDecRingBytes, rr_decode_table_bytes(model), q);
}

cst_status range_decode_ragged_select(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const RaggedSelect& b,
                                      const uint64_t* d_jump_lower, const uint64_t* d_jump_range, int32_t* d_symbols, void* d_scratch,
                                      int32_t* d_status, hipStream_t hs) {
    const RaggedSelectPieces v(d_scratch, b.n_pieces_total);
    return ragged_select_run<false>(b, v, d_status, hs, [&]() {
        // (the slices handed on are absolute offsets that passed the check, or empty: `words_capacity` bounds them once more)
        RangeRaggedArgs a = rr_decode_args(model, d_words, nullptr, 0, b.words_capacity, nullptr, b.n_pieces_total, v.status, nullptr);
        a.symbols_out = d_symbols;
        return rr_decode_select_lanes(model, cfg, a, select_lanes(v, b.jump_pos, d_jump_lower, d_jump_range), hs);
    });
}
#undef CST_RANGE_RAGGED_DISPATCH

} // namespace cst
