// cst_ragged_ps.hip -- streams of DIFFERENT lengths, ONE TABLE PER STREAM: many documents or images of different sizes, each coded
// under its own fitted table (Model.fit_per_stream with sym_offsets), both coders, plain and with jump points.
//
// The last cell of the matrix: the ragged prologue of cst_ans_ragged.hip / cst_range_ragged.hip (read their headers first: a CSR-style
// symbol array, slabs by offsets or by a stride, the schedule `order`, a lane per stream or per chunk, symbols in groups of eight with
// one memory point per group) around the coder step of cst_ans_ps.hip / cst_range_ps.hip (a lane's own 16-bit cdf row, transposed per
// wave in LDS: cst_per_stream_rows.hpp).  A lane's row is no function of its number here -- the stream a schedule gives it, or the
// stream that owns its chunk -- so every lane first writes its row's number into a small LDS array and the rows are staged from that
// (stage_rows_by_index); a lane without a stream holds a row of zeros and codes nothing.
//   * encoders: (c, p) = (row[i], row[i + 1] - row[i]); the ANS encoder also reads floor(2^64 / p) from the model's reciprocal table
//     (shared by all streams, L1 / L2 resident), all eight of a group before the group's first step;
//   * decoders: ps_search (a 64-bucket index of the lane's row where 6 <= P <= 15, a bounded 4-ary search otherwise);
//   * jump points: the encoders note AnsCoder::pos() / RangeEncoder::pos() in front of every chunk on their way (the words are
//     unchanged); the decoders run one lane per table entry, each holding ITS OWN copy of its stream's row.  The ANS chunk decoder finds
//     the stream that owns its entry by a bounded bisection of the chunk offsets (the table is caller data: whatever it holds, an entry
//     gets a symbol range inside ONE stream's symbols or none at all); the range chunk decoder takes the owner rr_chunks_kernel wrote.
// Plain C++ throughout, presets (32,64) and (16,32), P <= 16 (what a 16-bit row holds).  The workgroup shrinks from 256 to 64 lanes
// until rows + rings + (decoders) bucket index fit in the 160 KiB of a CU (rps_pick_block); a support too large for that is refused.
// Every stream's words, count and status are those of the rectangular per-stream call for that stream alone.
#include "cst_range_kernels.hpp"
#include "cst_per_stream_rows.hpp"
#include "cst_ragged_ps.hpp"

namespace cst {

struct RaggedPsArgs {
    const int32_t* symbols_in;
    int32_t* symbols_out;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    size_t n_streams;                // streams of the batch = tables of the model
    size_t n_lanes;                  // lanes with work: n_streams, or the table entries of a jump decoder
    const uint16_t* cdf16;           // [n_streams][L]
    int32_t L;                       // row length (power of two)
    const uint64_t* recip;           // [2^P] (ANS encoder)
    int32_t n_symbols, min_symbol, precision;
    uint32_t* words_out;
    const uint32_t* words_in;
    const uint64_t* word_offsets;    // [n_streams + 1] (encode: slab of stream s = [off[s], off[s + 1])) or null
    size_t stride_words;
    uint32_t* n_words_out;
    const uint32_t* n_words_in;
    int32_t* status;
    uint64_t words_capacity;
    const uint32_t* order;           // null, or [n_streams]: lane slot i codes stream order[i]
    // jump points: chunk j of stream s is entry chunk_offsets[s] + j; (pos, a) = AnsCoder::pos(), (pos, a, b) = (pos, lower, range)
    uint32_t jump_interval;          // 0 = none; a multiple of kRpsGroup
    const uint64_t* chunk_offsets;   // [n_streams + 1]
    uint32_t* jump_pos;              // encoders
    uint64_t *jump_a, *jump_b;
    const uint32_t* in_pos;          // chunk decoders
    const uint64_t *in_a, *in_b;
    // range chunk decoder: what rr_chunks_kernel (cst_range_ragged.hip) made of the table, one entry per chunk
    const uint64_t* chunk_sym_lo;
    const uint32_t* chunk_len;
    const uint64_t* chunk_word_off;
    const uint32_t* chunk_n_words;
    const uint32_t* chunk_owner;     // kPsNoRow: the entry belongs to no stream
};

constexpr int kRpsGroup = 8;                             // symbols per memory point
constexpr int kRpsRangeEncSlots = 32;                    // the range encoder's ring (cst_range_ragged.hip: kRrEncSlots)
constexpr int kRpsDecSlots = 32, kRpsDecAhead = 24;      // the decoders' rings: 8 KiB per wave
static_assert(2 * kRpsGroup <= kRpsDecAhead - 4, "a group may consume kRpsGroup words before the chunks requested at its start land");
static_assert(kRpsDecAhead + 4 <= kRpsDecSlots, "the window (rounded up to a chunk) must fit the ring");
static_assert(kRpsGroup + 3 <= 4 * kMaxChunksPerPoint, "a memory point must be able to request what a group consumed");
static_assert(3 + 2 * kRpsGroup < kRpsRangeEncSlots && kRpsRangeEncSlots / 2 + kRpsGroup < kRpsRangeEncSlots &&
                  kRpsRangeEncSlots / 2 - 1 + kRpsGroup <= 3 + 4 * kMaxChunksPerPoint,
              "the range encoder's ring must hold a group's words, and a memory point must be able to move them out");

// a workgroup's LDS: rows [wave][entry][lane] | rings [wave][slot][lane] | (decoders) bucket index [wave][bucket][lane] | row numbers [lane]
__host__ __device__ inline size_t rps_lds_bytes(size_t threads, size_t L, int ring_slots, bool decoder) {
    return threads * L * 2 + (threads / kWave) * (size_t)ring_slots * kWave * 4 + (decoder ? threads * kPsIdxStride * 2 : 0) + threads * 4;
}
struct RpsLds {
    uint16_t* rows;
    uint32_t* ring;          // this wave's
    uint16_t* bidx;          // this lane's column of its wave's bucket index
    uint32_t* lane_row;
};
template <int SLOTS, bool DECODER>
__device__ __forceinline__ RpsLds rps_lds(unsigned char* smem, int L) {
    const size_t rows_bytes = (size_t)blockDim.x * L * 2;
    const size_t ring_bytes = (size_t)(blockDim.x / kWave) * SLOTS * kWave * 4;
    RpsLds l;
    l.rows = reinterpret_cast<uint16_t*>(smem);
    l.ring = reinterpret_cast<uint32_t*>(smem + rows_bytes) + (threadIdx.x >> 6) * (SLOTS * kWave);
    l.bidx = reinterpret_cast<uint16_t*>(smem + rows_bytes + ring_bytes) + (size_t)(threadIdx.x >> 6) * kPsIdxStride * kWave + (threadIdx.x & 63u);
    l.lane_row = reinterpret_cast<uint32_t*>(smem + rps_lds_bytes(blockDim.x, L, SLOTS, DECODER) - (size_t)blockDim.x * 4);
    return l;
}

// lane slot -> stream: the slot itself, or order[slot] (an entry that is not a stream leaves its lane idle)
__device__ __forceinline__ size_t rps_stream(const RaggedPsArgs& a, size_t slot, bool& active) {
    active = slot < a.n_streams;
    if (!active || !a.order) return slot;
    const size_t s = a.order[slot];
    active = s < a.n_streams;
    return s;
}

// every thread of the workgroup: the lanes' rows into LDS (the only barriers of a kernel)
__device__ __forceinline__ void rps_stage(const RaggedPsArgs& a, const RpsLds& lds, bool active, size_t row, bool pad) {
    lds.lane_row[threadIdx.x] = active ? (uint32_t)row : kPsNoRow;
    __syncthreads();
    stage_rows_by_index(lds.rows, a, lds.lane_row, pad);
    __syncthreads();
}

__device__ __forceinline__ uint32_t rps_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

typedef int32_t rps_v4i __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) rps_v4i_unaligned { rps_v4i v; };      // 16-byte access at a 4-byte boundary

// "the values requested a group ago are needed HERE": the compiler's wait goes in front of this, not behind the new group's requests
__device__ __forceinline__ void rps_consume(rps_v4i& a, rps_v4i& b) {
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
}

// what the lane of an encoder owns: its symbols and its slab (offsets that run backwards give the stream a slab of NO words:
// CST_STREAM_CAPACITY, nothing written)
struct RpsEncStream {
    uint64_t sym_lo, slab_lo;
    uint32_t len, slab_n;
    bool too_long;
};
__device__ __forceinline__ RpsEncStream rps_enc_stream(const RaggedPsArgs& a, size_t s, bool active) {
    RpsEncStream r;
    r.sym_lo = active ? a.sym_offsets[s] : 0;
    const uint64_t sym_hi = active ? a.sym_offsets[s + 1] : 0;
    r.too_long = sym_hi - r.sym_lo > 0xffffffffull || sym_hi < r.sym_lo;
    r.len = r.too_long ? 0u : (uint32_t)(sym_hi - r.sym_lo);
    r.slab_lo = !active ? 0 : (a.word_offsets ? a.word_offsets[s] : (uint64_t)s * a.stride_words);
    const uint64_t slab_hi = !active ? 0 : (a.word_offsets ? a.word_offsets[s + 1] : 0);
    const uint64_t slab_n = !active ? 0 : (a.word_offsets ? (slab_hi >= r.slab_lo ? slab_hi - r.slab_lo : 0) : (uint64_t)a.stride_words);
    r.slab_n = (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n);
    return r;
}

// ---- ANS (a stack: the last symbol first) ----
template <int W, int S, bool JUMP>
__global__ __launch_bounds__(kBlock) void ans_encode_ragged_ps_kernel(const RaggedPsArgs a) {
    constexpr int G = kRpsGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const RpsLds lds = rps_lds<kRingSlots, false>(smem, a.L);
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active;
    const size_t s = rps_stream(a, slot, active);
    rps_stage(a, lds, active, s, false);
    if (slot - lane >= a.n_lanes) return;
    const LaneRow R{lds.rows + (size_t)(threadIdx.x >> 6) * a.L * kWave + lane};
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols;
    const RpsEncStream st = rps_enc_stream(a, s, active);
    const uint32_t len = st.len;
    EncLane<W, S> L;
    L.init(a.words_out + st.slab_lo, st.slab_n, lds.ring, lane);
    const int32_t* row = a.symbols_in + st.sym_lo;
    auto entry = [&](int32_t v) {
        const uint32_t i = enc_index(v, a.min_symbol, nsym, L.bad);
        const uint32_t c = R.at(i);
        const uint32_t p = (R.at(i + 1) - c) & 0xffffu;      // (P = 16: the row stores 2^16 as 0)
        const uint64_t m = a.recip[p];
        return EncEntry{c, p, (uint32_t)m, (uint32_t)(m >> 32)};
    };
    // AnsCoder::pos() once the symbols [start, len) are encoded, whenever a chunk starts at `start` (JUMP).  No division in the loop:
    // the lane counts groups down to its next chunk boundary (`to_jump`) and walks the table backwards (`next_chunk`).  A jump point is
    // NOTED where it occurs and STORED at the next group's memory point, next to the word chunks (as ans_encode_ragged_kernel does).
    [[maybe_unused]] bool jumps = false, jp_pending = false;
    [[maybe_unused]] uint32_t groups_per_chunk = 1, to_jump = 0, jp_pos = 0;
    [[maybe_unused]] uint64_t next_chunk = 0, jp_state = 0, jp_chunk = 0;
    const uint32_t ng = len / G, pre = len & (uint32_t)(G - 1);       // whole groups, coded from the last one down; the ragged end first
    if constexpr (JUMP) {
        jumps = active && len > 0;
        groups_per_chunk = a.jump_interval / (uint32_t)G;
        to_jump = ng % groups_per_chunk;                              // whole groups above the highest chunk boundary at or below 8 ng
        next_chunk = jumps ? a.chunk_offsets[s] + ng / groups_per_chunk : 0;      // the chunk that starts at that boundary
    }
    auto note_here = [&]() {
        jp_pos = L.out.wr; jp_state = (uint64_t)L.state; jp_chunk = next_chunk; jp_pending = true;
        --next_chunk;
    };
    auto store_jump_point = [&]() {
        if constexpr (JUMP) {
            if (jp_pending) { a.jump_pos[jp_chunk] = jp_pos; a.jump_a[jp_chunk] = jp_state; jp_pending = false; }
        }
    };
    if (__any(pre != 0)) {
        int32_t v[G - 1];
#pragma unroll
        for (int j = 0; j < G - 1; ++j) v[j] = (uint32_t)j < pre ? row[len - 1u - (uint32_t)j] : 0;
#pragma unroll
        for (int j = 0; j < G - 1; ++j)
            if ((uint32_t)j < pre) L.template step<false>(entry(v[j]), P);
        if constexpr (JUMP) {
            if (jumps && pre != 0 && to_jump == 0) note_here();       // the ragged top part IS a chunk (8 ng is a multiple of the interval)
        }
    }
    if constexpr (JUMP) {
        if (jumps && to_jump == 0) { to_jump = groups_per_chunk; if (pre == 0) --next_chunk; }      // (no chunk starts at len itself)
    }
    const uint32_t mxg = rps_wave_max_u32(ng);
    const rps_v4i_unaligned* g4 = reinterpret_cast<const rps_v4i_unaligned*>(row);      // group g = pieces 2 g, 2 g + 1
    rps_v4i nx0 = rps_v4i{0, 0, 0, 0}, nx1 = rps_v4i{0, 0, 0, 0};
    if (ng > 0) { nx0 = g4[2 * (size_t)(ng - 1)].v; nx1 = g4[2 * (size_t)(ng - 1) + 1].v; }
    for (uint32_t g = 0; g < mxg; ++g) {
        rps_consume(nx0, nx1);              // group g's symbols (requested a group ago) -- and every older store
        const rps_v4i c0 = nx0, c1 = nx1;
        if (g + 1 < ng) { nx0 = g4[2 * (size_t)(ng - g - 2)].v; nx1 = g4[2 * (size_t)(ng - g - 2) + 1].v; }
        L.flush_chunks();                   // complete 16-byte chunks of the words of earlier groups: ring -> slab (at most 5)
        store_jump_point();                 // (a jump point noted by the previous group)
        if (g < ng) {
            const EncEntry e7 = entry(c1.w), e6 = entry(c1.z), e5 = entry(c1.y), e4 = entry(c1.x);
            const EncEntry e3 = entry(c0.w), e2 = entry(c0.z), e1 = entry(c0.y), e0 = entry(c0.x);
            L.template step<false>(e7, P); L.template step<false>(e6, P); L.template step<false>(e5, P); L.template step<false>(e4, P);
            L.template step<false>(e3, P); L.template step<false>(e2, P); L.template step<false>(e1, P); L.template step<false>(e0, P);
            if constexpr (JUMP) {
                if (jumps && --to_jump == 0) { note_here(); to_jump = groups_per_chunk; }
            }
        }
    }
    store_jump_point();
    uint32_t n_words = 0;
    int32_t status = L.finish(true, nsym, n_words);
    if (st.too_long) status = CST_STREAM_CAPACITY;
    if (!active) return;
    a.n_words_out[s] = status == CST_STREAM_OK ? n_words : 0u;
    a.status[s] = status;
}

// CHUNKS = false: a lane per stream.  CHUNKS = true (reported as ans_decode_ragged_ps_kernel<jump>): a lane per table entry c, which
// decodes symbols [j I, min(j I + I, len)) of the stream s with chunk_offsets[s] <= c < chunk_offsets[s + 1], j = c - chunk_offsets[s],
// from that stream's words in front of its jump point, with the coder state noted there (AnsCoder::seek).
template <int W, int S, bool CHUNKS>
__global__ __launch_bounds__(kBlock) void ans_decode_ragged_ps_kernel(const RaggedPsArgs a) {
    using st_t = typename StateT<S>::type;
    constexpr int G = kRpsGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const RpsLds lds = rps_lds<kRpsDecSlots, true>(smem, a.L);
    const int P = a.precision;
    const bool indexed = ps_indexed(P);
    const uint32_t n = (uint32_t)a.n_symbols;
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active;
    size_t s = 0;
    uint64_t sym_lo = 0, sym_hi = 0;
    if constexpr (CHUNKS) {
        active = false;
        if (slot < a.n_lanes) {
            size_t hi = a.n_streams;           // the last stream with chunk_offsets[s] <= slot (at most 32 rounds)
            while (hi - s > 1) {
                const size_t mid = s + (hi - s) / 2;
                if (a.chunk_offsets[mid] <= slot) s = mid; else hi = mid;
            }
            const uint64_t c0 = a.chunk_offsets[s], c1 = a.chunk_offsets[s + 1];
            const uint64_t lo = a.sym_offsets[s], end = a.sym_offsets[s + 1];
            active = slot >= c0 && slot < c1 && end >= lo && end - lo <= 0xffffffffull && (slot - c0) * a.jump_interval < end - lo;
            if (active) {
                sym_lo = lo + (slot - c0) * a.jump_interval;
                sym_hi = end - sym_lo < a.jump_interval ? end : sym_lo + a.jump_interval;
            }
        }
    } else {
        s = rps_stream(a, slot, active);
        if (active) { sym_lo = a.sym_offsets[s]; sym_hi = a.sym_offsets[s + 1]; }
    }
    rps_stage(a, lds, active, s, indexed);
    if (slot - lane >= a.n_lanes) return;
    const LaneRow R{lds.rows + (size_t)(threadIdx.x >> 6) * a.L * kWave + lane};

    // the lane's coder on its (checked) slice of the words, window primed
    DecLane<W, S, kRpsDecSlots, kRpsDecAhead> L;
    WordSlice ws = active ? word_slice(a.word_offsets, a.stride_words, a.n_words_in, s, a.words_capacity) : WordSlice{0, 0u, false};
    if constexpr (CHUNKS) {
        if (active && !ws.bad) {
            const uint32_t pos = a.in_pos[slot];
            if (pos > ws.n) ws = WordSlice{0, 0u, true};      // a jump point beyond its stream's words: caller data gone wrong
            else ws.n = pos;
        }
    }
    L.init(a.words_in + ws.off, ws.n, lds.ring, lane);
    if constexpr (CHUNKS) L.state = (active && !ws.bad) ? (st_t)a.in_a[slot] : (st_t)0;
    else L.read_initial_state();
    L.in.prime();
    wave_lds_fence();
    if (indexed) ps_build_bucket_index(R, lds.bidx, P, n);

    const uint32_t qmask = (1u << P) - 1u;
    auto decode_one = [&]() -> int32_t {
        const uint32_t q = (uint32_t)L.state & qmask;
        const uint32_t next_word = *L.in.slot(L.in.rd - 1u + L.in.shift);           // ignored if no refill
        const uint32_t i = ps_search(R, lds.bidx, indexed, q, P, n);
        const uint32_t c = R.at(i);
        const uint32_t p = (R.at(i + 1) - c) & 0xffffu;
        const st_t st = (st_t)((st_t)(L.state >> P) * (st_t)p + (st_t)(q - c));      // stack.rs:1086-1088
        const bool refill = st < ((st_t)1 << (S - W)) && L.in.rd > 0;               // stack.rs:1089-1097
        L.state = refill ? (st_t)((st << (W % S)) | (st_t)next_word) : st;
        L.in.rd -= refill ? 1u : 0u;
        return a.min_symbol + (int32_t)i;
    };

    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    int32_t* row = a.symbols_out + sym_lo;
    const uint32_t mx = rps_wave_max_u32(len);
    int32_t o[G];
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = 0;
    // symbols k0 - 8 .. k0 - 1 (decoded by the previous group) -> HBM: two 16-byte pieces, or one by one at the end of a row
    auto store_group = [&](uint32_t k0) {
        if (k0 < (uint32_t)G || k0 - G >= len) return;
        const uint32_t b = k0 - G;
        if (k0 <= len) {
            rps_v4i_unaligned* d = reinterpret_cast<rps_v4i_unaligned*>(row + b);
            d[0].v = rps_v4i{o[0], o[1], o[2], o[3]};
            d[1].v = rps_v4i{o[4], o[5], o[6], o[7]};
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (b + (uint32_t)j < len) row[b + (uint32_t)j] = o[j];
        }
    };
    for (uint32_t k0 = 0; k0 < mx; k0 += G) {
        L.in.advance_window();              // lands the chunks requested a group ago, requests this group's
        store_group(k0);
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (k0 + (uint32_t)j < len) o[j] = decode_one();
    }
    store_group((mx + G - 1) / G * G);
    if constexpr (CHUNKS) {
        // (an entry no stream owns: INVALID_DATA, so that a stream whose chunks the table gives to another one cannot report OK)
        if (slot < a.n_lanes) a.status[slot] = (!active || ws.bad) ? (int32_t)CST_STREAM_INVALID_DATA : L.status;
    } else {
        if (!active) return;
        a.status[s] = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (too_long ? (int32_t)CST_STREAM_CAPACITY : L.status);
    }
}

// ---- the range coder (a queue: the first symbol first) ----
template <int W, int S, bool JUMP>
__global__ __launch_bounds__(kBlock) void range_encode_ragged_ps_kernel(const RaggedPsArgs a) {
    constexpr int G = kRpsGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const RpsLds lds = rps_lds<kRpsRangeEncSlots, false>(smem, a.L);
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active;
    const size_t s = rps_stream(a, slot, active);
    rps_stage(a, lds, active, s, false);
    if (slot - lane >= a.n_lanes) return;
    const LaneRow R{lds.rows + (size_t)(threadIdx.x >> 6) * a.L * kWave + lane};
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols;
    const RpsEncStream st = rps_enc_stream(a, s, active);
    const uint32_t len = st.len;
    RangeEncLane<W, S, kRpsRangeEncSlots> L;
    L.init(a.words_out + st.slab_lo, st.slab_n, lds.ring, lane);
    const int32_t* row = a.symbols_in + st.sym_lo;
    struct CP { uint32_t c, p; };
    auto entry = [&](int32_t v) {
        const uint32_t i = enc_index(v, a.min_symbol, nsym, L.bad);
        const uint32_t c = R.at(i);
        return CP{c, (R.at(i + 1) - c) & 0xffffu};      // (P = 16: the row stores 2^16 as 0)
    };
    // behind a general step: whole chunks leave the ring until less than half of it is pending (a resolved run of held-back words
    // may have filled it up to four slots below its brim, and the steps that follow push without looking)
    auto relieve = [&]() { while (L.out.wr + L.out.shift - L.out.flushed >= (uint32_t)(kRpsRangeEncSlots / 2)) L.out.flush_chunks(); };
    // quads of the branch-free step; a quad in which some lane leaves an Inverted run of two or more held-back words is rolled back and
    // repeated with the general step (nothing of the quad has left the ring: no memory point lies inside it)
    auto quad = [&](const rps_v4i v) {
        const CP e0 = entry(v.x), e1 = entry(v.y), e2 = entry(v.z), e3 = entry(v.w);
        const auto lower0 = L.lower, range0 = L.range;
        const uint32_t wr0 = L.out.wr, inv_n0 = L.inv_n, inv_first0 = L.inv_first;
        bool slow = false;
        L.step_inline(e0.c, e0.p, P, slow); L.step_inline(e1.c, e1.p, P, slow);
        L.step_inline(e2.c, e2.p, P, slow); L.step_inline(e3.c, e3.p, P, slow);
        if (__any(slow)) {
            L.lower = lower0; L.range = range0; L.out.wr = wr0; L.inv_n = inv_n0; L.inv_first = inv_first0;
            L.step(e0.c, e0.p, P); relieve(); L.step(e1.c, e1.p, P); relieve();
            L.step(e2.c, e2.p, P); relieve(); L.step(e3.c, e3.p, P); relieve();
        }
    };
    const uint32_t ng = len / G, pre = len & (uint32_t)(G - 1);       // whole groups, then the ragged end of the row
    const uint32_t mxg = rps_wave_max_u32(ng);
    // the (len mod 8) symbols at the end of the row: requested now, coded last (row + 8 ng + j < row + len: inside the row)
    int32_t tail[G - 1];
#pragma unroll
    for (int j = 0; j < G - 1; ++j) tail[j] = (uint32_t)j < pre ? row[(size_t)G * ng + (uint32_t)j] : 0;
    const rps_v4i_unaligned* g4 = reinterpret_cast<const rps_v4i_unaligned*>(row);      // group g = pieces 2 g, 2 g + 1
    rps_v4i nx0 = rps_v4i{0, 0, 0, 0}, nx1 = rps_v4i{0, 0, 0, 0};
    if (ng > 0) { nx0 = g4[0].v; nx1 = g4[1].v; }
    // RangeEncoder::pos() in front of every chunk (JUMP).  A queue codes first to last, so chunk j starts in front of group j I / 8 and
    // is known AT that group's memory point, where it is stored next to the word chunks.  Between groups no quad is in flight, so a
    // rolled-back quad never sees a jump point; pos counts the held-back words of an Inverted run (range_encode_ragged_jump_kernel).
    [[maybe_unused]] uint32_t to_jump = 0;
    [[maybe_unused]] uint64_t next_chunk = 0;
    [[maybe_unused]] bool jumps = false;
    if constexpr (JUMP) {
        jumps = active && len > 0;
        if (jumps) next_chunk = a.chunk_offsets[s];
    }
    auto store_jump_point = [&]() {
        a.jump_pos[next_chunk] = L.out.wr + L.inv_n; a.jump_a[next_chunk] = (uint64_t)L.lower; a.jump_b[next_chunk] = (uint64_t)L.range;
        ++next_chunk;
        to_jump = a.jump_interval / (uint32_t)G;
    };
    for (uint32_t g = 0; g < mxg; ++g) {
        rps_consume(nx0, nx1);                 // group g's symbols (requested a group ago) -- and every older store
        const rps_v4i c0 = nx0, c1 = nx1;
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
                const CP e = entry(tail[j]);
                L.step(e.c, e.p, P);
                relieve();
            }
    }
    uint32_t n_words = 0;
    int32_t status = L.finish(nsym, n_words);
    if (st.too_long) status = CST_STREAM_CAPACITY;
    if (!active) return;
    a.n_words_out[s] = status == CST_STREAM_OK ? n_words : 0u;
    a.status[s] = status;
}

// MODE kRpsPlain: a lane per stream.  kRpsJump: a lane per chunk as rr_chunks_kernel describes it -- RangeDecoder::seek to its jump point
// on its STREAM's slice of the words (a range chunk reads FORWARD and may read on past its chunk, never past its stream).
constexpr int kRpsPlain = 0, kRpsJump = 1;
template <int W, int S, int MODE>
__global__ __launch_bounds__(kBlock) void range_decode_ragged_ps_kernel(const RaggedPsArgs a) {
    using st_t = typename StateT<S>::type;
    constexpr int G = kRpsGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const RpsLds lds = rps_lds<kRpsDecSlots, true>(smem, a.L);
    const int P = a.precision;
    const bool indexed = ps_indexed(P);
    const uint32_t n = (uint32_t)a.n_symbols;
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active;
    size_t s, table;               // where the lane's status goes (stream or chunk), and its row
    if constexpr (MODE == kRpsJump) {
        s = slot;
        const uint32_t owner = slot < a.n_lanes ? a.chunk_owner[slot] : kPsNoRow;
        active = owner != kPsNoRow && owner < a.n_streams;
        table = owner;
    } else {
        s = rps_stream(a, slot, active);
        table = s;
    }
    rps_stage(a, lds, active, table, indexed);
    if (slot - lane >= a.n_lanes) return;
    const LaneRow R{lds.rows + (size_t)(threadIdx.x >> 6) * a.L * kWave + lane};

    RangeDecLane<W, S, kRpsDecSlots, kRpsDecAhead> L;
    WordSlice ws{0, 0u, false};
    uint64_t sym_lo = 0, sym_hi = 0;
    if constexpr (MODE == kRpsJump) {
        // (the slices handed on are absolute offsets that passed the check, or empty: `words_capacity` bounds them once more)
        if (active) ws = word_slice(a.chunk_word_off, 0, a.chunk_n_words, s, a.words_capacity);
        L.init_at(a.words_in + ws.off, ws.n, active ? a.in_pos[s] : 0u, active ? (st_t)a.in_a[s] : (st_t)0, active ? (st_t)a.in_b[s] : (st_t)0,
                  lds.ring, lane);
        if (active) { sym_lo = a.chunk_sym_lo[s]; sym_hi = sym_lo + a.chunk_len[s]; }
    } else {
        if (active) ws = word_slice(a.word_offsets, a.stride_words, a.n_words_in, s, a.words_capacity);
        L.init(a.words_in + ws.off, ws.n, lds.ring, lane);
        if (active) { sym_lo = a.sym_offsets[s]; sym_hi = a.sym_offsets[s + 1]; }
    }
    L.in.prime();
    wave_lds_fence();
    if (indexed) ps_build_bucket_index(R, lds.bidx, P, n);

    auto decode_one = [&]() -> int32_t {
        const uint32_t q = L.peek_quantile(P);
        const uint32_t next_word = L.in.peek();
        const uint32_t i = ps_search(R, lds.bidx, indexed, q, P, n);
        const uint32_t c = R.at(i);
        const uint32_t p = (R.at(i + 1) - c) & 0xffffu;
        L.in.pos += L.advance(c, p, P, next_word, L.in.pos < L.in.len) ? 1u : 0u;
        return a.min_symbol + (int32_t)i;
    };

    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    int32_t* row = a.symbols_out + sym_lo;
    const uint32_t mx = rps_wave_max_u32(len);
    int32_t o[G];
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = 0;
    // symbols k0 - 8 .. k0 - 1 (decoded by the previous group) -> HBM: two 16-byte pieces, or one by one at the end of a row
    auto store_group = [&](uint32_t k0) {
        if (k0 < (uint32_t)G || k0 - G >= len) return;
        const uint32_t b = k0 - G;
        if (k0 <= len) {
            rps_v4i_unaligned* d = reinterpret_cast<rps_v4i_unaligned*>(row + b);
            d[0].v = rps_v4i{o[0], o[1], o[2], o[3]};
            d[1].v = rps_v4i{o[4], o[5], o[6], o[7]};
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (b + (uint32_t)j < len) row[b + (uint32_t)j] = o[j];
        }
    };
    for (uint32_t k0 = 0; k0 < mx; k0 += G) {
        L.in.advance_window();              // lands the chunks requested a group ago, requests this group's
        store_group(k0);
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (k0 + (uint32_t)j < len) o[j] = decode_one();
    }
    store_group((mx + G - 1) / G * G);
    if constexpr (MODE == kRpsJump) {
        // (every table entry reports: rr_chunk_status_kernel reads the owners itself)
        if (slot < a.n_lanes) a.status[s] = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : L.status;
    } else {
        if (!active) return;
        a.status[s] = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (too_long ? (int32_t)CST_STREAM_CAPACITY : L.status);
    }
}

// ---- host ----
// threads per workgroup such that rows (threads * L * 2 bytes) + rings + (decoders) bucket index + row numbers fit in the 160 KiB of LDS
// of one CU: 256 down to 64, 0 if even one wave's rows do not fit
static int rps_pick_block(int L, int ring_slots, bool decoder, size_t& lds) {
    for (int threads = kBlock; threads >= kWave; threads -= kWave) {
        lds = rps_lds_bytes((size_t)threads, (size_t)L, ring_slots, decoder);
        if (lds <= 160 * 1024) return threads;
    }
    return 0;
}

template <typename K>
static cst_status rps_launch(K kernel, const RaggedPsArgs& a, int ring_slots, bool decoder, hipStream_t hs) {
    if (a.n_lanes == 0) return CST_OK;
    size_t lds = 0;
    const int threads = rps_pick_block(a.L, ring_slots, decoder, lds);
    if (threads == 0) return CST_ERR_INVALID_ARGUMENT;   // support too large for LDS-resident per-stream tables
    const size_t blocks = (a.n_lanes + threads - 1) / threads;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (lds > 64 * 1024)
        CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, hs, a);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

static RaggedPsArgs rps_args(const cst_model* model, const uint64_t* d_sym_offsets, size_t n_streams, const uint64_t* d_word_offsets,
                             size_t stride_words, int32_t* d_status, const uint32_t* d_order) {
    RaggedPsArgs a{};
    a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.n_lanes = n_streams;
    a.cdf16 = model->d_cdf16; a.L = model->cdf16_stride; a.recip = model->d_recip;
    a.n_symbols = model->n_symbols; a.min_symbol = model->min_symbol; a.precision = model->precision;
    a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.status = d_status; a.order = d_order;
    return a;
}

cst_status ans_encode_ragged_ps(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                int32_t* d_status, const uint32_t* d_order, uint32_t interval, const uint64_t* d_chunk_offsets,
                                uint32_t* d_jump_pos, uint64_t* d_jump_state, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, n_streams, true)) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, d_sym_offsets, n_streams, d_word_offsets, stride_words, d_status, d_order);
    a.symbols_in = d_symbols; a.words_out = d_words; a.n_words_out = d_n_words;
    if (interval != 0) {
        if (interval % kRpsGroup != 0) return CST_ERR_INVALID_ARGUMENT;
        a.jump_interval = interval; a.chunk_offsets = d_chunk_offsets; a.jump_pos = d_jump_pos; a.jump_a = d_jump_state;
        if (cfg.word_bits == 32) return rps_launch(ans_encode_ragged_ps_kernel<32, 64, true>, a, kRingSlots, false, hs);
        return rps_launch(ans_encode_ragged_ps_kernel<16, 32, true>, a, kRingSlots, false, hs);
    }
    if (cfg.word_bits == 32) return rps_launch(ans_encode_ragged_ps_kernel<32, 64, false>, a, kRingSlots, false, hs);
    return rps_launch(ans_encode_ragged_ps_kernel<16, 32, false>, a, kRingSlots, false, hs);
}

cst_status ans_decode_ragged_ps(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, const uint32_t* d_order, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, n_streams, false)) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, d_sym_offsets, n_streams, d_word_offsets, stride_words, d_status, d_order);
    a.symbols_out = d_symbols; a.words_in = d_words; a.n_words_in = d_n_words; a.words_capacity = words_capacity;
    if (cfg.word_bits == 32) return rps_launch(ans_decode_ragged_ps_kernel<32, 64, false>, a, kRpsDecSlots, true, hs);
    return rps_launch(ans_decode_ragged_ps_kernel<16, 32, false>, a, kRpsDecSlots, true, hs);
}

cst_status ans_decode_ragged_ps_chunks(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                       size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                       const uint64_t* d_sym_offsets, size_t n_streams, uint32_t interval, const uint64_t* d_chunk_offsets,
                                       size_t n_chunks_total, const uint32_t* d_jump_pos, const uint64_t* d_jump_state,
                                       int32_t* d_chunk_status, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, n_streams, false) || interval == 0) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, d_sym_offsets, n_streams, d_word_offsets, stride_words, d_chunk_status, nullptr);
    a.n_lanes = n_chunks_total;
    a.symbols_out = d_symbols; a.words_in = d_words; a.n_words_in = d_n_words; a.words_capacity = words_capacity;
    a.jump_interval = interval; a.chunk_offsets = d_chunk_offsets; a.in_pos = d_jump_pos; a.in_a = d_jump_state;
    if (cfg.word_bits == 32) return rps_launch(ans_decode_ragged_ps_kernel<32, 64, true>, a, kRpsDecSlots, true, hs);
    return rps_launch(ans_decode_ragged_ps_kernel<16, 32, true>, a, kRpsDecSlots, true, hs);
}

cst_status range_encode_ragged_ps(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                  size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                  int32_t* d_status, const uint32_t* d_order, uint32_t interval, const uint64_t* d_chunk_offsets,
                                  uint32_t* d_jump_pos, uint64_t* d_jump_lower, uint64_t* d_jump_range, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, n_streams, false)) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, d_sym_offsets, n_streams, d_word_offsets, stride_words, d_status, d_order);
    a.symbols_in = d_symbols; a.words_out = d_words; a.n_words_out = d_n_words;
    if (interval != 0) {
        if (interval % kRpsGroup != 0) return CST_ERR_INVALID_ARGUMENT;
        a.jump_interval = interval; a.chunk_offsets = d_chunk_offsets; a.jump_pos = d_jump_pos; a.jump_a = d_jump_lower; a.jump_b = d_jump_range;
        if (cfg.word_bits == 32) return rps_launch(range_encode_ragged_ps_kernel<32, 64, true>, a, kRpsRangeEncSlots, false, hs);
        return rps_launch(range_encode_ragged_ps_kernel<16, 32, true>, a, kRpsRangeEncSlots, false, hs);
    }
    if (cfg.word_bits == 32) return rps_launch(range_encode_ragged_ps_kernel<32, 64, false>, a, kRpsRangeEncSlots, false, hs);
    return rps_launch(range_encode_ragged_ps_kernel<16, 32, false>, a, kRpsRangeEncSlots, false, hs);
}

cst_status range_decode_ragged_ps(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                  size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols,
                                  const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, const uint32_t* d_order, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, n_streams, false)) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, d_sym_offsets, n_streams, d_word_offsets, stride_words, d_status, d_order);
    a.symbols_out = d_symbols; a.words_in = d_words; a.n_words_in = d_n_words; a.words_capacity = words_capacity;
    if (cfg.word_bits == 32) return rps_launch(range_decode_ragged_ps_kernel<32, 64, kRpsPlain>, a, kRpsDecSlots, true, hs);
    return rps_launch(range_decode_ragged_ps_kernel<16, 32, kRpsPlain>, a, kRpsDecSlots, true, hs);
}

cst_status range_decode_ragged_ps_chunks(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, size_t words_capacity,
                                         int32_t* d_symbols, size_t n_chunks_total, const uint64_t* d_chunk_sym_lo, const uint32_t* d_chunk_len,
                                         const uint64_t* d_chunk_word_off, const uint32_t* d_chunk_n_words, const uint32_t* d_chunk_owner,
                                         const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                         int32_t* d_chunk_status, hipStream_t hs) {
    if (!ragged_ps_model_ok(model, cfg, model->n_tables, false)) return CST_ERR_INVALID_ARGUMENT;
    RaggedPsArgs a = rps_args(model, nullptr, model->n_tables, nullptr, 0, d_chunk_status, nullptr);
    a.n_lanes = n_chunks_total;
    a.symbols_out = d_symbols; a.words_in = d_words; a.words_capacity = words_capacity;
    a.in_pos = d_jump_pos; a.in_a = d_jump_lower; a.in_b = d_jump_range;
    a.chunk_sym_lo = d_chunk_sym_lo; a.chunk_len = d_chunk_len; a.chunk_word_off = d_chunk_word_off; a.chunk_n_words = d_chunk_n_words;
    a.chunk_owner = d_chunk_owner;
    return cfg.word_bits == 32 ? rps_launch(range_decode_ragged_ps_kernel<32, 64, kRpsJump>, a, kRpsDecSlots, true, hs)
                               : rps_launch(range_decode_ragged_ps_kernel<16, 32, kRpsJump>, a, kRpsDecSlots, true, hs);
}

} // namespace cst
