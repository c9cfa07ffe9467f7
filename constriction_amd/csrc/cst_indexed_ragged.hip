// cst_indexed_ragged.hip -- indexed table coding (cst_indexed.hip) for streams of DIFFERENT lengths, plain and with jump
// points: stream s codes symbols[off[s] .. off[s + 1]) with tables[indices[same range]], its words go to / come from a
// slab of its own (the convention of every ragged call: cst_persymbol_ragged.hpp).
//   geometry  one lane per stream, lane slot i on stream order[i] (persymbol_ragged_stream); a wave runs as long as its longest lane;
//             workgroups of four waves, the table set's image staged once per workgroup -- the ONLY workgroup barrier
//   fetch     every lane fetches its own row in groups of kIrGroup symbols, requested a whole group ahead of their use: no
//             transposition tiles.  A row starts anywhere: int32 rows at any 4-byte boundary (16-byte accesses at 4-byte alignment),
//             uint8 index rows at any byte (aligned dwords that lie wholly inside the row, shifted into place; the group at either end
//             of a row whose dwords would leave the row goes byte by byte).  Nothing outside a stream's own elements is ever read,
//             except element 0 of the arrays where a lane has nothing to read (a wave with a step to take has an element)
//   encode    per symbol exactly the rectangular kernel's work: pack_position's clamp and the second clamp of `entry`, two row reads,
//             make_entry_f64 + ans_encode_step resp. the range step with its rollback, a memory point every 16 symbols (P <= 12) or 8 (above): the ring
//             bound of cst_indexed.hpp's kIxRingSlots holds as it stands.  JUMP: the lane notes pos() in front of every chunk, as
//             encode_entries_ragged_kernel does (cst_persymbol_categorical_ragged.hip)
//   decode    DirectDecoder with the 16-slot word window and the 16-symbol output tile of decode_gaussian_ragged_kernel, the model
//             search replaced by indexed_lookup.  MODE kRgPlain: a lane per stream; kRgJump: a lane per table entry, between the two
//             kernels of decode_jump_chunks; kRgSelect: a lane per PIECE of a query, between the queries and status
//             kernels of cst_ragged_select.hpp and the per-symbol piece builder
#include "cst_indexed.hpp"
#include "cst_persymbol_ragged_select.hpp"

namespace cst {

constexpr int kIrGroup = 8;                                   // symbols a lane requests together
constexpr size_t kIrEncFixedLds = kIxRingBytes;               // 32 KiB of word rings beside the rows
constexpr int kIrOutSyms = 16, kIrOutStride = 20;             // store_symbol_tile_ragged's tile
constexpr int kIrWindow = 16;                                 // word slots per lane: position p lives in slot p % kIrWindow
constexpr size_t kIrDecWaveBytes = (size_t)kWave * kIrOutStride * 4 + (size_t)kIrWindow * kWave * 4;      // 5 KiB + 4 KiB
constexpr size_t kIrDecFixedLds = (size_t)(kBlock / kWave) * kIrDecWaveBytes;                             // 36 KiB beside the image
static_assert(kIrEncFixedLds <= 69632 && kIrDecFixedLds <= 69632, "every image cst_table_set_create accepts fits beside them");
static_assert(kIxMaxImage + kIrDecFixedLds <= 160 * 1024, "a CU's LDS");

struct IndexedRaggedEncodeArgs {
    const unsigned char* image; uint32_t rows_bytes;
    int32_t pitch, n_symbols, n_tables, min_symbol, precision;
    const int32_t* symbols; const void* indices;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    size_t n_streams;
    const uint32_t* order;           // null, or [n_streams]
    uint32_t* words;
    const uint64_t* word_offsets;    // [n_streams + 1], or null: s * stride_words
    size_t stride_words;
    uint32_t* n_words;
    int32_t* status;
};
// (the table of GaussianRaggedEncodeJumpArgs; chunks are counted in symbols)
struct IndexedRaggedEncodeJumpArgs : IndexedRaggedEncodeArgs {
    uint32_t jump_interval;
    const uint64_t* jump_chunk_offsets;     // [n_streams + 1]
    uint32_t* jump_pos;
    uint64_t* jump_a;                       // ANS: the state; the range coder: lower
    uint64_t* jump_b;                       // the range coder: range
};

// kIrGroup indices of one lane as they come from memory, converted where they are used (a group ahead of that, the loads are in flight)
template <class IDX> struct IxRawGroup;
template <> struct IxRawGroup<int32_t> { uint32_t x[kIrGroup]; };
template <> struct IxRawGroup<uint8_t> { uint32_t w0, w1, w2, mis; };    // the bytes start `mis` bytes into w0

// eight dwords [gb, gb + 8) of a row of `len` at `row` (4-byte aligned, nothing more).  Positions behind the row's end read element 0 of
// the array (`base`): an unconditional load from an address that is always valid
__device__ __forceinline__ void fetch_group_i32(const int32_t* base, const int32_t* row, uint32_t gb, uint32_t len, uint32_t (&r)[kIrGroup]) {
    static_assert(kIrGroup == 8, "two 16-byte pieces");
    if ((uint64_t)gb + kIrGroup <= (uint64_t)len) {
        const v4i lo = reinterpret_cast<const v4i_at4*>(row + gb)->v, hi = reinterpret_cast<const v4i_at4*>(row + gb + 4)->v;
        r[0] = (uint32_t)lo.x; r[1] = (uint32_t)lo.y; r[2] = (uint32_t)lo.z; r[3] = (uint32_t)lo.w;
        r[4] = (uint32_t)hi.x; r[5] = (uint32_t)hi.y; r[6] = (uint32_t)hi.z; r[7] = (uint32_t)hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < kIrGroup; ++j) r[j] = (uint32_t)*((uint64_t)gb + (uint64_t)j < (uint64_t)len ? row + gb + j : base);
    }
}

// eight bytes [gb, gb + 8) of a row of `len` bytes at `row` (any byte address): the two or three aligned dwords that cover them where all
// of these lie inside the row, else the bytes of the row one by one -- no byte outside [row, row + len) is read, but byte 0 of the array
__device__ __forceinline__ void fetch_group_u8(const uint8_t* base, const uint8_t* row, uint32_t gb, uint32_t len, IxRawGroup<uint8_t>& r) {
    static_assert(kIrGroup == 8, "two dwords of bytes");
    const uint8_t* at = row + gb;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3u);
    const uint64_t n_bytes = mis ? 12u : 8u;
    if (gb >= mis && (uint64_t)(gb - mis) + n_bytes <= (uint64_t)len) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(at - mis);
        r.w0 = d[0]; r.w1 = d[1]; r.w2 = d[mis ? 2 : 0]; r.mis = mis;
    } else {
        uint32_t b[kIrGroup];
#pragma unroll
        for (int j = 0; j < kIrGroup; ++j) b[j] = (uint32_t)*((uint64_t)gb + (uint64_t)j < (uint64_t)len ? at + j : base);
        r.w0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        r.w1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        r.w2 = 0; r.mis = 0;
    }
}

template <class IDX>
__device__ __forceinline__ void fetch_group_indices(const IDX* base, const IDX* row, uint32_t gb, uint32_t len, IxRawGroup<IDX>& r) {
    if constexpr (sizeof(IDX) == 4) fetch_group_i32(reinterpret_cast<const int32_t*>(base), reinterpret_cast<const int32_t*>(row), gb, len, r.x);
    else fetch_group_u8(base, row, gb, len, r);
}

// the eight bytes of a uint8 group, in place: (low four, high four)
__device__ __forceinline__ uint2 group_bytes(const IxRawGroup<uint8_t>& r) {
    return uint2{__builtin_amdgcn_alignbyte(r.w1, r.w0, r.mis), __builtin_amdgcn_alignbyte(r.w2, r.w1, r.mis)};
}

// the raw index of position j of a group (int32: as the caller gave it; uint8: 0 .. 255)
template <class IDX>
__device__ __forceinline__ int32_t group_index(const IxRawGroup<IDX>& r, int j) {
    if constexpr (sizeof(IDX) == 4) return (int32_t)r.x[j];
    else {
        const uint2 b = group_bytes(r);
        return (int32_t)(((j < 4 ? b.x : b.y) >> (8 * (j & 3))) & 0xffu);
    }
}

// LDS: [word rings, one per wave][rows of the image]
// One lane per stream.  The wave walks position t of ALL its streams together -- the range coder t = 0 .. mx - 1, ANS t = mx - 1 .. 0, mx
// the wave's longest stream -- and a lane takes a step where t < its own length: t, the countdown to the memory point and the jump
// counters are wave-uniform (encode_entries_ragged_kernel's scheme).  Groups are cut from the WAVE's end, so a lane's first (ANS) or last
// (range) group may hold fewer than kIrGroup of its symbols.
// JUMP: chunk j of a stream is symbols [j I, j I + I): a queue notes pos() BEFORE t = j I is coded, a stack AFTER it (the symbols from j I
// on are then encoded).  Only where t < len: no chunk starts at a stream's end.
template <int KIND, class IDX, bool WIDE, bool JUMP>
__global__ __launch_bounds__(kBlock) void indexed_ragged_encode_kernel(const std::conditional_t<JUMP, IndexedRaggedEncodeJumpArgs, IndexedRaggedEncodeArgs> a) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Lane = std::conditional_t<KIND == kAns, EncLane<32, 64, kIxRingSlots>, RangeEncLane<32, 64, kIxRingSlots>>;
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (kIxRingSlots * kWave);
    const unsigned char* rows = smem + kIrEncFixedLds;
    stage_image(smem + kIrEncFixedLds, a.image, a.rows_bytes);
    __syncthreads();

    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot - lane >= a.n_streams) return;                     // whole wave idle (after the only barrier)
    bool active;
    const size_t s = persymbol_ragged_stream(a.order, slot, a.n_streams, active);
    const uint64_t sym_lo = active ? a.sym_offsets[s] : 0, sym_hi = active ? a.sym_offsets[s + 1] : 0;
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    const uint32_t mx = persymbol_wave_max(len);
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols, K = (uint32_t)a.n_tables, pitch = (uint32_t)a.pitch, pmask = (1u << P) - 1u;
    const int G = P <= 12 ? 16 : 8;                             // a memory point every 16 symbols (at most 7 words), or every 8 (7)
    const IDX* indices = reinterpret_cast<const IDX*>(a.indices);
    const int32_t* srow = a.symbols + (len ? sym_lo : 0);
    const IDX* irow = indices + (len ? sym_lo : 0);

    const uint64_t slab_lo = !active ? 0 : (a.word_offsets ? a.word_offsets[s] : (uint64_t)s * a.stride_words);
    // (offsets that run backwards give the stream a slab of NO words: it reports CST_STREAM_CAPACITY and writes nothing)
    const uint64_t slab_hi = !active ? 0 : (a.word_offsets ? a.word_offsets[s + 1] : 0);
    const uint64_t slab_n = !active ? 0 : (a.word_offsets ? (slab_hi >= slab_lo ? slab_hi - slab_lo : 0) : (uint64_t)a.stride_words);
    Lane L;
    L.init(a.words + slab_lo, (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n), ring, lane);
    int countdown = G;
    // JUMP: position t is symbol `jump_in` of chunk `jump_j` of every stream (wave-uniform counters: no division per symbol)
    uint32_t jump_in = 0, jump_j = 0;
    uint64_t jump_c0 = 0;
    if constexpr (JUMP) {
        if (KIND == kAns && mx > 0) { jump_in = (mx - 1u) % a.jump_interval; jump_j = (mx - 1u) / a.jump_interval; }
        jump_c0 = active ? a.jump_chunk_offsets[s] : 0;
    }

    // (c, p) of a packed position; the ANS coder's entry carries floor(2^64 / p) as well.  Every address is legal whatever was packed
    auto entry = [&](uint32_t packed, bool mine) __attribute__((always_inline)) -> EncEntry {
        const uint32_t i = packed & 0xffffu, k = packed >> 16;
        L.bad = max(L.bad, (mine && (i >= nsym || k >= K)) ? nsym : 0u);
        const uint32_t e = min(k, K - 1u) * pitch + min(i, nsym - 1u);
        const uint32_t c = row_at<WIDE>(rows, e), p = (row_at<WIDE>(rows, e + 1u) - c) & pmask;
        if constexpr (KIND == kAns) return make_entry_f64(c, p);
        else return EncEntry{c, p, 0u, 0u};
    };
    // (always_inline, all of them: a lambda that stays a function takes its EncEntry through scratch memory)
    const auto one = [&](const EncEntry e, uint32_t t) __attribute__((always_inline)) {
        const bool mine = t < len;
        if constexpr (JUMP && KIND == kRange) {
            if (jump_in == 0 && mine) {
                a.jump_pos[jump_c0 + jump_j] = L.out.wr + L.inv_n;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)L.lower;
                a.jump_b[jump_c0 + jump_j] = (uint64_t)L.range;
            }
            if (++jump_in == a.jump_interval) { jump_in = 0; ++jump_j; }
        }
        if constexpr (KIND == kAns) {
            if (mine) L.template step<false>(e, P);
        } else {
            // the branch-free step; a position at which some lane leaves a long Inverted run is repeated with the general one
            // (cst_indexed.hip does this by quads: here a lane may have nothing at a position, so by positions)
            const auto lower0 = L.lower, range0 = L.range;
            const uint32_t wr0 = L.out.wr, inv_n0 = L.inv_n, inv_first0 = L.inv_first;
            bool slow = false;
            if (mine) L.step_inline(e.c, e.p, P, slow);
            if (__any(slow)) {
                if (mine) {
                    L.lower = lower0; L.range = range0; L.out.wr = wr0; L.inv_n = inv_n0; L.inv_first = inv_first0;
                    L.step(e.c, e.p, P);
                }
            }
        }
        if constexpr (JUMP && KIND == kAns) {
            if (jump_in == 0 && mine) {
                a.jump_pos[jump_c0 + jump_j] = L.out.wr;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)L.state;
            }
            // (selects: see encode_entries_ragged_kernel)
            const bool first = jump_in == 0;
            jump_j -= first ? 1u : 0u;
            jump_in = first ? a.jump_interval - 1u : jump_in - 1u;
        }
        if (--countdown == 0) { countdown = G; L.out.flush_chunks(); }
    };
    // a position on its own (what the wave's length leaves over of a group)
    const auto single = [&](uint32_t t) __attribute__((always_inline)) {
        const bool mine = t < len;
        const int32_t sy = *(mine ? srow + t : a.symbols);
        const int32_t ix = (int32_t)*(mine ? irow + t : indices);
        one(entry(pack_position(sy, ix, a.min_symbol, nsym, K), mine), t);
    };

    struct Raw { uint32_t s[kIrGroup]; IxRawGroup<IDX> x; };
    const auto request = [&](Raw& r, uint32_t gb) __attribute__((always_inline)) {
        fetch_group_i32(a.symbols, srow, gb, len, r.s);
        fetch_group_indices<IDX>(indices, irow, gb, len, r.x);
    };
    static_assert(kIrGroup == 8, "code_group names its eight entries");
    // positions [gb, gb + kIrGroup): all entries first (their row reads do not wait for the coder), then the steps in coding order
    const auto code_group = [&](const Raw& r, uint32_t gb) __attribute__((always_inline)) {
        EncEntry e0, e1, e2, e3, e4, e5, e6, e7;
        const auto at = [&](int j) __attribute__((always_inline)) { return entry(pack_position((int32_t)r.s[j], group_index<IDX>(r.x, j), a.min_symbol, nsym, K), (uint64_t)gb + (uint64_t)j < (uint64_t)len); };
        e0 = at(0); e1 = at(1); e2 = at(2); e3 = at(3); e4 = at(4); e5 = at(5); e6 = at(6); e7 = at(7);
        if constexpr (KIND == kAns) {
            one(e7, gb + 7u); one(e6, gb + 6u); one(e5, gb + 5u); one(e4, gb + 4u); one(e3, gb + 3u); one(e2, gb + 2u); one(e1, gb + 1u); one(e0, gb);
        } else {
            one(e0, gb); one(e1, gb + 1u); one(e2, gb + 2u); one(e3, gb + 3u); one(e4, gb + 4u); one(e5, gb + 5u); one(e6, gb + 6u); one(e7, gb + 7u);
        }
    };

    const uint32_t tail = mx % kIrGroup;
    Raw cur, nxt;
    if constexpr (KIND == kAns) {
        uint32_t g = mx - tail;                    // positions [g - kIrGroup, g) are the next group
        if (g > 0) request(nxt, g - kIrGroup);
        for (uint32_t t = mx; t-- > mx - tail;) single(t);
        while (g > 0) {
            cur = nxt;
            g -= kIrGroup;
            if (g > 0) request(nxt, g - kIrGroup);
            code_group(cur, g);
        }
    } else {
        const uint32_t n_grouped = mx - tail;
        uint32_t g = 0;                            // positions [g, g + kIrGroup) are the next group
        if (n_grouped > 0) request(nxt, 0u);
        while (g < n_grouped) {
            cur = nxt;
            g += kIrGroup;
            if (g < n_grouped) request(nxt, g);
            code_group(cur, g - kIrGroup);
        }
        for (uint32_t t = n_grouped; t < mx; ++t) single(t);
    }

    uint32_t n_words = 0;
    int32_t status;
    if constexpr (KIND == kAns) status = L.finish(true, nsym, n_words);
    else status = L.finish(nsym, n_words);                // (no symbols: `range` is still all ones and nothing is sealed)
    if (!active) return;
    if (too_long) status = CST_STREAM_CAPACITY;
    a.status[s] = status;
    a.n_words[s] = status == CST_STREAM_OK ? n_words : 0u;
}

// One struct for both forms of the decoder.  kRgPlain: stream s owns symbols [sym_offsets[s], sym_offsets[s + 1]), lane slot i decodes
// stream order[i].  kRgJump: every "stream" of p is an entry of the jump table with its symbols given outright (sym_lo, len: what
// persymbol_jump_chunks_kernel made of the caller's table) and its coder started from the raw state of the jump point (p.state / p.rstate).
struct IndexedRaggedDecodeArgs {
    PerSymbolDecodeArgs p;           // words / offsets / stride_words / n_words / words_capacity, symbols (flat), min_symbol, status
    const uint64_t* sym_offsets; const uint32_t* order;
    const uint64_t* sym_lo; const uint32_t* len;
    const uint32_t* owner; const int32_t* stream_status;      // kRgJump: the stream of an entry, and what the precheck said of that stream
    const unsigned char* image; uint32_t rows_bytes, image_bytes;
    int32_t pitch, n_tables, bucket_bits, bucket_wide;
    const void* indices;
};

// SELECT form: every "stream" of p is a PIECE of a query (PerSymbolSelectPieces).  sym_lo is then the element of the
// piece's first INDEX -- its jump point's, or its stream's start without a table -- and the row is skip + len long: the dropped symbols
// run through the fetch, the window and the tile as the stored ones do, and symbol t >= skip goes to p.symbols[out_lo + (t - skip)].
// `raw`: the pieces start from the raw state of a jump point (p.state / p.rstate per piece), else from all of their stream's words.
struct IndexedRaggedSelectArgs : IndexedRaggedDecodeArgs {
    const uint64_t* out_lo;          // [n pieces]: first symbol stored, in p.symbols
    const uint32_t* skip;            // [n pieces]: symbols decoded and dropped (skip + len <= 2^32 - 1)
    bool raw;
};
template <int MODE> using IndexedRaggedDecodeArgsOf = std::conditional_t<MODE == kRgSelect, IndexedRaggedSelectArgs, IndexedRaggedDecodeArgs>;

// LDS: [rows and buckets of the image][per wave: the 16-symbol output tile, the word window]
// decode_gaussian_ragged_kernel's loop: tiles of kIrGroup symbols, the words of the tile after next requested while this one is decoded,
// the indices of the next tile likewise (per lane: eight clamped indices packed into two registers, picked by a shift).
template <int KIND, class IDX, bool WIDE, int MODE>
__global__ __launch_bounds__(kBlock) void indexed_ragged_decode_kernel(const IndexedRaggedDecodeArgsOf<MODE> ra) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    static_assert(MODE == kRgPlain || MODE == kRgJump || MODE == kRgSelect, "whole streams, the entries of a jump table, or pieces of queries");
    static_assert(2 * kIrGroup == kIrWindow && kIrGroup == 8, "the window holds this tile's words and the next one's");
    const PerSymbolDecodeArgs& a = ra.p;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned char* rows = smem;
    const unsigned char* buckets = rows + ra.rows_bytes;
    stage_image(smem, ra.image, ra.image_bytes);
    __syncthreads();

    const int lane = threadIdx.x & (kWave - 1);
    unsigned char* mine_lds = smem + ra.image_bytes + (size_t)(threadIdx.x >> 6) * kIrDecWaveBytes;      // (image_bytes: a multiple of 16)
    int32_t* tile = reinterpret_cast<int32_t*>(mine_lds);
    uint32_t* win = reinterpret_cast<uint32_t*>(mine_lds + (size_t)kWave * kIrOutStride * 4);
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot - lane >= a.n_streams) return;                     // whole wave idle (after the only barrier)
    bool active;
    size_t s;
    if constexpr (MODE != kRgPlain) { active = slot < a.n_streams; s = slot; }
    else s = persymbol_ragged_stream(ra.order, slot, a.n_streams, active);
    const size_t se = active ? s : 0;                           // idle lanes look at stream 0's words and decode nothing
    uint64_t sym_lo = 0, sym_hi = 0;
    if (active) {
        if constexpr (MODE == kRgJump) {
            // (a stream whose table does not describe it decodes nothing: its symbols stay as they were)
            const uint32_t owner = ra.owner[s];
            const bool keep = owner != kPjNoOwner && ra.stream_status[owner] == CST_STREAM_OK;
            sym_lo = ra.sym_lo[s]; sym_hi = sym_lo + (keep ? (uint64_t)ra.len[s] : 0);
        }
        // (a piece that belongs to no accepted query is empty: the builder gave it no symbols and no words)
        else if constexpr (MODE == kRgSelect) { sym_lo = ra.sym_lo[s]; sym_hi = sym_lo + (uint64_t)ra.skip[s] + (uint64_t)ra.len[s]; }
        else { sym_lo = ra.sym_offsets[s]; sym_hi = ra.sym_offsets[s + 1]; }
    }
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;      // (never a chunk: at most jump_interval symbols)
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    const uint32_t off_lo = (uint32_t)sym_lo, off_hi = (uint32_t)(sym_lo >> 32);
    // SELECT: where the lane's symbols go, and how many of the decoded ones stay out (`len` is skip + len of the piece)
    uint32_t out_lo = 0, out_hi = 0, skip = 0;
    if constexpr (MODE == kRgSelect) {
        const uint64_t o = active ? ra.out_lo[s] : 0;
        out_lo = (uint32_t)o; out_hi = (uint32_t)(o >> 32); skip = active ? ra.skip[s] : 0u;
    }
    const uint32_t mx = persymbol_wave_max(len);
    const int P = a.precision;
    const uint32_t K = (uint32_t)ra.n_tables, pitch = (uint32_t)ra.pitch, pmask = (1u << P) - 1u;
    const uint32_t bstride = (1u << ra.bucket_bits) + 1u;
    const int shift = P - ra.bucket_bits;
    const bool bucket_wide = ra.bucket_wide != 0;
    const IDX* indices = reinterpret_cast<const IDX*>(ra.indices);
    const IDX* irow = indices + (len ? sym_lo : 0);

    DirectDecoder<32, 64, KIND> D;
    if constexpr (MODE == kRgSelect) D.init(a, se, ra.raw);     // (a call with a table: the piece builder has done the seek)
    else D.init(a, se, MODE == kRgJump);                        // (JUMP: AnsCoder::seek / RangeDecoder::seek have been done for it)

    // ---- word window: as in decode_gaussian_ragged_kernel (a tile of 8 symbols takes at most 8 words; the range coder's first two words
    // are taken by init, before the window starts).  ANS reads downwards from its position: every index from 0 up to it exists.  The
    // range coder reads upwards: an index exists below the stream's length. ----
    constexpr bool kDownward = DirectDecoder<32, 64, KIND>::kDownward;
    uint32_t w_r[kIrGroup];
    int64_t w_first = 0;                                        // index of w_r[0]
    auto win_request = [&](int64_t first) {
        w_first = first;
        if constexpr (kDownward) {
            if (!__any(first < 0)) {                              // every lane's words exist: one pointer, eight offsets
                const uint32_t* pw = D.in + first;
#pragma unroll
                for (int i = 0; i < kIrGroup; ++i) w_r[i] = pw[i];
                return;
            }
#pragma unroll
            for (int i = 0; i < kIrGroup; ++i) {
                const int64_t p = first + i;
                w_r[i] = *(p >= 0 ? D.in + p : D.idle);
            }
        } else {
            const int64_t n = (int64_t)D.length();
            if (!__any(first < 0 || first + kIrGroup > n)) {
                const uint32_t* pw = D.in + first;
#pragma unroll
                for (int i = 0; i < kIrGroup; ++i) w_r[i] = pw[i];
                return;
            }
#pragma unroll
            for (int i = 0; i < kIrGroup; ++i) {
                const int64_t p = first + i;
                w_r[i] = *(p >= 0 && p < n ? D.in + p : D.idle);
            }
        }
    };
    auto win_land = [&]() {
#pragma unroll
        for (int i = 0; i < kIrGroup; ++i) win[(((uint32_t)(w_first + i)) & (kIrWindow - 1)) * kWave + lane] = w_r[i];
    };
    const auto window_of = [&](int ahead_tiles) -> int64_t {    // first index of the 8 words `ahead_tiles` tiles ahead
        if constexpr (kDownward) return (int64_t)D.position() - (int64_t)kIrGroup * (ahead_tiles + 1);
        else return (int64_t)D.position() + (int64_t)kIrGroup * ahead_tiles;
    };

    // ---- indices: the lane's next eight, raw; then as eight bytes clamped to K - 1 with a bit for each that had to be clamped ----
    IxRawGroup<IDX> x_r;
    uint32_t x_lo = 0, x_hi = 0, x_bad = 0;
    auto idx_land = [&](uint32_t t0) {
        if constexpr (sizeof(IDX) == 4) {
            x_lo = 0; x_hi = 0; x_bad = 0;
#pragma unroll
            for (int j = 0; j < kIrGroup; ++j) {
                const uint32_t raw = x_r.x[j];
                x_bad |= (raw >= K ? 1u : 0u) << j;
                const uint32_t k = min(raw, K - 1u) << (8 * (j & 3));
                if (j < 4) x_lo |= k; else x_hi |= k;
            }
        } else {
            const uint2 b = group_bytes(x_r);
            x_lo = b.x; x_hi = b.y; x_bad = 0;                  // (judged byte by byte where they are used: K <= 256)
        }
        (void)t0;
    };
    bool bad_index = false;

    if (mx > 0) {
        fetch_group_indices<IDX>(indices, irow, 0u, len, x_r);
        win_request(window_of(0));
    }
    for (uint32_t t0 = 0; t0 < mx; t0 += kIrGroup) {            // (mx <= 2^32 - 1: t0 + 8 may wrap only behind the last tile)
        wave_lds_fence();                                       // (the previous tile's words have been read)
        win_land();
        idx_land(t0);
        const bool more = mx - t0 > (uint32_t)kIrGroup;
        if (more) fetch_group_indices<IDX>(indices, irow, t0 + kIrGroup, len, x_r);
        win_request(window_of(1));                              // (the words one tile further: used from the next tile on)
        wave_lds_fence();
        const int n_wave = (int)(more ? (uint32_t)kIrGroup : mx - t0);
#pragma unroll 1
        for (int tl = 0; tl < n_wave; ++tl) {
            const uint32_t t = t0 + (uint32_t)tl;
            int32_t sym = 0;
            const uint32_t k_raw = ((tl < 4 ? x_lo : x_hi) >> (8 * (tl & 3))) & 0xffu;
            D.ahead = win[(((uint32_t)D.next_index()) & (kIrWindow - 1)) * kWave + lane];
            if (t < len) {
                bad_index |= k_raw >= K || ((x_bad >> tl) & 1u) != 0;
                const uint32_t k = min(k_raw, K - 1u);
                const uint32_t q = D.quantile(P);               // (below 2^P: every address of the lookup is legal)
                uint32_t idx, c, p;
                indexed_lookup<WIDE>(rows, buckets, bucket_wide, bstride, pitch, k, q, shift, pmask, idx, c, p);
                D.advance(q, c, p, P);
                sym = a.min_symbol + (int32_t)idx;
            }
            // (a lane past its length writes a zero into its own LDS row: never stored)
            tile[lane * kIrOutStride + (int)(t % kIrOutSyms)] = sym;
            if (t % kIrOutSyms == kIrOutSyms - 1) {
                wave_lds_fence();
                if constexpr (MODE == kRgSelect) store_symbol_tile_select(a.symbols, out_lo, out_hi, skip, len, (uint64_t)t - (kIrOutSyms - 1), lane, tile);
                else store_symbol_tile_ragged(a.symbols, off_lo, off_hi, len, (uint64_t)t - (kIrOutSyms - 1), lane, tile);
                wave_lds_fence();
            }
        }
        if (!more) break;
    }
    if (mx % kIrOutSyms != 0) {
        wave_lds_fence();
        if constexpr (MODE == kRgSelect) store_symbol_tile_select(a.symbols, out_lo, out_hi, skip, len, (uint64_t)(mx - mx % kIrOutSyms), lane, tile);
        else store_symbol_tile_ragged(a.symbols, off_lo, off_hi, len, (uint64_t)(mx - mx % kIrOutSyms), lane, tile);
    }
    if (!active) return;
    a.status[s] = too_long ? (int32_t)CST_STREAM_CAPACITY : (bad_index ? (int32_t)CST_STREAM_INVALID_DATA : D.status);
}

// What persymbol_jump_status_kernel will say of every stream as far as the TABLE and the slices go, before a chunk is decoded (one thread
// per stream, into d_status, which the status kernel overwrites at the end): the chunk decoder leaves the symbols of a stream alone whose
// table does not describe it -- they stay as the caller filled them.  The same conditions, in the same order.
__global__ void indexed_jump_precheck_kernel(PerSymbolJumpScratch v, const uint64_t* __restrict__ sym_offsets, const uint64_t* __restrict__ word_offsets,
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
        for (uint64_t c = c0; c < c1; ++c)
            if (v.owner[c] != (uint32_t)s || jump_pos[c] > n_words[s]) worst = CST_STREAM_INVALID_DATA;
    status[s] = worst;
}

// ---- host side ----
static constexpr const char* kIrNames[2][2][2] = {
    {{"ans_encode_indexed_ragged_kernel", "ans_decode_indexed_ragged_kernel"}, {"range_encode_indexed_ragged_kernel", "range_decode_indexed_ragged_kernel"}},
    {{"ans_encode_indexed_ragged_kernel<jump>", "ans_decode_indexed_ragged_kernel<jump>"},
     {"range_encode_indexed_ragged_kernel<jump>", "range_decode_indexed_ragged_kernel<jump>"}}};

// everything that can be said about a call without the device; `tables` is read last, and only once it is known to be a handle
static cst_status check_indexed_ragged_args(const cst_table_set* tables, cst_coder_config cfg, const void* d_symbols, const void* d_indices,
                                            int32_t index_bytes, const void* d_sym_offsets, const void* d_words, const void* d_word_offsets,
                                            size_t stride_words, const void* d_n_words, const void* d_status, size_t n_streams) {
    if (!tables || !d_symbols || !d_indices || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (index_bytes != 1 && index_bytes != 4) return CST_ERR_INVALID_ARGUMENT;
    if (cfg.word_bits != 32 || cfg.state_bits != 64) return CST_ERR_INVALID_ARGUMENT;      // the (32, 64) preset only
    if (!d_word_offsets && stride_words == 0) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams > 0xffffffffull) return CST_ERR_INVALID_ARGUMENT;                        // (an order names 32-bit indices)
    if (!table_set_alive(tables) || cfg.precision != tables->precision) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

static cst_status check_indexed_ragged_device(const cst_table_set* tables, size_t n_lanes) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != tables->device) return CST_ERR_INVALID_ARGUMENT;
    if ((n_lanes + kBlock - 1) / kBlock > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

template <int KIND, bool JUMP>
static cst_status encode_indexed_ragged(cst_coder_config cfg, const cst_table_set* tables, const int32_t* d_symbols, const void* d_indices,
                                        int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                        uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                        size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_a,
                                        uint64_t* d_jump_b, int32_t* d_status, hipStream_t hs) {
    if constexpr (JUMP)
        if (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b)) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_indexed_ragged_args(tables, cfg, d_symbols, d_indices, index_bytes, d_sym_offsets, d_words, d_word_offsets, stride_words,
                                                  d_n_words, d_status, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    if (cst_status st = check_indexed_ragged_device(tables, n_streams)) return st;
    std::conditional_t<JUMP, IndexedRaggedEncodeJumpArgs, IndexedRaggedEncodeArgs> a{};
    a.image = tables->d_image; a.rows_bytes = tables->rows_bytes;
    a.pitch = tables->pitch; a.n_symbols = tables->n_symbols; a.n_tables = tables->n_tables; a.min_symbol = tables->min_symbol;
    a.precision = tables->precision;
    a.symbols = d_symbols; a.indices = d_indices; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.order = d_order;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words = d_n_words; a.status = d_status;
    if constexpr (JUMP) {
        a.jump_interval = (uint32_t)jump_interval; a.jump_chunk_offsets = d_chunk_offsets; a.jump_pos = d_jump_pos; a.jump_a = d_jump_a;
        a.jump_b = d_jump_b;
    }
    const size_t blocks = (n_streams + kBlock - 1) / kBlock, lds = kIrEncFixedLds + tables->rows_bytes;
    cst_status rc;
    if (tables->wide) rc = index_bytes == 1 ? launch_with_lds(indexed_ragged_encode_kernel<KIND, uint8_t, true, JUMP>, blocks, kBlock, lds, a, hs)
                                            : launch_with_lds(indexed_ragged_encode_kernel<KIND, int32_t, true, JUMP>, blocks, kBlock, lds, a, hs);
    else rc = index_bytes == 1 ? launch_with_lds(indexed_ragged_encode_kernel<KIND, uint8_t, false, JUMP>, blocks, kBlock, lds, a, hs)
                               : launch_with_lds(indexed_ragged_encode_kernel<KIND, int32_t, false, JUMP>, blocks, kBlock, lds, a, hs);
    return note_kernel(kIrNames[JUMP][KIND == kRange][0], rc);
}

template <int KIND, int MODE>
static cst_status launch_decode_indexed_ragged(const cst_table_set* tables, IndexedRaggedDecodeArgsOf<MODE> a, int32_t index_bytes, hipStream_t hs) {
    if (cst_status st = check_indexed_ragged_device(tables, a.p.n_streams)) return st;
    a.p.min_symbol = tables->min_symbol; a.p.n_symbols = tables->n_symbols; a.p.precision = tables->precision;
    a.image = tables->d_image; a.rows_bytes = tables->rows_bytes; a.image_bytes = tables->image_bytes;
    a.pitch = tables->pitch; a.n_tables = tables->n_tables; a.bucket_bits = tables->bucket_bits; a.bucket_wide = tables->bucket_wide;
    const size_t blocks = (a.p.n_streams + kBlock - 1) / kBlock, lds = kIrDecFixedLds + tables->image_bytes;
    if (tables->wide) return index_bytes == 1 ? launch_with_lds(indexed_ragged_decode_kernel<KIND, uint8_t, true, MODE>, blocks, kBlock, lds, a, hs)
                                              : launch_with_lds(indexed_ragged_decode_kernel<KIND, int32_t, true, MODE>, blocks, kBlock, lds, a, hs);
    return index_bytes == 1 ? launch_with_lds(indexed_ragged_decode_kernel<KIND, uint8_t, false, MODE>, blocks, kBlock, lds, a, hs)
                            : launch_with_lds(indexed_ragged_decode_kernel<KIND, int32_t, false, MODE>, blocks, kBlock, lds, a, hs);
}

template <int KIND>
static cst_status decode_indexed_ragged(cst_coder_config cfg, const cst_table_set* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                        size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                        int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                        const uint32_t* d_order, int32_t* d_status, hipStream_t hs) {
    if (cst_status st = check_indexed_ragged_args(tables, cfg, d_symbols, d_indices, index_bytes, d_sym_offsets, d_words, d_word_offsets, stride_words,
                                                  d_n_words, d_status, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    IndexedRaggedDecodeArgs a{};
    a.p.words = d_words; a.p.offsets = d_word_offsets; a.p.stride_words = stride_words; a.p.n_words = d_n_words; a.p.words_capacity = words_capacity;
    a.p.symbols = d_symbols; a.p.n_streams = n_streams; a.p.status = d_status;
    a.sym_offsets = d_sym_offsets; a.order = d_order; a.indices = d_indices;
    return note_kernel(kIrNames[0][KIND == kRange][1], launch_decode_indexed_ragged<KIND, kRgPlain>(tables, a, index_bytes, hs));
}

// the indexed chunk decoder between the two table kernels (decode_jump_chunks, cst_persymbol_ragged.hpp)
template <int KIND>
static cst_status decode_indexed_ragged_jump(cst_coder_config cfg, const cst_table_set* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                             size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                             int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                             size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                             const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    cst_status plain = check_indexed_ragged_args(tables, cfg, d_symbols, d_indices, index_bytes, d_sym_offsets, d_words, d_word_offsets, stride_words,
                                                 d_n_words, d_status, n_streams);
    // (the device is asked only about a handle that lives, and only where something will be launched)
    if (plain == CST_OK && n_streams > 0) plain = check_indexed_ragged_device(tables, n_chunks_total);
    const char* name = kIrNames[1][KIND == kRange][1];
    return decode_jump_chunks<KIND>(cfg, plain, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams,
                                    jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_a, d_jump_b, d_scratch, d_status, name, hs,
                                    [&](const PerSymbolDecodeArgs& p, const PerSymbolJumpScratch& v) {
        // (p.words_capacity: the capacity decode_jump_chunks worked out for its two kernels)
        hipLaunchKernelGGL(indexed_jump_precheck_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, hs, v, d_sym_offsets, d_word_offsets,
                           stride_words, p.words_capacity, d_chunk_offsets, d_jump_pos, d_n_words, n_streams, n_chunks_total, (uint32_t)jump_interval,
                           d_status);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_hip_error(e, "indexed_jump_precheck_kernel"); return note_kernel(name, CST_ERR_HIP); }
        IndexedRaggedDecodeArgs a{};
        a.p = p; a.sym_lo = v.sym_lo; a.len = v.len; a.owner = v.owner; a.stream_status = d_status; a.indices = d_indices;
        const cst_status rc = launch_decode_indexed_ragged<KIND, kRgJump>(tables, a, index_bytes, hs);
        return rc == CST_OK ? rc : note_kernel(name, rc);
    });
}

// random access: decode_ragged_select of cst_persymbol_ragged_select.hip with the indexed decoder between the queries
// kernel, the per-symbol piece builder and the status kernel.  No precheck: a query whose stream the table does not describe is
// refused by the queries kernel, gets no piece and writes nothing.
static constexpr const char* kIrSelectNames[2] = {"ans_decode_indexed_ragged_kernel<select>", "range_decode_indexed_ragged_kernel<select>"};

template <int KIND>
static cst_status decode_indexed_ragged_select(cst_coder_config cfg, const cst_table_set* tables, const uint32_t* d_words,
                                               const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                               const void* d_indices, int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams,
                                               size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                               const uint64_t* d_jump_a, const uint64_t* d_jump_b, const uint32_t* d_query_stream,
                                               const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                               const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                               const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    // a table is an interval and ALL its arrays (jump_table_bad: the jump decoders' rule, whole tiles of 16 included), or nothing at all
    const bool table = jump_interval != 0 || d_chunk_offsets || d_jump_pos || d_jump_a || d_jump_b;
    if (table && (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b) || n_chunks_total > 0xffffffffull))
        return CST_ERR_INVALID_ARGUMENT;
    if (n_pieces_total > 0xffffffffull || (d_query_first == nullptr) != (d_query_count == nullptr)) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_indexed_ragged_args(tables, cfg, d_symbols_out, d_indices, index_bytes, d_sym_offsets, d_words, d_word_offsets,
                                                  stride_words, d_n_words, d_status, n_streams)) return st;
    if (n_queries > 0 && (!d_query_stream || !d_piece_offsets || !d_out_offsets || !d_scratch)) return CST_ERR_INVALID_ARGUMENT;
    if (n_queries == 0) return CST_OK;
    if (n_queries > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_indexed_ragged_device(tables, n_pieces_total)) return st;
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
        hipLaunchKernelGGL((persymbol_select_pieces_kernel<32, 64, KIND>), dim3(p_grid), dim3(256), 0, hs, b, d_words, d_jump_a, d_jump_b, d_status, v);
        CST_HIP_TRY(hipGetLastError());
        // (the slices handed on are absolute offsets that passed the check, or empty: the capacity bounds them once more)
        IndexedRaggedSelectArgs a{};
        a.p.words = d_words; a.p.offsets = v.word_off; a.p.stride_words = 0; a.p.n_words = v.n_words; a.p.words_capacity = b.words_capacity;
        a.p.symbols = d_symbols_out; a.p.n_streams = n_pieces_total; a.p.status = v.status; a.p.state = v.state; a.p.rstate = v.rstate;
        a.sym_lo = v.par_lo; a.len = v.len; a.out_lo = v.out_lo; a.skip = v.skip; a.raw = jump_interval != 0; a.indices = d_indices;
        const cst_status rc = launch_decode_indexed_ragged<KIND, kRgSelect>(tables, a, index_bytes, hs);
        if (rc != CST_OK) return note_kernel(kIrSelectNames[KIND == kRange], rc);
    }
    hipLaunchKernelGGL(ragged_select_status_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, v.folded(), d_status);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(kIrSelectNames[KIND == kRange], CST_OK);
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_ans_encode_indexed_ragged(cst_coder_config cfg, const void* tables, const int32_t* d_symbols, const void* d_indices, int32_t index_bytes,
                                         const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, uint32_t* d_words,
                                         const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_indexed_ragged<kAns, false>(cfg, as_table_set(tables), d_symbols, d_indices, index_bytes, d_sym_offsets, n_streams, d_order, d_words,
                                              d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_indexed_ragged(cst_coder_config cfg, const void* tables, const int32_t* d_symbols, const void* d_indices, int32_t index_bytes,
                                           const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, uint32_t* d_words,
                                           const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_indexed_ragged<kRange, false>(cfg, as_table_set(tables), d_symbols, d_indices, index_bytes, d_sym_offsets, n_streams, d_order, d_words,
                                                d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_indexed_ragged(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                         size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                         int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                         const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_indexed_ragged<kAns>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_indices, index_bytes,
                                       d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_indexed_ragged(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                           size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                           int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                           const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_indexed_ragged<kRange>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_indices,
                                         index_bytes, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_ans_encode_indexed_ragged_jump(cst_coder_config cfg, const void* tables, const int32_t* d_symbols, const void* d_indices,
                                              int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                              uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                              size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_state,
                                              int32_t* d_status, void* stream) {
    return encode_indexed_ragged<kAns, true>(cfg, as_table_set(tables), d_symbols, d_indices, index_bytes, d_sym_offsets, n_streams, d_order, d_words,
                                             d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state, nullptr,
                                             d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_indexed_ragged_jump(cst_coder_config cfg, const void* tables, const int32_t* d_symbols, const void* d_indices,
                                                int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                                uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                                size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_lower,
                                                uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return encode_indexed_ragged<kRange, true>(cfg, as_table_set(tables), d_symbols, d_indices, index_bytes, d_sym_offsets, n_streams, d_order, d_words,
                                               d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower,
                                               d_jump_range, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_indexed_ragged_jump(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                              size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                              int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                              size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                              const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_indexed_ragged_jump<kAns>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_indices,
                                            index_bytes, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos,
                                            d_jump_state, nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_indexed_ragged_jump(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                                int32_t index_bytes, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                                size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                void* d_scratch, int32_t* d_status, void* stream) {
    return decode_indexed_ragged_jump<kRange>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_indices,
                                              index_bytes, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos,
                                              d_jump_lower, d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_indexed_ragged_select(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                                int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                                const uint64_t* d_jump_state, const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                                const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets,
                                                size_t n_pieces_total, int32_t* d_symbols_out, const uint64_t* d_out_offsets, void* d_scratch,
                                                int32_t* d_status, void* stream) {
    return decode_indexed_ragged_select<kAns>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_indices,
                                              index_bytes, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos,
                                              d_jump_state, nullptr, d_query_stream, d_query_first, d_query_count, n_queries, d_piece_offsets,
                                              n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_indexed_ragged_select(cst_coder_config cfg, const void* tables, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                  size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                                  int32_t index_bytes, const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                  const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                                  const uint64_t* d_jump_lower, const uint64_t* d_jump_range, const uint32_t* d_query_stream,
                                                  const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                  const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                  const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_indexed_ragged_select<kRange>(cfg, as_table_set(tables), d_words, d_word_offsets, stride_words, words_capacity, d_n_words,
                                                d_indices, index_bytes, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                d_jump_pos, d_jump_lower, d_jump_range, d_query_stream, d_query_first, d_query_count, n_queries,
                                                d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status,
                                                (hipStream_t)stream);
}

} // extern "C"
