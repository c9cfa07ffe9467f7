// cst_persymbol_ragged.hpp -- the kernels of the per-symbol coders for streams of DIFFERENT lengths, shared by the two files that
// instantiate them: cst_persymbol_ragged.hip (the plain forms), cst_persymbol_ragged_jump.hip (the JUMP forms) and
// cst_persymbol_ragged_select.hip (the decoder's SELECT form).  Every
// instantiation of these still lives in ONE file (cst_persymbol.hpp): the template parameter decides which.  At the end: the
// model-independent kernels around a jump table and the host routine that launches them around a caller's chunk decoder
// (decode_jump_chunks), for cst_persymbol_categorical_ragged.hip too.
#pragma once
#include "cst_persymbol.hpp"

namespace cst {

// ------------------------------------------------------------------------------------------------
// per-symbol models for streams of DIFFERENT lengths (cst_ans_{encode,decode}_gaussian_ragged): the fused encoder and the
// lane-per-stream decoder above with CSR-style indexing -- stream s owns elements [sym_offsets[s], sym_offsets[s + 1]) of the flat
// symbols / means / stds, and its words go to / come from a slab of its own (cst_ans_ragged.hip's convention, word_slice's
// bounds check).  Lane slot i codes stream order[i] (null: i).  A wave runs as many tiles as its longest stream has; the lanes of
// shorter streams sit the others out.  One route for every batch size: few streams leave most of the chip idle (the
// rectangular calls have their two-pass and by-rows forms for that; here it is a matter of speed, never of correctness).
// Every stream's words, count and status are those of the rectangular kernels for that stream alone: the entries, the coder
// steps and the bracket search are the same code.
// ------------------------------------------------------------------------------------------------

// lane slot -> stream: the slot itself, or order[slot] (an entry that is not a stream leaves its lane idle)
__device__ __forceinline__ size_t persymbol_ragged_stream(const uint32_t* order, size_t slot, size_t n_streams, bool& active) {
    active = slot < n_streams;
    if (!active || !order) return slot;
    const size_t s = order[slot];
    active = s < n_streams;
    return s;
}

__device__ __forceinline__ uint32_t persymbol_wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

struct GaussianRaggedEncodeArgs {
    const int32_t* symbols;
    const void* means;               // PT arrays, PT the kernel's parameter type (cst_persymbol.hpp)
    const void* stds;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    size_t n_streams;
    const uint32_t* order;           // null, or [n_streams]
    int32_t precision, lo, hi;
    uint32_t* words;
    const uint64_t* word_offsets;    // [n_streams + 1]: slab of stream s = [off[s], off[s + 1]), or null: s * stride_words
    size_t stride_words;
    uint32_t* n_words;
    int32_t* status;
};

// LDS per wave on top of the fused kernel's ring and entry tile: (element offset, length) of the wave's kFuStreams streams,
// staged once -- the sixteen lanes that build stream j's entries read j's pair from here, not from HBM per item
// Jump points (the reference's Pos / Seek): the coder's pos() in front of every chunk of `jump_interval` symbols of every stream -- chunk j
// of stream s is entry jump_chunk_offsets[s] + j of the table arrays (cst_ans_encode_ragged_jump's layout), noted by the stream's lane in
// phase B.  The words are untouched.  Arguments of the JUMP form of the kernel only: the plain form's are the struct above.
struct GaussianRaggedEncodeJumpArgs : GaussianRaggedEncodeArgs {
    uint32_t jump_tiles;                    // tiles per chunk: jump_interval / kFuTile >= 1
    const uint64_t* jump_chunk_offsets;     // [n_streams + 1]
    uint32_t* jump_pos;
    uint64_t* jump_a;                       // ANS: the state; the range coder: lower
    uint64_t* jump_b;                       // the range coder: range
};

constexpr size_t kRgMetaBytes = (size_t)kFuStreams * sizeof(uint4);
constexpr size_t kRgEncWaveBytes = kFuWaveBytes + kRgMetaBytes;

// encode_gaussian_fused_kernel<W, S, KIND> in its general form (per-item index and ok_q; walking by adding and PAIR need whole
// tiles of one matrix).  Tile k of stream j covers symbols [16 k, 16 k + 16) of its row; the wave codes max_j ceil(len_j / 16)
// tiles, last to first (ANS, a stack) or first to last (the range coder, a queue); whole-tile or symbol-by-symbol steps are
// each lane's own decision.
// JUMP: a chunk is a whole number of tiles, so the tile with t0 = j * interval is the first (the range coder) or the last coded (ANS) of
// chunk j, whichever path through phase B codes it: a stack notes AFTER that tile (AnsCoder::pos() once the symbols from t0 on are
// encoded), a queue BEFORE it (RangeEncoder::pos()), as encode_gaussian_fused_kernel notes its checkpoints.  Only where t0 < len: no
// chunk starts at the end of a stream.
template <int W, int S, int KIND, class FAM = GaussianFamily, bool JUMP = false, class PT = double>
__global__ __launch_bounds__(kFuBlock) void encode_gaussian_ragged_kernel(const std::conditional_t<JUMP, GaussianRaggedEncodeJumpArgs, GaussianRaggedEncodeArgs> a) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    constexpr size_t kTabBytes = FAM::kErfTab ? kFuTabBytes : 0;
    constexpr int kWaves = kFuBlock / kWave;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1), wave_in_block = threadIdx.x >> 6;
    // LDS: [word rings, one per wave, aligned to their size][erf tables][entry tiles, one per wave][stream offsets and lengths, per wave]
    constexpr size_t kRingBytes = (size_t)kFuRingSlots * kWave * 4, kTileBytes = kFuWaveBytes - kRingBytes;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem + (size_t)wave_in_block * kRingBytes);
    double2* erf_tab = reinterpret_cast<double2*>(smem + kWaves * kRingBytes);
    EncEntry* tile = reinterpret_cast<EncEntry*>(smem + kWaves * kRingBytes + kTabBytes + (size_t)wave_in_block * kTileBytes);
    uint4* meta = reinterpret_cast<uint4*>(smem + kWaves * kRingBytes + kTabBytes + kWaves * kTileBytes + (size_t)wave_in_block * kRgMetaBytes);
    if ((lds_addr(ring) & (uint32_t)(kRingBytes - 1)) != 0) __builtin_trap();
    if constexpr (FAM::kErfTab) {
        erf_tab_fill(erf_tab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const size_t slot0 = ((size_t)blockIdx.x * kWaves + wave_in_block) * kFuStreams;
    if (slot0 >= a.n_streams) return;
    const int P = a.precision;
    const bool use_inv = KIND == kAns && W == 32 && S == 64 && P >= kInvMinPrecision;      // entries with 1 / p (make_entry_inv)
    bool active = false;
    size_t s = 0;
    if (lane < kFuStreams) s = persymbol_ragged_stream(a.order, slot0 + (size_t)lane, a.n_streams, active);   // this lane codes a stream in phase B
    const uint64_t sym_lo = active ? a.sym_offsets[s] : 0, sym_hi = active ? a.sym_offsets[s + 1] : 0;
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    if (lane < kFuStreams) meta[lane] = uint4{(uint32_t)sym_lo, (uint32_t)(sym_lo >> 32), len, 0u};
    const uint32_t n_tiles = persymbol_wave_max((len >> 4) + ((len & (uint32_t)(kFuTile - 1)) != 0 ? 1u : 0u));
    static_assert(kFuTile == 16, "tile counts above shift by four");
    wave_lds_fence();

    // phase A's work items: item w = it * 64 + lane of a tile is (stream j = w / 16, symbol tl = w % 16): sixteen consecutive
    // lanes on consecutive elements of one stream's row.  Requested kFuAhead items ahead of their use, as in the fused kernel.
    int32_t sy_q[kFuAhead];
    PT mu_q[kFuAhead], sd_q[kFuAhead];              // (widened where an item takes them up)
    bool ok_q[kFuAhead];
    const PT* const means = params_as<PT>(a.means);
    const PT* const stds = params_as<PT>(a.stds);
    const int item_t = lane & (kFuTile - 1), item_j0 = lane >> 4;
    auto request = [&](int slot, uint32_t k, int it) {
        const uint4 m = meta[it * (kWave / kFuTile) + item_j0];
        const uint64_t t = (uint64_t)k * kFuTile + (uint64_t)item_t;
        ok_q[slot] = t < (uint64_t)m.z;
        // (unconditional loads from an address that is always valid -- a wave with a tile to code has a symbol, so element 0
        //  exists: a conditional load is waited for at once)
        const uint64_t e = ok_q[slot] ? ((((uint64_t)m.y) << 32) | (uint64_t)m.x) + t : 0;
        sy_q[slot] = __builtin_nontemporal_load(a.symbols + e);
        mu_q[slot] = __builtin_nontemporal_load(means + e);
        sd_q[slot] = __builtin_nontemporal_load(stds + e);
    };

    const uint64_t slab_lo = !active ? 0 : (a.word_offsets ? a.word_offsets[s] : (uint64_t)s * a.stride_words);
    // (offsets that run backwards give the stream a slab of NO words: it reports CST_STREAM_CAPACITY and writes nothing)
    const uint64_t slab_hi = !active ? 0 : (a.word_offsets ? a.word_offsets[s + 1] : 0);
    const uint64_t slab_n = !active ? 0 : (a.word_offsets ? (slab_hi >= slab_lo ? slab_hi - slab_lo : 0) : (uint64_t)a.stride_words);
    EncLane<W, S, kFuRingSlots> LA;
    RangeEncLane<W, S, kFuRingSlots> LR;
    if constexpr (KIND == kAns) LA.init(a.words + slab_lo, (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n), ring, lane);
    else LR.init(a.words + slab_lo, (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n), ring, lane);
    uint32_t bad = 0;
    // JUMP: tile k is tile `jump_in` of chunk `jump_j` of every stream (wave-uniform counters: no division per tile)
    uint32_t jump_in = 0, jump_j = 0;
    uint64_t jump_c0 = 0;
    if constexpr (JUMP) {
        if (KIND == kAns && n_tiles > 0) { jump_in = (n_tiles - 1u) % a.jump_tiles; jump_j = (n_tiles - 1u) / a.jump_tiles; }
        jump_c0 = active ? a.jump_chunk_offsets[s] : 0;
    }

    if (n_tiles > 0) {
#pragma unroll
        for (int q = 0; q < kFuAhead; ++q) request(q, KIND == kAns ? n_tiles - 1u : 0u, q);
    }
    for (uint32_t step = 0; step < n_tiles; ++step) {
        const uint32_t k = KIND == kAns ? n_tiles - 1u - step : step;      // ANS codes last to first, the range coder first to last
        wave_lds_fence();                                      // (the previous tile has been read)
        // ---- phase A: entries of tile k ----
#pragma unroll 1
        for (int it0 = 0; it0 < kFuIters; it0 += kFuAhead) {
#pragma unroll
            for (int q = 0; q < kFuAhead; ++q) {
                const int it = it0 + q;
                const int32_t sy = ok_q[q] ? sy_q[q] : a.lo;       // (items past their stream's end: never coded)
                const double m = ok_q[q] ? (double)mu_q[q] : 0.0, sg = ok_q[q] ? (double)sd_q[q] : 1.0;
                if (it + kFuAhead < kFuIters) request(q, k, it + kFuAhead);
                else if (step + 1 < n_tiles) request(q, KIND == kAns ? k - 1u : k + 1u, it + kFuAhead - kFuIters);
                uint32_t c = 0, p = 0;
                // invalid parameters, out-of-support symbols and degenerate distributions all end up with p = 0 = impossible
                // (see the fused kernel); no branches: invalid parameters are evaluated as (0, 1) and thrown away
                const bool valid = FAM::valid(m, sg);
                const bool inside = FAM::lcp(sy, a.lo, a.hi, P, valid ? m : 0.0, valid ? sg : 1.0, c, p, erf_tab);
                if (!valid || !inside || (uint64_t)c + p > ((uint64_t)1 << P)) p = 0;
                EncEntry entry{c, p, 0u, 0u};                                   // (the range coder divides by nothing)
                if constexpr (KIND == kAns) entry = use_inv ? make_entry_inv(c, p) : make_entry_f64(c, p);
                tile[item_t * kFuRowStride + it * (kWave / kFuTile) + item_j0] = entry;
            }
        }
        wave_lds_fence();
        // ---- phase B: every stream's lane over what its row has of this tile ----
        const uint64_t t0 = (uint64_t)k * kFuTile;
        const int n_here = !active || t0 >= (uint64_t)len ? 0 : ((uint64_t)len - t0 < (uint64_t)kFuTile ? (int)((uint64_t)len - t0) : kFuTile);
        if constexpr (JUMP && KIND == kRange) {
            if (jump_in == 0 && n_here > 0) {
                a.jump_pos[jump_c0 + jump_j] = LR.out.wr + LR.inv_n;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)LR.lower;
                a.jump_b[jump_c0 + jump_j] = (uint64_t)LR.range;
            }
            if (++jump_in == a.jump_tiles) { jump_in = 0; ++jump_j; }
        }
        if constexpr (KIND == kAns) {
            constexpr bool FAST = W == 32 && S == 64;               // the 32-bit-halves step (8 <= P)
            if (FAST && P >= 8 && n_here == kFuTile) {
                // a whole tile: all sixteen entries first (one LDS wait), then sixteen hand-scheduled steps.  An impossible symbol
                // is coded as (0, 1) -- its stream is flagged and its words are never used.
                EncEntry e[kFuTile];
#pragma unroll
                for (int tl = 0; tl < kFuTile; ++tl) e[tl] = tile[tl * kFuRowStride + lane];
#pragma unroll
                for (int tl = kFuTile - 1; tl >= 0; --tl) {
                    const bool none = e[tl].p == 0;
                    bad |= none ? 1u : 0u;
                    if constexpr (FAST) {
                        if (use_inv) encode_step_inv(LA, none ? 0u : e[tl].c, none ? 1u : e[tl].p, none ? 1.0 : f64_from(e[tl].m_lo, e[tl].m_hi), P);
                        else LA.template step<FAST>(EncEntry{none ? 0u : e[tl].c, none ? 1u : e[tl].p, none ? 0xffffffffu : e[tl].m_lo, none ? 0xffffffffu : e[tl].m_hi}, P);
                    }
                }
            } else {
                // (other presets, P < 8, the end of a row; n_here = 0: this lane's stream has nothing in the tile)
                for (int tl = n_here - 1; tl >= 0; --tl) {
                    const EncEntry e = tile[tl * kFuRowStride + lane];
                    if (e.p == 0) bad = 1;
                    else if (!bad) LA.template step<false>(use_inv ? make_entry(e.c, e.p) : e, P);
                }
            }
        } else if (n_here == kFuTile) {
            // a whole tile: all sixteen (c, p) first (one LDS wait), then sixteen steps in coding order; an impossible symbol is
            // coded as (0, 1) -- its stream is flagged and its words are never used
            uint2 e[kFuTile];
#pragma unroll
            for (int tl = 0; tl < kFuTile; ++tl) e[tl] = *reinterpret_cast<const uint2*>(&tile[tl * kFuRowStride + lane]);
#pragma unroll
            for (int tl = 0; tl < kFuTile; ++tl) {
                const bool none = e[tl].y == 0;
                bad |= none ? 1u : 0u;
                LR.step(none ? 0u : e[tl].x, none ? 1u : e[tl].y, P);
            }
        } else {
            // (the end of a row; n_here = 0: this lane's stream has nothing in the tile)
            for (int tl = 0; tl < n_here; ++tl) {
                const EncEntry e = tile[tl * kFuRowStride + lane];
                if (e.p == 0) bad = 1;
                else if (!bad) LR.step(e.c, e.p, P);
            }
        }
        if constexpr (JUMP && KIND == kAns) {
            if (jump_in == 0 && n_here > 0) {
                a.jump_pos[jump_c0 + jump_j] = LA.out.wr;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)LA.state;
            }
            if (jump_in == 0) { jump_in = a.jump_tiles - 1u; --jump_j; } else --jump_in;
        }
        // at most kFuTile new words per stream and tile: whole chunks leave here (<= 19 pending before, < 4 after)
        if constexpr (KIND == kAns) LA.flush_chunks(); else LR.out.flush_chunks();
    }

    uint32_t n_words = 0;
    int32_t status;
    if constexpr (KIND == kAns) status = LA.finish(true, 1u, n_words);
    else status = LR.finish(1u, n_words);               // (no symbols: `range` is still all ones and nothing is sealed)
    if (!active) return;
    if (bad) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
    if (too_long) status = CST_STREAM_CAPACITY;
    a.status[s] = status;
    a.n_words[s] = status == CST_STREAM_OK ? n_words : 0u;
}

struct GaussianRaggedDecodeArgs {
    PerSymbolDecodeArgs p;           // words / offsets / stride_words / n_words / words_capacity, symbols (flat), means, stds (flat), the support
    const uint64_t* sym_offsets;     // [n_streams + 1]
    const uint32_t* order;           // null, or [n_streams]
};

// JUMP form: every "stream" of the launch is a chunk of a stream -- entry c of the jump table -- with its symbols given outright,
// not as the difference of two offsets (the table is caller data: persymbol_jump_chunks_kernel gives every entry a range inside ONE
// stream's symbols or none), and its coder started from the raw state of the jump point (p.state / p.rstate, p.n_words: per chunk).
struct GaussianRaggedChunkArgs {
    PerSymbolDecodeArgs p;
    const uint64_t* sym_lo;          // [n chunks]: first element
    const uint32_t* len;             // [n chunks]: symbols, <= jump_interval
};

// SELECT form (cst_persymbol_ragged_select.hip): every "stream" of the launch is a PIECE of a query (cst_ragged_select.hpp's
// cut).  The two roles of the other forms' one number come apart: a piece reads its parameters from element par_lo on -- the element of its
// jump point, or of its document's start without a table -- for skip + len symbols, and stores decoded symbol t >= skip at
// p.symbols[out_lo + (t - skip)].  `raw`: the pieces start from the raw state of a jump point (p.state / p.rstate per piece), else from
// all of their stream's words as the plain form does.
struct GaussianRaggedSelectArgs {
    PerSymbolDecodeArgs p;
    const uint64_t* par_lo;          // [n pieces]: first element of means / stds
    const uint64_t* out_lo;          // [n pieces]: first symbol stored, in p.symbols
    const uint32_t* skip;            // [n pieces]: symbols decoded and dropped
    const uint32_t* len;             // [n pieces]: symbols stored (skip + len <= 2^32 - 1)
    bool raw;
};

// the forms of decode_gaussian_ragged_kernel
constexpr int kRgPlain = 0, kRgJump = 1, kRgSelect = 2;
template <int MODE>
using GaussianRaggedDecodeArgsOf =
    std::conditional_t<MODE == kRgSelect, GaussianRaggedSelectArgs, std::conditional_t<MODE == kRgJump, GaussianRaggedChunkArgs, GaussianRaggedDecodeArgs>>;

// which stream (plain), table entry (JUMP) or piece (SELECT) a lane slot decodes, where its parameters begin and end, and how its coder
// starts: the plain form's expressions are the ones the kernel held before it had other forms
template <int MODE, class Args>
__device__ __forceinline__ size_t ragged_lane_stream(const Args& ra, size_t slot, size_t n_streams, bool& active) {
    if constexpr (MODE != kRgPlain) { active = slot < n_streams; return slot; }
    else return persymbol_ragged_stream(ra.order, slot, n_streams, active);
}
template <int MODE, class Args> __device__ __forceinline__ uint64_t ragged_lane_begin(const Args& ra, size_t s) {
    if constexpr (MODE == kRgSelect) return ra.par_lo[s];
    else if constexpr (MODE == kRgJump) return ra.sym_lo[s];
    else return ra.sym_offsets[s];
}
template <int MODE, class Args> __device__ __forceinline__ uint64_t ragged_lane_end(const Args& ra, size_t s) {
    if constexpr (MODE == kRgSelect) return ra.par_lo[s] + (uint64_t)ra.skip[s] + (uint64_t)ra.len[s];
    else if constexpr (MODE == kRgJump) return ra.sym_lo[s] + (uint64_t)ra.len[s];
    else return ra.sym_offsets[s + 1];
}
template <int MODE, class Args> __device__ __forceinline__ bool ragged_lane_raw(const Args& ra) {
    if constexpr (MODE == kRgSelect) return ra.raw; else return MODE == kRgJump;
}

typedef struct __attribute__((packed, aligned(4))) { v4i v; } v4i_at4;      // a 16-byte access at a 4-byte boundary

// The decoder's geometry: the tiles of LaneGeo<true> (parameter tiles of 8, a 16-slot word window, a 16-symbol output tile:
// 17 KiB per wave) in workgroups of FOUR waves -- two workgroups per CU, so two waves per SIMD cover each other's waits as
// in the rectangular small geometry, which matters more here (a wave waits for its longest lane, and a row that starts
// anywhere takes two cache lines for its eight doubles), while a batch spreads over twice as many CUs as with eight-wave
// workgroups.  The pair requests of the rectangular small geometry need rows of one length and do not apply.
constexpr int kRgDecThreads = kBlock;
constexpr size_t kRgDecLdsBytes = kErfTabBytes + (size_t)(kRgDecThreads / kWave) * LaneGeo<true>::kWaveBytes;
constexpr size_t kRgDecLdsBytesNoTab = (size_t)(kRgDecThreads / kWave) * LaneGeo<true>::kWaveBytes;

// 16-symbol output tile -> HBM: piece (lane & 3) of rows (lane >> 2) + 16 k, as store_symbol_tile16 -- but every row has its
// own start (4-byte aligned, nothing more) and its own end: the owner lane's (offset, length) come by cross-lane read, a
// piece that lies wholly inside its row is one unaligned 16-byte store, the piece at a row's end goes word by word.
static __device__ __noinline__ void store_symbol_tile_ragged(int32_t* sym, uint32_t off_lo, uint32_t off_hi, uint32_t len, uint64_t t0, int lane,
                                                      const int32_t* tile) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (lane >> 2) + 16 * k;
        const uint64_t off = ((uint64_t)(uint32_t)__shfl((int)off_hi, r) << 32) | (uint64_t)(uint32_t)__shfl((int)off_lo, r);
        const uint64_t n = (uint64_t)(uint32_t)__shfl((int)len, r);
        const uint64_t tp = t0 + 4u * (uint32_t)(lane & 3);
        if (tp >= n) continue;
        const int32_t* src = tile + r * 20 + 4 * (lane & 3);
        int32_t* dst = sym + off + tp;
        if (tp + 4 <= n) {
            const int4 v = *reinterpret_cast<const int4*>(src);
            v4i t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
            reinterpret_cast<v4i_at4*>(dst)->v = t;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (tp + (uint64_t)i < n) dst[i] = src[i];
        }
    }
}

// ... for the SELECT form: row r stores its decoded symbols [skip, n) at out + (t - skip), and nothing outside [out, out + n - skip).  A
// piece of four that lies wholly inside [skip, n) keeps the 16-byte store; the piece that holds the first stored symbol or the row's end
// goes word by word (a piece may hold both: a range of one or two symbols); a piece in front of `skip` or behind `n` stores nothing.
static __device__ __noinline__ void store_symbol_tile_select(int32_t* sym, uint32_t out_lo, uint32_t out_hi, uint32_t skip, uint32_t len, uint64_t t0,
                                                             int lane, const int32_t* tile) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (lane >> 2) + 16 * k;
        const uint64_t out = ((uint64_t)(uint32_t)__shfl((int)out_hi, r) << 32) | (uint64_t)(uint32_t)__shfl((int)out_lo, r);
        const uint64_t n = (uint64_t)(uint32_t)__shfl((int)len, r), sk = (uint64_t)(uint32_t)__shfl((int)skip, r);
        const uint64_t tp = t0 + 4u * (uint32_t)(lane & 3);
        if (tp >= n || tp + 4 <= sk) continue;
        const int32_t* src = tile + r * 20 + 4 * (lane & 3);
        if (tp >= sk && tp + 4 <= n) {
            const int4 v = *reinterpret_cast<const int4*>(src);
            v4i t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
            reinterpret_cast<v4i_at4*>(sym + out + (tp - sk))->v = t;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (tp + (uint64_t)i >= sk && tp + (uint64_t)i < n) sym[out + (tp + (uint64_t)i - sk)] = src[i];
        }
    }
}

// decode_gaussian_lane_kernel<W, S, KIND> for ragged rows: one lane per stream, parameters one tile ahead in the item mapping
// that puts consecutive lanes on consecutive addresses, the word window, FAM::left3 and the bracket search as they are.  The
// loop runs to the wave's longest stream; a lane past its own length decodes and stores nothing but goes on taking part in the
// wave-wide loads and fences.
// MODE: kRgPlain, kRgJump (a lane per table entry) or kRgSelect (a lane per piece of a query: `len` below is skip + len of the piece,
// `sym_lo` where its PARAMETERS begin; the symbols in front of `skip` run through the same loop and only their stores are left out).
template <int W, int S, int KIND, class FAM = GaussianFamily, int MODE = kRgPlain, class PT = double>
__global__ __launch_bounds__(kRgDecThreads) void decode_gaussian_ragged_kernel(const GaussianRaggedDecodeArgsOf<MODE> ra) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    using G = LaneGeo<true>;
    constexpr int kParTile = G::kParTile, kWordWindow = G::kWordWindow, kOutSyms = G::kOutSyms, kOutStride = G::kOutStride;
    static_assert(kOutSyms == 16 && kOutStride == 20, "store_symbol_tile_ragged's tile");
    const PerSymbolDecodeArgs& a = ra.p;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* erf_tab = reinterpret_cast<double2*>(smem);
    if constexpr (FAM::kErfTab) {
        erf_tab_fill(erf_tab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int lane = threadIdx.x & (kWave - 1);
    unsigned char* mine = smem + (FAM::kErfTab ? kErfTabBytes : 0) + (size_t)(threadIdx.x >> 6) * G::kWaveBytes;
    int32_t* tile = reinterpret_cast<int32_t*>(mine);
    double* par_mu = reinterpret_cast<double*>(mine + (size_t)kWave * kOutStride * 4);
    double* par_sd = par_mu + kParTile * kParStride;
    uint32_t* win = reinterpret_cast<uint32_t*>(par_sd + kParTile * kParStride);
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot - lane >= a.n_streams) return;
    bool active;
    const size_t s = ragged_lane_stream<MODE>(ra, slot, a.n_streams, active);
    const size_t se = active ? s : 0;                         // idle lanes look at stream 0's words and decode nothing
    const uint64_t sym_lo = active ? ragged_lane_begin<MODE>(ra, s) : 0, sym_hi = active ? ragged_lane_end<MODE>(ra, s) : 0;
    const bool too_long = sym_hi - sym_lo > 0xffffffffull || sym_hi < sym_lo;      // (never a chunk: at most jump_interval symbols)
    const uint32_t len = too_long ? 0u : (uint32_t)(sym_hi - sym_lo);
    const uint32_t off_lo = (uint32_t)sym_lo, off_hi = (uint32_t)(sym_lo >> 32);
    // SELECT: where the lane's symbols go, and how many of the decoded ones stay out
    uint32_t out_lo = 0, out_hi = 0, skip = 0;
    if constexpr (MODE == kRgSelect) {
        const uint64_t o = active ? ra.out_lo[s] : 0;
        out_lo = (uint32_t)o; out_hi = (uint32_t)(o >> 32); skip = active ? ra.skip[s] : 0u;
    }
    const uint64_t mx = persymbol_wave_max(len);
    const int P = a.precision;
    const uint32_t n = (uint32_t)a.n_symbols;
    const double free_weight = (double)((P >= 32 ? 0xffffffffu : ((1u << P) - 1u)) - (n - 1u));
    const float total_f = (float)(1ull << P), free_f = (float)free_weight, inv_total_f = 1.0f / total_f, inv_free_f = 1.0f / free_f;
    const double guess_shift = 0.5 - (double)a.min_symbol;            // symbol index of the real number x: x - min_symbol + 0.5
    const bool two_step_guess = (double)n * 64.0 > free_weight;      // the leak moves the guess by more than 1/64 quantile

    DirectDecoder<W, S, KIND> D;
    D.init(a, se, ragged_lane_raw<MODE>(ra));                 // (JUMP: AnsCoder::seek / RangeDecoder::seek have been done for it)
    int32_t status = D.status;

    // ---- parameter tiles: item w = it * 64 + lane of a tile is (stream j = w / 8, symbol tl = w % 8): eight consecutive lanes
    // on consecutive doubles of one stream's row, element sym_offsets[sj] + t0 + tl, predicated on len_sj (lane j's values, by
    // cross-lane read) ----
    PT mu_r[kParTile], sd_r[kParTile];              // (widened where they land in the f64 tiles)
    const PT* const means = params_as<PT>(a.means);
    const PT* const stds = params_as<PT>(a.stds);
    const int item_t = lane & (kParTile - 1), item_j0 = lane / kParTile;
    auto par_request = [&](uint64_t t0) {
#pragma unroll
        for (int it = 0; it < kParTile; ++it) {
            const int j = it * (kWave / kParTile) + item_j0;
            const uint64_t off = ((uint64_t)(uint32_t)__shfl((int)off_hi, j) << 32) | (uint64_t)(uint32_t)__shfl((int)off_lo, j);
            const uint64_t t = t0 + (uint64_t)item_t;
            // (an element that does not exist: element 0, which does -- the wave has a symbol to decode)
            const uint64_t e = t < (uint64_t)(uint32_t)__shfl((int)len, j) ? off + t : 0;
            mu_r[it] = __builtin_nontemporal_load(means + e);
            sd_r[it] = __builtin_nontemporal_load(stds + e);
        }
    };
    auto par_land = [&]() {
#pragma unroll
        for (int it = 0; it < kParTile; ++it) {
            par_mu[item_t * kParStride + it * (kWave / kParTile) + item_j0] = (double)mu_r[it];
            par_sd[item_t * kParStride + it * (kWave / kParTile) + item_j0] = (double)sd_r[it];
        }
    };
    // ---- word window: as in the lane kernel (a tile of 8 symbols takes at most 8 words; the range coder's first S / W words
    // are taken by init, before the window starts).  ANS reads downwards from its position: every index from 0 up to it exists.
    // The range coder reads upwards: an index exists below the stream's length. ----
    constexpr bool kDownward = DirectDecoder<W, S, KIND>::kDownward;
    uint32_t w_r[kParTile];
    int64_t w_first = 0;                                      // index of w_r[0]
    auto win_request = [&](int64_t first) {
        w_first = first;
        if constexpr (kDownward) {
            if (!__any(first < 0)) {                              // every lane's words exist: one pointer, eight offsets
                const uint32_t* pw = D.in + first;
#pragma unroll
                for (int i = 0; i < kParTile; ++i) w_r[i] = pw[i];
                return;
            }
#pragma unroll
            for (int i = 0; i < kParTile; ++i) {
                const int64_t p = first + i;
                w_r[i] = *(p >= 0 ? D.in + p : D.idle);
            }
        } else {
            const int64_t len = (int64_t)D.length();
            if (!__any(first < 0 || first + kParTile > len)) {
                const uint32_t* pw = D.in + first;
#pragma unroll
                for (int i = 0; i < kParTile; ++i) w_r[i] = pw[i];
                return;
            }
#pragma unroll
            for (int i = 0; i < kParTile; ++i) {
                const int64_t p = first + i;
                w_r[i] = *(p >= 0 && p < len ? D.in + p : D.idle);
            }
        }
    };
    auto win_land = [&]() {
#pragma unroll
        for (int i = 0; i < kParTile; ++i) win[(((uint32_t)(w_first + i)) & (kWordWindow - 1)) * kWave + lane] = w_r[i];
    };
    const auto window_of = [&](int ahead_tiles) -> int64_t {  // first index of the 8 words `ahead_tiles` tiles ahead
        if constexpr (kDownward) return (int64_t)D.position() - (int64_t)kParTile * (ahead_tiles + 1);
        else return (int64_t)D.position() + (int64_t)kParTile * ahead_tiles;
    };

    if (mx > 0) {
        par_request(0);
        win_request(window_of(0));
    }
    for (uint64_t t0 = 0; t0 < mx; t0 += kParTile) {
        wave_lds_fence();                                     // (the previous tile's parameters have been read)
        par_land();
        win_land();
        if (t0 + kParTile < mx) par_request(t0 + kParTile);
        win_request(window_of(1));                            // (the words one tile further: used from the next tile on)
        wave_lds_fence();
        const int n_wave = (int)(mx - t0 < (uint64_t)kParTile ? mx - t0 : (uint64_t)kParTile);
#pragma unroll 1
        for (int tl = 0; tl < n_wave; ++tl) {
            const uint64_t t = t0 + (uint64_t)tl;
            int32_t sym = 0;
            const double mu = par_mu[tl * kParStride + lane], sd = par_sd[tl * kParStride + lane];
            D.ahead = win[(((uint32_t)D.next_index()) & (kWordWindow - 1)) * kWave + lane];
            if (t < (uint64_t)len && status == CST_STREAM_OK) {
                // the reference panics on an invalid model (pybindings/stream/model.rs:654-657)
                const bool model_ok = FAM::valid(mu, sd);
                const uint32_t q = model_ok ? D.quantile(P) : 0u;
                if (!model_ok) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
                else if (D.status != CST_STREAM_OK) status = D.status;
                else {
                    // the lane kernel's search, unchanged: guess, three left cumulatives around it, then the bracket
                    const float below = (float)q + 0.5f, above = total_f - below;
                    const bool coarse = FAM::kGaussian && !__any(sd >= 200.0);          // (wave-uniform: the cheap quantile is good enough)
                    float z = coarse ? FAM::guess_z_coarse(fminf(below, above) * inv_total_f) : FAM::guess_z(fminf(below, above) * inv_total_f);
                    double x = mu + sd * (double)(below < above ? z : -z) + guess_shift;
                    if (two_step_guess) {
                        const float b1 = below - (float)fmin(fmax(x, 0.0), (double)(n - 1u)), a1 = free_f - b1;
                        z = FAM::guess_z(fmaxf(fminf(b1, a1), 0.25f) * inv_free_f);
                        x = mu + sd * (double)(b1 < a1 ? z : -z) + guess_shift;
                    }
                    const uint32_t g = (uint32_t)fmin(fmax(x + 0.5, 1.0), (double)(n - 1u));
                    // bracket [lo_i, hi_i): left(lo_i) = lo_v <= q < hi_v = left(hi_i)
                    uint32_t lo_i = 0, hi_i = n, lo_v = 0, hi_v = P >= 32 ? 0u : (1u << P);
                    uint32_t probe = g, step = 1;
                    bool up = false, down = false;
                    {
                        uint32_t v3[3];
                        FAM::left3(g, a.min_symbol, n, P, mu, sd, erf_tab, v3);
                        if (v3[1] <= q) {
                            up = true;
                            if (q < v3[2]) { lo_i = g; lo_v = v3[1]; hi_i = g + 1u; hi_v = v3[2]; }
                            else { lo_i = g + 1u; lo_v = v3[2]; probe = min(g + 2u, n - 1u); step = 2; }
                        } else {
                            down = true;
                            if (v3[0] <= q) { lo_i = g - 1u; lo_v = v3[0]; hi_i = g; hi_v = v3[1]; }
                            else { hi_i = g - 1u; hi_v = v3[0]; probe = max(g - 1u, 2u) - 1u; step = 2; }
                        }
                    }
                    while (hi_i - lo_i > 1) {
                        // (every probe lies strictly inside (lo_i, hi_i), a subset of (0, n))
                        const uint32_t v = FAM::template left<true>((int32_t)probe, a.min_symbol, (int32_t)n, P, mu, sd, erf_tab);
                        if (v <= q) { lo_i = probe; lo_v = v; up = true; } else { hi_i = probe; hi_v = v; down = true; }
                        if (up && down) probe = lo_i + (hi_i - lo_i) / 2;
                        else if (up) probe = min(lo_i + step, hi_i - 1u);
                        else probe = max(hi_i - min(step, hi_i - 1u), lo_i + 1u);
                        step *= 2;
                    }
                    const uint32_t c = lo_v, p = hi_v - lo_v;
                    if (p == 0 || c > q || (uint64_t)c + p > ((uint64_t)1 << P)) status = CST_STREAM_IMPOSSIBLE_SYMBOL;   // degenerate distribution (quantize.rs:562-565)
                    else {
                        sym = a.min_symbol + (int32_t)lo_i;
                        D.advance(q, c, p, P);
                    }
                }
            }
            // (a lane past its length writes a zero into its own LDS row: never stored)
            tile[lane * kOutStride + (int)(t % kOutSyms)] = sym;
            if (t % kOutSyms == kOutSyms - 1) {
                wave_lds_fence();
                if constexpr (MODE == kRgSelect) store_symbol_tile_select(a.symbols, out_lo, out_hi, skip, len, t - (kOutSyms - 1), lane, tile);
                else store_symbol_tile_ragged(a.symbols, off_lo, off_hi, len, t - (kOutSyms - 1), lane, tile);
                wave_lds_fence();
            }
        }
    }
    if (mx % kOutSyms != 0) {
        wave_lds_fence();
        if constexpr (MODE == kRgSelect) store_symbol_tile_select(a.symbols, out_lo, out_hi, skip, len, mx - mx % kOutSyms, lane, tile);
        else store_symbol_tile_ragged(a.symbols, off_lo, off_hi, len, mx - mx % kOutSyms, lane, tile);
    }
    if (!active) return;
    a.status[s] = too_long ? (int32_t)CST_STREAM_CAPACITY : status;
}

// ---- host side ----
// what both calls refuse before they touch the device
inline cst_status check_ragged_gaussian_args(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const void* d_symbols, const void* d_means,
                                             const void* d_stds, const void* d_sym_offsets, const void* d_words, const void* d_word_offsets,
                                             size_t stride_words, const void* d_n_words, const void* d_status, const void* d_order, size_t n_streams) {
    if (!d_symbols || !d_means || !d_stds || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!config_supported(cfg) || max_symbol <= min_symbol) return CST_ERR_INVALID_ARGUMENT;
    if (!d_word_offsets && stride_words == 0) return CST_ERR_INVALID_ARGUMENT;
    if (d_order && n_streams > 0xffffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;      // (the support limit of the rectangular calls)
    return CST_OK;
}

// ------------------------------------------------------------------------------------------------
// jump points: the encoder's JUMP form notes the table; the decoder runs every table entry as a coder of its own.  What follows knows
// nothing of the model: cst_persymbol_ragged_jump.hip and cst_persymbol_categorical_ragged.hip both hand their own chunk decoder to
// decode_jump_chunks, which launches it between the two kernels (templates, all of them: each unit's code object carries its copy,
// the host side folds them).
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
template <int = 0>       // (a template only so that every unit that launches it may hold a copy: launched as ...<>)
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

// what the jump calls refuse on top of the plain calls' refusals: an interval that is no whole number of tiles, or a table that is not
// all there (d_jump_a / d_jump_b: the state (ANS, d_jump_b unused), or lower / range (the range coder))
template <int KIND>
inline bool jump_table_bad(size_t jump_interval, const void* d_chunk_offsets, const void* d_jump_pos, const void* d_jump_a, const void* d_jump_b) {
    return jump_interval == 0 || jump_interval % kFuTile != 0 || jump_interval > 0x7fffffffull || !d_chunk_offsets || !d_jump_pos || !d_jump_a ||
           (KIND == kRange && !d_jump_b);
}

// The host side of a jump decode, whatever the model: the chunks kernel fills the scratch, `launch_chunks(p, v)` runs the caller's
// chunk decoder over it -- p: the coder's arguments, one "stream" per table entry, to which the caller adds its model's fields and the
// chunks' symbols (v.sym_lo, v.len); it returns the launch's status -- and the status kernel folds the chunks' statuses into d_status.
// `plain`: what the caller's plain decode says of the arguments, looked at AFTER the table's own refusals, as the calls always did.
template <int KIND, class LaunchChunks>
cst_status decode_jump_chunks(cst_coder_config cfg, cst_status plain, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                              size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                              size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                              const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch, int32_t* d_status, const char* name,
                              hipStream_t hs, LaunchChunks launch_chunks) {
    if (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b) || n_chunks_total > 0xffffffffull || !d_scratch)
        return CST_ERR_INVALID_ARGUMENT;
    if (plain != CST_OK) return plain;
    if (n_streams == 0) return CST_OK;
    if (n_streams > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;      // (the status kernel: a thread per stream)
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
        // (the slices handed on are absolute offsets that passed the check, or empty: `capacity` bounds them once more; the symbol
        //  ranges lie inside ONE stream's symbols)
        PerSymbolDecodeArgs p{};
        p.words = d_words; p.offsets = v.word_off; p.stride_words = 0; p.n_words = v.n_words; p.words_capacity = capacity;
        p.symbols = d_symbols; p.n_streams = n_chunks_total; p.precision = cfg.precision;
        p.status = v.status; p.state = v.state; p.rstate = v.rstate;
        const cst_status rc = launch_chunks(p, v);
        if (rc != CST_OK) return rc;
    }
    hipLaunchKernelGGL(persymbol_jump_status_kernel<>, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, hs, v, d_sym_offsets, d_word_offsets,
                       stride_words, capacity, d_chunk_offsets, d_jump_pos, d_n_words, n_streams, n_chunks_total, interval, d_status);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(name, CST_OK);
}

} // namespace cst
