// cst_persymbol.hpp -- what the translation units of the per-symbol coders share: the coder entries, the argument
// structs and decoder front ends that kernels of several files are built from, and the host helpers that cross files.
//   cst_persymbol.hip              what every family shares, the explicit models, every rectangular decoder but the Categorical ones
//   cst_persymbol_encode.hip       Gaussian / Laplace / Cauchy encoders
//   cst_persymbol_ragged.hip       streams of different lengths
//   cst_persymbol_ragged_jump.hip  ... with jump points (both share their kernels through cst_persymbol_ragged.hpp)
//   cst_persymbol_categorical.hip  Categorical models from probability matrices
//   cst_persymbol_categorical_ragged.hip  ... for streams of different lengths, plain and with jump points (they share the row tile and
//                                  pass 1 of the encoders through cst_persymbol_categorical.hpp), under both quantisers: the ragged
//                                  Categorical(perfect=True) decoder over rows that cst_categorical_perfect.hip tabulates lives here too
// EVERY KERNEL INSTANTIATION LIVES IN ONE FILE: nothing here is relocatable device code, so a second implicit instantiation would
// compile and ship the kernel twice.  A kernel needed from another file is reached through a host launcher declared here and defined
// next to the kernel.  (The exceptions are small and named where they are: categorical_entries_kernel, cst_persymbol_categorical.hpp,
// and the two kernels around a jump table, cst_persymbol_ragged.hpp.)
#pragma once
#include <type_traits>

#include "cst_range_kernels.hpp"
#include "cst_math.hpp"
#include "cst_family_policy.hpp"

namespace cst {

enum CoderKind : int { kAns = 0, kRange = 1, kChain = 2 };

// ------------------------------------------------------------------------------------------------
// The element type PT of the per-symbol parameter matrices (means / stds, a / b): double, or float.  A kernel built for
// float reads float32 and widens in registers right behind the load; the family policies, the erf path and the LDS tiles see doubles
// either way.  Widening is exact for every float32 -- subnormals and signed zeros included: v_cvt_f64_f32 honours the f32 denormal mode,
// and these kernels run with f32 denormals ON (the compiler's default for this target, .amdhsa_float_denorm_mode_32 = 3; nothing here is
// built with -fgpu-flush-denormals-to-zero) -- so the models are those of the f64 call on the widened matrices, bit for bit.
// The argument structs carry the matrices untyped; the kernel's PT says what they hold.
// ------------------------------------------------------------------------------------------------
template <class PT> __device__ __forceinline__ const PT* params_as(const void* p) { return static_cast<const PT*>(p); }
template <class PT> __device__ __forceinline__ double load_param(const PT* p) { return (double)*p; }
template <class PT> inline constexpr bool kParamF32 = std::is_same_v<PT, float>;
// parameters to one 128-byte line
template <class PT> inline constexpr int kParamsPerLine = 128 / (int)sizeof(PT);

// Every entry point that takes parameter matrices exists twice: NAME over f64 matrices and NAME_f32 over f32 ones, which the header
// declares untyped (`const void *`, as the Categorical calls take their matrices).  Both are one call of the same host template, which
// deduces PT from the pointers: the twin makes it on the arrays as floats.
inline const float* f32(const void* p) { return static_cast<const float*>(p); }

__device__ __forceinline__ EncEntry make_entry(uint32_t c, uint32_t p) {
    uint64_t m = 0;
    if (p == 1) m = ~0ull;
    else if (p > 1) {                      // floor(2^64 / p) without 128-bit arithmetic
        const uint64_t q = (~0ull) / p;    // floor((2^64 - 1) / p)
        const uint64_t r = (~0ull) - q * p;
        m = q + ((r + 1 == p) ? 1 : 0);
    }
    return EncEntry{c, p, (uint32_t)m, (uint32_t)(m >> 32)};
}

struct EntriesEncodeArgs {
    const EncEntry* entries;
    size_t n_streams, n_per_stream;
    int32_t layout, precision;
    uint32_t* words;
    size_t stride_words;
    uint32_t* n_words;
    uint64_t* state;            // ANS raw state
    cst_range_state* rstate;    // range raw state
    int32_t* status;
    uint32_t flags;
    // chain coder: the remainders stack that is popped, and the heads
    const uint32_t* pop_words; const uint64_t* pop_offsets; size_t pop_stride; uint32_t* n_pop;
    cst_chain_heads* heads;
};

// pass 2 of the two-pass encoders (encode_entries_kernel in cst_persymbol.hip, encode_entries_ragged_kernel)
constexpr int kEntryGroup = 8;     // entries requested together (8 x 16 bytes = one 128-byte line of a stream-major row)

// the fused encoders' tiles (encode_gaussian_fused_kernel in cst_persymbol_encode.hip, encode_gaussian_ragged_kernel)
constexpr int kFuTile = 16;                               // symbols per tile
constexpr int kFuStreams = 32;                            // streams per wave
constexpr int kFuIters = kFuTile * kFuStreams / kWave;    // entries per lane and tile
constexpr int kFuRingSlots = 32;
constexpr int kFuAhead = 4;                               // items requested ahead of their use (kFuIters % kFuAhead == 0)
constexpr int kFuRowStride = kFuStreams + 1;              // entries: row t of the tile starts at t * kFuRowStride (conflict-free both ways)
constexpr int kFuBlock = 256;
constexpr size_t kFuTabBytes = kErfTabBytes;              // the erf tables (cst_math.hpp)
constexpr size_t kFuWaveBytes = (size_t)kFuRingSlots * kWave * 4 + (size_t)kFuTile * kFuRowStride * sizeof(EncEntry);

// floor(2^64 / p) for 2 <= p <= 2^24 through two f64 quotients, each corrected by its exact remainder:
// 2^64 / p = 2^32 q1 + 2^32 r1 / p with q1 = floor(2^32 / p), r1 = 2^32 - q1 p
__device__ __forceinline__ EncEntry make_entry_f64(uint32_t c, uint32_t p) {
    // straight line (one model per lane: a branch would be taken by some lane every time); p <= 1 is patched in at the end
    const uint32_t pp = p > 1u ? p : 2u;
    const double inv = fast_rcp1((double)pp);                           // 2^-48: both quotients below are within one
    uint32_t q1 = f64_as_u32_hw(4294967296.0 * inv);
    int64_t r1 = (int64_t)(1ull << 32) - (int64_t)((uint64_t)q1 * pp);
    const uint32_t dn1 = r1 < 0 ? 1u : 0u, up1 = r1 >= (int64_t)pp ? 1u : 0u;
    q1 = q1 - dn1 + up1;
    const uint32_t r1u = (uint32_t)r1 + (dn1 ? pp : 0u) - (up1 ? pp : 0u);          // 0 <= r1 < p now
    const double x2 = __builtin_amdgcn_ldexp((double)r1u, 32);         // < 2^56: exact as a double
    uint32_t q2 = f64_as_u32_hw(x2 * inv);
    const int64_t r2 = (int64_t)((uint64_t)r1u << 32) - (int64_t)((uint64_t)q2 * pp);
    q2 = q2 - (r2 < 0 ? 1u : 0u) + (r2 >= (int64_t)pp ? 1u : 0u);
    const uint32_t ones = p ? 0xffffffffu : 0u;
    return EncEntry{c, p, p > 1u ? q2 : ones, p > 1u ? q1 : ones};
}

// From P = 18 on (kInvMinPrecision: the Python API's P = 24) the fused encoder's entries carry 1 / p as an f64 (2^-48:
// v_rcp_f64 + one Newton step) where the table kernels carry floor(2^64 / p): with one model per symbol the entry is built as
// often as it is used, and floor(2^64 / p) costs ~35 instructions against 4.  The (32,64) step that goes with it
// (encode_step_inv below) has the length of the table kernels' hand-scheduled one.
constexpr int kInvMinPrecision = 18;
__device__ __forceinline__ EncEntry make_entry_inv(uint32_t c, uint32_t p) {
    const double inv = fast_rcp1((double)p);                       // (p = 0: an impossible symbol, replaced before it is used)
    return EncEntry{c, p, f64_lo(inv), f64_hi(inv)};
}

// One ANS encoder step (stack.rs:1014-1048) on the 32-bit halves of a 64-bit state, 18 <= P <= 24, 1 <= p < 2^P, with
// inv = 1 / p to 2^-48:  A = emit ? state >> 32 : state  is below p 2^(64 - P) <= 2^46 p, so  A inv  is within 2^-1.9 of the
// quotient (2^-7.9 at P = 24) and its nearest integer q' is the quotient or one more; A - q' p then fits 32 signed bits and
// its sign says which.
template <int SLOTS>
__device__ __forceinline__ void encode_step_inv(EncLane<32, 64, SLOTS>& L, uint32_t c, uint32_t p, double inv, int P) {
    const uint32_t lo = (uint32_t)L.state, hi = (uint32_t)(L.state >> 32);
    const bool emit = hi >= (p << (32 - P));                       // (state >> (64 - P)) >= p
    L.out.push(lo, emit ? 1u : 0u);
    const uint32_t a0 = emit ? hi : lo, a1 = emit ? 0u : hi;
    const double af = __builtin_fma((double)a1, 4294967296.0, (double)a0);
    const double qm = af * inv + 0x1p52;                           // the integer nearest to A / p in the low mantissa bits
    const uint32_t ql = f64_lo(qm), qh = f64_hi(qm) & 0xfffffu;
    const int32_t r = (int32_t)(a0 - ql * p);                      // A - q' p, exact: -p <= r < p
    const int32_t y = r + (r < 0 ? (int32_t)(c + p) - (int32_t)(1u << P) : (int32_t)c);   // q' one too large: q = q' - 1, r + p
    L.state = ((((uint64_t)qh << 32) | ql) << P) + (uint64_t)(int64_t)y;
}

// ------------------------------------------------------------------------------------------------
// decoding with per-symbol models
// ------------------------------------------------------------------------------------------------

struct PerSymbolDecodeArgs {
    const uint32_t* words;
    const uint64_t* offsets;
    size_t stride_words;
    const uint32_t* n_words;
    int32_t* symbols;
    size_t n_streams, n_per_stream;
    int32_t layout, precision;
    int32_t min_symbol, n_symbols;
    const void* means;          // Gaussian (a family's a / b): PT matrices, PT the kernel's parameter type (params_as)
    const void* stds;
    const uint32_t* cdf_rows;   // explicit rows
    uint64_t* state;            // ANS raw
    uint32_t* n_words_out;
    cst_range_state* rstate;    // range raw
    size_t row_stride;          // explicit rows: entries from one symbol's row to the next (0: one row for all)
    // chain coder: the remainders pushed, and the heads (n_words_out = what is left of the popped stack)
    uint32_t* push_words; size_t push_stride; uint32_t* n_push;
    cst_chain_heads* heads;
    int32_t* status;
    uint32_t flags;
    uint64_t words_capacity;    // uint32 slots behind `words` (0 = unknown): see word_slice
    __device__ __forceinline__ WordSlice slice(size_t s) const { return word_slice(offsets, stride_words, n_words, s, words_capacity); }
};

struct DecodeResume { uint64_t s0, s1, s2; uint32_t pos; int32_t status; };

// Uniform (per-wave or per-lane) coder front end reading words straight from HBM.
template <int W, int S, int KIND> struct DirectDecoder;

template <int W, int S>
struct DirectDecoder<W, S, kAns> {
    using st_t = typename StateT<S>::type;
    st_t state; uint32_t rd; const uint32_t* in; int32_t status;
    uint32_t ahead;                                           // in[rd - 1], requested when the word before it was taken
    __device__ __forceinline__ void init(const PerSymbolDecodeArgs& a, size_t s, bool raw) {
        const WordSlice ws = a.slice(s);
        in = a.words + ws.off;
        rd = ws.n; status = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (int32_t)CST_STREAM_OK; state = 0; ahead = 0; idle = a.n_words + s;
        if (raw) { state = (st_t)a.state[s]; look_ahead(); return; }
        if (rd == 0) return;                                  // read_initial_state, stack.rs:440-462
        const uint32_t first = in[--rd];
        if (first == 0) { status = CST_STREAM_INVALID_DATA; rd = 0; return; }
        st_t st = first;
        while (rd > 0) { st = (st_t)((st << (W % S)) | (st_t)in[--rd]); if (st >= ((st_t)1 << (S - W))) break; }
        state = st;
        look_ahead();
    }
    // (an unconditional load from a pointer that is always valid: a conditional one makes the compiler wait for it at once)
    const uint32_t* idle;
    __device__ __forceinline__ void look_ahead() { ahead = *(rd > 0 ? in + (rd - 1) : idle); }
    // the lane-per-stream decoder keeps a window of the stream's words in LDS: where the window starts / which word is next
    static constexpr bool kDownward = true;
    __device__ __forceinline__ uint32_t position() const { return rd; }
    __device__ __forceinline__ int64_t next_index() const { return (int64_t)rd - 1; }
    __device__ __forceinline__ uint32_t length() const { return 0xffffffffu; }          // (every index below rd exists)
    __device__ __forceinline__ uint32_t quantile(int P) { return (uint32_t)state & ((1u << P) - 1u); }
    __device__ __forceinline__ void advance(uint32_t q, uint32_t c, uint32_t p, int P) {      // stack.rs:1086-1097
        st_t st = (st_t)((st_t)(state >> P) * (st_t)p + (st_t)(q - c));
        const bool refill = st < ((st_t)1 << (S - W)) && rd > 0;        // (the caller looks ahead again: once per symbol, outside
        state = refill ? (st_t)((st << (W % S)) | (st_t)ahead) : st;    //  any divergent branch)
        rd -= refill ? 1u : 0u;
    }
    __device__ __forceinline__ void finish(const PerSymbolDecodeArgs& a, size_t s, bool raw) {
        if (raw) { a.state[s] = (uint64_t)state; if (a.n_words_out) a.n_words_out[s] = rd; }
    }
    // a decoder parked between two launches over consecutive pieces of the same stream
    __device__ __forceinline__ void park(DecodeResume& r) const { r.s0 = (uint64_t)state; r.pos = rd; }
    __device__ __forceinline__ void resume(const PerSymbolDecodeArgs& a, size_t s, const DecodeResume& r) {
        in = a.words + a.slice(s).off;
        idle = a.n_words + s; status = CST_STREAM_OK; ahead = 0;
        state = (st_t)r.s0; rd = r.pos;
        look_ahead();
    }
};

template <int W, int S>
struct DirectDecoder<W, S, kRange> {
    using st_t = typename StateT<S>::type;
    RangeDecLane<W, S> L; uint32_t pos, len; const uint32_t* in; int32_t status;
    uint32_t ahead;                                           // in[pos], requested when the word before it was taken
    const uint32_t* idle;                                     // (see the ANS decoder)
    __device__ __forceinline__ void look_ahead() { ahead = *(pos < len ? in + pos : idle); }
    static constexpr bool kDownward = false;
    __device__ __forceinline__ uint32_t position() const { return pos; }
    __device__ __forceinline__ int64_t next_index() const { return (int64_t)pos; }
    __device__ __forceinline__ uint32_t length() const { return len; }
    __device__ __forceinline__ void init(const PerSymbolDecodeArgs& a, size_t s, bool raw) {
        const WordSlice ws = a.slice(s);
        in = a.words + ws.off;
        len = ws.n; pos = 0; L.status = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (int32_t)CST_STREAM_OK; idle = a.n_words + s;
        L.lower = 0; L.range = (st_t)~(st_t)0;
        if (raw) {
            const cst_range_state r = a.rstate[s];
            L.lower = (st_t)r.lower; L.range = (st_t)r.range; L.point = (st_t)r.point; pos = (uint32_t)r.position;
        } else {                                              // read_point, queue.rs:847-868
            st_t pt = 0; int num_read = 0;
            while (pos < len) { pt = (st_t)((pt << (W % S)) | (st_t)in[pos++]); if (++num_read == S / W) break; }
            if (num_read < S / W && num_read != 0) pt = (st_t)(pt << (S - num_read * W));
            L.point = pt;
        }
        status = L.status; ahead = 0;
        look_ahead();
    }
    __device__ __forceinline__ uint32_t quantile(int P) { const uint32_t q = L.peek_quantile(P); status = L.status; return q; }
    __device__ __forceinline__ void advance(uint32_t, uint32_t c, uint32_t p, int P) {
        const bool have = pos < len;
        pos += L.advance(c, p, P, have ? ahead : 0u, have) ? 1u : 0u;       // (the caller looks ahead again)
    }
    __device__ __forceinline__ void finish(const PerSymbolDecodeArgs& a, size_t s, bool raw) {
        if (raw) {
            cst_range_state r = a.rstate[s];
            r.lower = (uint64_t)L.lower; r.range = (uint64_t)L.range; r.point = (uint64_t)L.point; r.position = pos;
            a.rstate[s] = r;
        }
    }
    __device__ __forceinline__ void park(DecodeResume& r) const {
        r.s0 = (uint64_t)L.lower; r.s1 = (uint64_t)L.range; r.s2 = (uint64_t)L.point; r.pos = pos;
    }
    __device__ __forceinline__ void resume(const PerSymbolDecodeArgs& a, size_t s, const DecodeResume& r) {
        const WordSlice ws = a.slice(s);
        in = a.words + ws.off;
        idle = a.n_words + s; len = ws.n; status = CST_STREAM_OK; L.status = CST_STREAM_OK; ahead = 0;
        L.lower = (st_t)r.s0; L.range = (st_t)r.s1; L.point = (st_t)r.s2; pos = r.pos;
        look_ahead();
    }
};

// ChainCoder::decode_symbol (src/stream/chain.rs:1044-1122): P bits per symbol come off `compressed` whatever the model;
// what the symbol did not use goes onto `remainders` (flush_remainders_head, :784-796).
template <int W, int S>
struct DirectDecoder<W, S, kChain> {
    using st_t = typename StateT<S>::type;
    static constexpr uint32_t wmask = W == 32 ? 0xffffffffu : ((1u << (W % 32)) - 1u);
    st_t rh; uint32_t ch, rd, wr, cap; const uint32_t* in; uint32_t* out; int32_t status;
    uint32_t ahead; const uint32_t* idle;
    __device__ __forceinline__ void look_ahead() { ahead = *(rd > 0 ? in + (rd - 1) : idle); }
    static constexpr bool kDownward = true;
    __device__ __forceinline__ uint32_t position() const { return rd; }
    __device__ __forceinline__ int64_t next_index() const { return (int64_t)rd - 1; }
    __device__ __forceinline__ uint32_t length() const { return 0xffffffffu; }
    __device__ __forceinline__ void init(const PerSymbolDecodeArgs& a, size_t s, bool) {
        const WordSlice ws = a.slice(s);
        in = a.words + ws.off;
        rd = ws.n; idle = a.n_words + s; status = ws.bad ? (int32_t)CST_STREAM_INVALID_DATA : (int32_t)CST_STREAM_OK;
        const cst_chain_heads h = a.heads[s];
        rh = (st_t)h.remainders_head; ch = h.compressed_head;
        out = a.push_words + s * a.push_stride;
        cap = (uint32_t)(a.push_stride > 0xffffffffull ? 0xffffffffull : a.push_stride); wr = 0;
        look_ahead();
    }
    __device__ __forceinline__ uint32_t quantile(int P) {
        uint32_t word;
        if (P == W || ch < (1u << P)) {
            if (rd == 0) { status = CST_STREAM_OUT_OF_DATA; return 0u; }
            word = ahead & wmask; --rd;                       // (the caller looks ahead again after advance())
            if (P != W) ch = ((ch << (W - P)) | (word >> P)) & wmask;
        } else {
            word = ch; ch >>= P;
        }
        return P == W ? word : (word & ((1u << P) - 1u));
    }
    __device__ __forceinline__ void advance(uint32_t q, uint32_t c, uint32_t p, int P) {
        rh = (st_t)(rh * (st_t)p + (st_t)(q - c));
        if (rh >= ((st_t)1 << (S - P))) {
            if (wr < cap) out[wr] = (uint32_t)rh & wmask;
            ++wr;
            rh = (st_t)(rh >> (W % S));
        }
    }
    __device__ __forceinline__ void finish(const PerSymbolDecodeArgs& a, size_t s, bool) {
        cst_chain_heads h; h.remainders_head = (uint64_t)rh; h.compressed_head = ch; h.reserved = 0;
        a.heads[s] = h;
        a.n_words_out[s] = rd; a.n_push[s] = wr;
        if (wr > cap && a.status[s] == CST_STREAM_OK) a.status[s] = CST_STREAM_CAPACITY;
    }
};

// LDS of the lane-per-stream decoder, per wave: the symbol tile (stream-major output), one tile of parameters
// [kParTile][64 streams (+1)] for each of mean and std, and a window of kWordWindow words per stream.  Everything that comes
// from HBM is requested ONE TILE (16 symbols ~ 40 000 cycles of model search) before it is used, with coalesced loads
// where the layout allows: per-lane loads issued a symbol ahead exposed ~2300 cycles of latency per symbol (half the
// kernel's time: rocprofv3 SQ_WAIT_ANY), because a wave-wide load of 64 different cache lines takes longer than a symbol.
constexpr int kParStride = kWave + 1;                 // doubles per tile row: conflict-free writes (stream-major) and reads
// Two geometries (round 5).  BIG: parameter tiles of 16 symbols, a 32-slot word window, a 32-symbol output tile -- 34 KiB of LDS per
// wave, four waves per CU: right while a batch has one wave per SIMD anyway (65 536 streams).  SMALL: tiles of 8, a 16-slot window, a
// 16-symbol output tile (rows of 20 words) -- 17 KiB per wave, EIGHT waves per workgroup and CU: with more than one wave of streams
// per SIMD (more than 65 536 streams: e.g. a batch decoded through jump points) the second wave covers what a lone wave waits for
// (690 of its 1970 cycles per symbol, profiles/r04_sq_counters.md).
template <bool SMALL> struct LaneGeo {
    static constexpr int kParTile = SMALL ? 8 : 16;
    static constexpr int kWordWindow = 2 * kParTile;          // slots per stream, position p lives in slot p % kWordWindow
    static constexpr int kOutSyms = SMALL ? 16 : kTileSyms;   // symbols per output tile
    static constexpr int kOutStride = SMALL ? 20 : kTileStride;
    static constexpr int kThreads = SMALL ? 512 : kBlock;
    static constexpr size_t kWaveBytes = (size_t)kWave * kOutStride * 4 + 2 * (size_t)kParTile * kParStride * 8 + (size_t)kWordWindow * kWave * 4;
    static constexpr size_t kLdsBytes = kErfTabBytes + (size_t)(kThreads / kWave) * kWaveBytes;
    static constexpr size_t kLdsBytesNoTab = (size_t)(kThreads / kWave) * kWaveBytes;      // families without erf tables
};

// entries of a tabulated cdf row as decode_rows_wave_kernel reads it (cst_persymbol.hip; gaussian_rows_kernel has the whole story)
constexpr int kRowEntries = 256;

// ---- host side ----
// f(W, S) with the coder's word and state bits as std::integral_constant<int, .>: (32, 64) or (16, 32)
template <typename F> auto dispatch_word_size(cst_coder_config cfg, F&& f) {
    return cfg.word_bits == 32 ? f(std::integral_constant<int, 32>{}, std::integral_constant<int, 64>{})
                               : f(std::integral_constant<int, 16>{}, std::integral_constant<int, 32>{});
}

// what note_kernel() reports for a family's routes; float parameter matrices (PT = float) add `f32` to a name's tag list
template <class FAM, class PT = double> struct FamilyNames;
#define CST_FAMILY_NAMES(FAM, PT, word, ALONE, MORE)                                                                                      \
    template <> struct FamilyNames<FAM, PT> {                                                                                             \
        static constexpr const char* fused[2] = {"ans_encode_" word "_fused_kernel" ALONE, "range_encode_" word "_fused_kernel" ALONE};   \
        static constexpr const char* fused_ckpt[2] = {"ans_encode_" word "_fused_kernel<ckpt" MORE ">", "range_encode_" word "_fused_kernel<ckpt" MORE ">"}; \
        static constexpr const char* two_pass[2] = {"ans_encode_" word "_two_pass" ALONE, "range_encode_" word "_two_pass" ALONE};        \
        static constexpr const char* lane[3] = {"ans_decode_" word "_lane_kernel" ALONE, "range_decode_" word "_lane_kernel" ALONE, "chain_decode_" word "_lane_kernel" ALONE}; \
        static constexpr const char* lane_small[2] = {"ans_decode_" word "_lane_kernel<small" MORE ">", "range_decode_" word "_lane_kernel<small" MORE ">"}; \
        static constexpr const char* wave[2] = {"ans_decode_" word "_wave_kernel" ALONE, "range_decode_" word "_wave_kernel" ALONE};      \
        static constexpr const char* by_rows = "decode_" word "_by_rows" ALONE;                                                           \
        static constexpr const char* ragged[2][2] = {{"ans_encode_" word "_ragged_kernel" ALONE, "ans_decode_" word "_ragged_kernel" ALONE}, \
                                                     {"range_encode_" word "_ragged_kernel" ALONE, "range_decode_" word "_ragged_kernel" ALONE}}; \
        static constexpr const char* ragged_jump[2][2] = {{"ans_encode_" word "_ragged_kernel<jump" MORE ">", "ans_decode_" word "_ragged_kernel<jump" MORE ">"},      \
                                                          {"range_encode_" word "_ragged_kernel<jump" MORE ">", "range_decode_" word "_ragged_kernel<jump" MORE ">"}}; \
        static constexpr const char* ragged_select[2] = {"ans_decode_" word "_ragged_kernel<select" MORE ">", "range_decode_" word "_ragged_kernel<select" MORE ">"}; \
    }
#define CST_FAMILY_NAMES_BOTH(FAM, word) CST_FAMILY_NAMES(FAM, double, word, "", ""); CST_FAMILY_NAMES(FAM, float, word, "<f32>", ", f32")
CST_FAMILY_NAMES_BOTH(GaussianFamily, "gaussian");
CST_FAMILY_NAMES_BOTH(LaplaceFamily, "laplace");
CST_FAMILY_NAMES_BOTH(CauchyFamily, "cauchy");
#undef CST_FAMILY_NAMES_BOTH
#undef CST_FAMILY_NAMES

// raises the kernel's dynamic LDS limit to `lds` bytes, launches it and reads the launch error
template <class Kernel, class Args>
cst_status launch_with_lds(Kernel kernel, size_t blocks, int threads, size_t lds, const Args& a, hipStream_t hs) {
    CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, hs, a);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

// call<KIND, FAM>(...) for the family a Laplace / Cauchy entry point names (nothing else)
#define CST_FAMILY_CALL(call, KIND, ...)                                                                                        \
    (family == CST_FAMILY_LAPLACE ? call<KIND, LaplaceFamily>(__VA_ARGS__)                                                      \
     : family == CST_FAMILY_CAUCHY ? call<KIND, CauchyFamily>(__VA_ARGS__) : CST_ERR_INVALID_ARGUMENT)

// CST_FLAG_RAW_STATE without the state of this coder
template <int KIND> inline bool raw_state_missing(uint32_t flags, const void* d_state, const void* d_rstate) {
    return (flags & CST_FLAG_RAW_STATE) && (KIND == kAns ? d_state : d_rstate) == nullptr;
}
// more symbols than quantiles (LeakyQuantizer::new asserts this; per-symbol models hold no tables, any n <= 2^P works)
inline bool support_too_large(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol) {
    return (int64_t)max_symbol - min_symbol + 1 > ((int64_t)1 << cfg.precision);
}

// ---- defined in cst_persymbol.hip ----
cst_status check_common(cst_coder_config cfg, cst_layout layout);
cst_status fill_decode_args(PerSymbolDecodeArgs& a, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets,
                            size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols, size_t n_streams,
                            size_t n_per_stream, cst_layout layout, int32_t min_symbol, int64_t n_symbols, int32_t* d_status, uint32_t flags);
cst_status check_family_args(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, cst_layout layout,
                             const void* d_symbols, const void* d_a, const void* d_b, const void* d_words, const void* d_n_words,
                             const void* d_status, const void* raw_state, uint32_t flags);
hipError_t scratch_alloc(void** ptr, size_t bytes, hipStream_t hs);
template <int KIND> cst_status launch_encode_entries(cst_coder_config cfg, const EntriesEncodeArgs& a, hipStream_t hs);
// one piece [t0, t0 + count) of every stream over tabulated rows: decode_rows_wave_kernel (`packed`: 256-entry rows) or decode_rows_piece_wave_kernel
template <int KIND> void launch_decode_rows(cst_coder_config cfg, bool packed, const PerSymbolDecodeArgs& a, const uint32_t* rows, size_t t0,
                                            size_t count, DecodeResume* resume, bool first, bool last, hipStream_t hs);

// the entry buffer of a two-pass encode: `fill` launches the entry kernel into it (pass 1), then the sequential coder (pass 2); `a`: all but the entries
template <int KIND, typename Fill>
cst_status encode_through_entries(cst_coder_config cfg, EntriesEncodeArgs a, hipStream_t hs, Fill fill) {
    const size_t n = a.n_streams * a.n_per_stream;
    EncEntry* entries = nullptr;
    if (n > 0) {
        CST_HIP_TRY(scratch_alloc((void**)&entries, n * sizeof(EncEntry), hs));
        fill(entries, n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_hip_error(e, "entry kernel"); (void)hipFreeAsync(entries, hs); return CST_ERR_HIP; }
    }
    a.entries = entries;
    const cst_status st = launch_encode_entries<KIND>(cfg, a, hs);
    if (entries) CST_HIP_TRY(hipFreeAsync(entries, hs));
    return st;
}

template <int KIND, typename Fill>
cst_status encode_two_pass(cst_coder_config cfg, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                           uint32_t* d_n_words, uint64_t* d_state, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, hipStream_t hs, Fill fill) {
    if (cst_status st = check_common(cfg, layout)) return st;
    if (!d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (raw_state_missing<KIND>(flags, d_state, d_rstate)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EntriesEncodeArgs a{};
    a.n_streams = n_streams; a.n_per_stream = n_per_stream; a.layout = layout; a.precision = cfg.precision;
    a.words = d_words; a.stride_words = stride_words; a.n_words = d_n_words; a.state = d_state; a.rstate = d_rstate;
    a.status = d_status; a.flags = flags;
    return encode_through_entries<KIND>(cfg, a, hs, fill);
}

// the chain coder's two-pass encode
template <typename Fill>
cst_status chain_encode_common(cst_coder_config cfg, size_t n_streams, size_t n_per_stream, cst_layout layout, const uint32_t* d_pop_words,
                               const uint64_t* d_pop_offsets, size_t pop_stride, uint32_t* d_n_pop, uint32_t* d_push_words, size_t push_stride,
                               uint32_t* d_n_push, cst_chain_heads* d_heads, int32_t* d_status, hipStream_t hs, Fill fill) {
    if (cst_status st = check_common(cfg, layout)) return st;
    if (!d_heads || !d_n_pop || !d_n_push || !d_status || !d_pop_words || (n_per_stream > 0 && !d_push_words)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EntriesEncodeArgs a{};
    a.n_streams = n_streams; a.n_per_stream = n_per_stream; a.layout = layout; a.precision = cfg.precision;
    a.words = d_push_words; a.stride_words = push_stride; a.n_words = d_n_push; a.status = d_status;
    a.pop_words = d_pop_words; a.pop_offsets = d_pop_offsets; a.pop_stride = pop_stride; a.n_pop = d_n_pop; a.heads = d_heads;
    return encode_through_entries<kChain>(cfg, a, hs, fill);
}

// Few streams: cdf rows at full occupancy, then a lookup per symbol, in pieces of `piece` >= 1 positions of every stream.
// `tabulate(t0, count, rows)` launches the caller's row kernel for positions [t0, t0 + count) -- rows of `pitch` words -- and returns its
// status.  (No symbols at all: one empty piece initialises and finishes the decoders.)  `note`: for note_kernel() unless HIP failed here, or null.
template <int KIND, typename Tabulate>
cst_status decode_in_pieces(cst_coder_config cfg, const PerSymbolDecodeArgs& a, bool packed, size_t pitch, size_t piece, Tabulate tabulate,
                            hipStream_t hs, const char* note = nullptr) {
    const size_t N = a.n_per_stream;
    uint32_t* rows = nullptr;
    DecodeResume* resume = nullptr;
    CST_HIP_TRY(scratch_alloc((void**)&rows, a.n_streams * piece * pitch * sizeof(uint32_t), hs));
    hipError_t err = scratch_alloc((void**)&resume, a.n_streams * sizeof(DecodeResume), hs);
    cst_status rc = CST_OK;
    for (size_t t0 = 0; (t0 < N || (N == 0 && t0 == 0)) && err == hipSuccess && rc == CST_OK; t0 += piece) {
        const size_t count = N - t0 < piece ? N - t0 : piece;
        rc = tabulate(t0, count, rows);
        if (rc != CST_OK) break;
        launch_decode_rows<KIND>(cfg, packed, a, rows, t0, count, resume, t0 == 0, t0 + count == N, hs);
        err = hipGetLastError();
    }
    if (resume) (void)hipFreeAsync(resume, hs);
    (void)hipFreeAsync(rows, hs);
    CST_HIP_TRY(err);
    return note ? note_kernel(note, rc) : rc;
}

} // namespace cst
