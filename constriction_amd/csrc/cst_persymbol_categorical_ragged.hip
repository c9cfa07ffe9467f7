// cst_persymbol_categorical_ragged.hip -- per-symbol Categorical models (the fast quantiser of cst_categorical.hpp; the perfect one of
// cst_categorical_perfect.hip at the end of the list) for streams of
// DIFFERENT lengths, plain and with jump points (cst_persymbol.hpp has the map of the per-symbol files): stream s owns
// rows [sym_offsets[s], sym_offsets[s + 1]) of a flat probability matrix [n_total][K] and of the flat symbols.
//   categorical_entries_kernel        encoder pass 1, as it is (cst_persymbol_categorical.hpp): rows are rows, whichever stream owns them
//   encode_entries_ragged_kernel      encoder pass 2: encode_entries_kernel's ANS and range branches with one lane per stream
//   decode_categorical_ragged_kernel  decode_categorical_lane_kernel with a row index per lane
//   decode_rows_piece_ragged_kernel   Categorical(perfect=True), DESIGN.md 4.23: decode_rows_piece_wave_kernel for units of different lengths, over
//                                     rows that categorical_perfect_kernel tabulates in its ragged mode; the encoders of that model are
//                                     host glue (the quantiser in entry mode for pass 1, then encode_entries_ragged_kernel)
// Their JUMP forms note / start from the jump table of cst_*_gaussian_ragged_jump; the kernels that turn a table into chunks and chunk
// statuses into stream statuses, and the host routine around them, are the model-independent ones of cst_persymbol_ragged.hpp.  A unit of its own: the instantiations
// stay out of cst_persymbol_categorical.hip, the build's longest compile.
// Their SELECT forms decode pieces of queries, a lane (the perfect quantiser: a unit) per piece of
// cst_persymbol_ragged_select.hpp's records, between the query and status kernels of cst_ragged_select.hpp.
#include "cst_persymbol_ragged_select.hpp"
#include "cst_categorical.hpp"
#include "cst_persymbol_categorical.hpp"
#include "cst_categorical_perfect.hpp"

namespace cst {

// (CatRaggedSpan, where a stream's symbols lie: cst_categorical_perfect.hpp, for the quantiser's ragged mode too)

// ------------------------------------------------------------------------------------------------
// encoder pass 2
// ------------------------------------------------------------------------------------------------
struct EntriesRaggedEncodeArgs {
    const EncEntry* entries;         // [n_total], entry i from row i (pass 1)
    uint64_t n_total;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    size_t n_streams;
    const uint32_t* order;           // null, or [n_streams]
    int32_t precision;
    uint32_t* words;
    const uint64_t* word_offsets;    // [n_streams + 1], or null: s * stride_words
    size_t stride_words;
    uint32_t* n_words;
    int32_t* status;
};
// (the table of GaussianRaggedEncodeJumpArgs; chunks are counted in symbols here, not in tiles)
struct EntriesRaggedEncodeJumpArgs : EntriesRaggedEncodeArgs {
    uint32_t jump_interval;
    const uint64_t* jump_chunk_offsets;     // [n_streams + 1]
    uint32_t* jump_pos;
    uint64_t* jump_a;                       // ANS: the state; the range coder: lower
    uint64_t* jump_b;                       // the range coder: range
};

// One lane per stream over the entries of pass 1, lane slot i on stream order[i] (null: i).  The wave walks position t of ALL its
// streams together -- the range coder t = 0 .. mx - 1, ANS t = mx - 1 .. 0, mx the wave's longest stream -- and a lane takes a step
// where t < its own length: t, the flush_chunks() countdown and the jump counters are wave-uniform, every stream is still coded first
// to last (last to first) without a gap.  Entries come kEntryGroup at a time, one group ahead of their use, as in
// encode_entries_kernel; the loads are unconditional, from entry 0 where the lane has nothing at t (a wave with a step to take has an
// entry).
// JUMP: chunk j of a stream is symbols [j I, j I + I): a queue notes pos() BEFORE t = j I is coded, a stack AFTER it (the symbols from
// j I on are then encoded) -- what encode_gaussian_ragged_kernel<JUMP> notes.  Only where t < len: no chunk starts at a stream's end.
template <int W, int S, int KIND, bool JUMP>
__global__ __launch_bounds__(kBlock) void encode_entries_ragged_kernel(const std::conditional_t<JUMP, EntriesRaggedEncodeJumpArgs, EntriesRaggedEncodeArgs> a) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * kRingWords;
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot - lane >= a.n_streams) return;
    bool active;
    const size_t s = persymbol_ragged_stream(a.order, slot, a.n_streams, active);
    const CatRaggedSpan span(active ? a.sym_offsets[s] : 0, active ? a.sym_offsets[s + 1] : 0, a.n_total);
    const uint32_t len = span.len;
    const uint32_t mx = persymbol_wave_max(len);
    const int P = a.precision;
    const int G4 = 4 * groups_per_point(W, P);
    const EncEntry* my = a.entries + span.lo;

    const uint64_t slab_lo = !active ? 0 : (a.word_offsets ? a.word_offsets[s] : (uint64_t)s * a.stride_words);
    // (offsets that run backwards give the stream a slab of NO words: it reports CST_STREAM_CAPACITY and writes nothing)
    const uint64_t slab_hi = !active ? 0 : (a.word_offsets ? a.word_offsets[s + 1] : 0);
    const uint64_t slab_n = !active ? 0 : (a.word_offsets ? (slab_hi >= slab_lo ? slab_hi - slab_lo : 0) : (uint64_t)a.stride_words);
    std::conditional_t<KIND == kAns, EncLane<W, S>, RangeEncLane<W, S>> L;
    L.init(a.words + slab_lo, (uint32_t)(slab_n > 0xffffffffull ? 0xffffffffull : slab_n), ring, lane);
    uint32_t bad = 0;
    int countdown = G4;
    // JUMP: position t is symbol `jump_in` of chunk `jump_j` of every stream (wave-uniform counters: no division per symbol)
    uint32_t jump_in = 0, jump_j = 0;
    uint64_t jump_c0 = 0;
    if constexpr (JUMP) {
        if (KIND == kAns && mx > 0) { jump_in = (mx - 1u) % a.jump_interval; jump_j = (mx - 1u) / a.jump_interval; }
        jump_c0 = active ? a.jump_chunk_offsets[s] : 0;
    }

    const auto load = [&](uint32_t t) { return a.entries == nullptr ? EncEntry{} : (t < len ? my[t] : a.entries[0]); };
    const auto one = [&](const EncEntry e, uint32_t t) {
        const bool mine = t < len;
        if constexpr (JUMP && KIND == kRange) {
            if (jump_in == 0 && mine) {
                a.jump_pos[jump_c0 + jump_j] = L.out.wr + L.inv_n;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)L.lower;
                a.jump_b[jump_c0 + jump_j] = (uint64_t)L.range;
            }
            if (++jump_in == a.jump_interval) { jump_in = 0; ++jump_j; }
        }
        if (mine) {
            if (e.p == 0) bad = 1;
            else if (!bad) {
                if constexpr (KIND == kAns) L.template step<false>(e, P); else L.step(e.c, e.p, P);
            }
        }
        if constexpr (JUMP && KIND == kAns) {
            if (jump_in == 0 && mine) {
                a.jump_pos[jump_c0 + jump_j] = L.out.wr;
                a.jump_a[jump_c0 + jump_j] = (uint64_t)L.state;
            }
            // (selects, not `if (..) { .. --jump_j; } else --jump_in;`: the compiler merges those two decrements into one store through a
            //  selected pointer, and both counters then live in scratch memory)
            const bool first = jump_in == 0;
            jump_j -= first ? 1u : 0u;
            jump_in = first ? a.jump_interval - 1u : jump_in - 1u;
        }
        if (--countdown == 0) { countdown = G4; L.out.flush_chunks(); }
    };

    const uint32_t tail = mx % kEntryGroup;
    EncEntry cur[kEntryGroup], nxt[kEntryGroup];
    if constexpr (KIND == kAns) {
        for (uint32_t t = mx; t-- > mx - tail;) one(load(t), t);
        uint32_t g = mx - tail;                    // entries [g - kEntryGroup, g) are the next group
        if (g > 0) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) nxt[j] = load(g - 1u - (uint32_t)j);
        }
        while (g > 0) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) cur[j] = nxt[j];
            g -= kEntryGroup;
            if (g > 0) {
#pragma unroll
                for (int j = 0; j < kEntryGroup; ++j) nxt[j] = load(g - 1u - (uint32_t)j);
            }
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) one(cur[j], g + (uint32_t)(kEntryGroup - 1 - j));
        }
    } else {
        const uint32_t n_grouped = mx - tail;
        uint32_t g = 0;                            // entries [g, g + kEntryGroup) are the next group
        if (n_grouped > 0) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) nxt[j] = load((uint32_t)j);
        }
        while (g < n_grouped) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) cur[j] = nxt[j];
            g += kEntryGroup;
            if (g < n_grouped) {
#pragma unroll
                for (int j = 0; j < kEntryGroup; ++j) nxt[j] = load(g + (uint32_t)j);
            }
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) one(cur[j], g - (uint32_t)kEntryGroup + (uint32_t)j);
        }
        for (uint32_t t = n_grouped; t < mx; ++t) one(load(t), t);
    }

    uint32_t n_words = 0;
    int32_t status;
    if constexpr (KIND == kAns) status = L.finish(true, 1u, n_words);
    else status = L.finish(1u, n_words);                // (no symbols: `range` is still all ones and nothing is sealed)
    if (!active) return;
    if (bad) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
    status = span.status(status);
    a.status[s] = status;
    a.n_words[s] = status == CST_STREAM_OK ? n_words : 0u;
}

// ------------------------------------------------------------------------------------------------
// decoder
// ------------------------------------------------------------------------------------------------
struct CatRaggedDecodeArgs {
    PerSymbolDecodeArgs p;           // words / offsets / stride_words / n_words / words_capacity, symbols (flat), n_symbols = K
    const void* probs;               // [n_total][K]
    uint64_t n_total;
    const uint64_t* sym_offsets;     // [n_streams + 1]
    const uint32_t* order;           // null, or [n_streams]
};
// JUMP form: every "stream" of the launch is entry c of the jump table, with its symbols given outright (GaussianRaggedChunkArgs)
struct CatRaggedChunkArgs {
    PerSymbolDecodeArgs p;
    const void* probs;
    uint64_t n_total;
    const uint64_t* sym_lo;          // [n chunks]: first element
    const uint32_t* len;             // [n chunks]: symbols, <= jump_interval
};
// SELECT form: every "stream" of the launch is a PIECE of a query, GaussianRaggedSelectArgs with rows for parameters --
// a piece walks rows par_lo + t, t in [0, skip + len), and stores decoded symbol t >= skip at p.symbols[out_lo + (t - skip)]
struct CatRaggedSelectArgs {
    PerSymbolDecodeArgs p;
    const void* probs;
    uint64_t n_total;
    const uint64_t* par_lo;          // [n pieces]: first row
    const uint64_t* out_lo;          // [n pieces]: first symbol stored, in p.symbols
    const uint32_t* skip;            // [n pieces]: symbols decoded and dropped
    const uint32_t* len;             // [n pieces]: symbols stored (skip + len <= 2^32 - 1)
    bool raw;                        // the pieces start from the raw state of a jump point (the call has a table)
};
template <int MODE>
using CatRaggedDecodeArgsOf = std::conditional_t<MODE == kRgSelect, CatRaggedSelectArgs, std::conditional_t<MODE == kRgJump, CatRaggedChunkArgs, CatRaggedDecodeArgs>>;

// behind the tile: the row that each of the wave's 64 lanes walks at this position
constexpr size_t kCatRowTableBytes = (size_t)kWave * sizeof(uint64_t);
template <class F> constexpr size_t kCatRaggedLdsBytes = kCatTileBytes<F> + kCatRowTableBytes;
static_assert(kCatTileBytes<float> % 8 == 0 && kCatTileBytes<double> % 8 == 0, "the row table is read as 64-bit words");

// cat_stage for rows that lie anywhere: row r of the wave is row rows[r] of the matrix -- always one that exists -- and is kept
// where bit r of `live` is set.  The loads are unconditional (a conditional load is waited for at once); the 16-byte path's condition
// is the same for every row.
template <class F>
__device__ __forceinline__ void cat_stage_rows(F* tile, const F* __restrict__ probs, const uint64_t* rows, unsigned long long live, size_t K,
                                               size_t c0, int n_here, bool vec, int lane) {
    if (vec) {
        using V = typename CatVec<F>::type;
        constexpr int kV = CatVec<F>::n, kLanesPerRow = kCatChunk / kV, kRowsPerLoad = kWave / kLanesPerRow;
        const int col = (lane % kLanesPerRow) * kV, r0 = lane / kLanesPerRow;
        const bool col_ok = col < n_here;
        const F* src = probs + c0 + (size_t)(col_ok ? col : 0);
#pragma unroll 8
        for (int it = 0; it < kWave / kRowsPerLoad; ++it) {
            const int r = it * kRowsPerLoad + r0;
            const V v = *reinterpret_cast<const V*>(src + (size_t)rows[r] * K);
            if (((live >> r) & 1ull) && col_ok) {
#pragma unroll
                for (int k = 0; k < kV; ++k) tile[r * kCatPitch + col + k] = v[k];
            }
        }
    } else {
        const bool col_ok = lane < n_here;
        const F* src = probs + c0 + (size_t)(col_ok ? lane : 0);
#pragma unroll 8
        for (int r = 0; r < kWave; ++r) {
            const F v = src[(size_t)rows[r] * K];
            if (((live >> r) & 1ull) && col_ok) tile[r * kCatPitch + lane] = v;
        }
    }
}

// decode_categorical_lane_kernel for ragged rows: one LANE per stream (JUMP: per table entry), 64 per wave, one wave per workgroup.
// At position t lane r walks row sym_lo_r + t: the lanes leave their row indices in a table behind the tile, and the staging loop takes
// row r's from there.  The loop runs to the wave's longest lane; a lane past its own length stages a row that exists (row 0: a wave
// with a symbol to decode has one), decodes and stores nothing, and goes on taking part in the wave-wide loads, fences and votes.
// MODE: kRgPlain, kRgJump (a lane per table entry) or kRgSelect (a lane per piece of a query: the span below is then rows
// [par_lo, par_lo + skip + len), and the symbols in front of `skip` run through the same loop with only their stores left out).
template <int W, int S, int KIND, class F, int MODE>
__global__ __launch_bounds__(kWave) void decode_categorical_ragged_kernel(const CatRaggedDecodeArgsOf<MODE> ra) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    F* tile = reinterpret_cast<F*>(smem);
    uint64_t* rows = reinterpret_cast<uint64_t*>(smem + kCatTileBytes<F>);
    const PerSymbolDecodeArgs& a = ra.p;
    const F* probs = reinterpret_cast<const F*>(ra.probs);
    const int lane = threadIdx.x;
    const size_t slot = (size_t)blockIdx.x * kWave + (size_t)lane;
    if (slot - lane >= a.n_streams) return;
    bool active;
    const size_t s = ragged_lane_stream<MODE>(ra, slot, a.n_streams, active);
    const size_t se = active ? s : 0;                         // idle lanes look at stream 0's words and decode nothing
    const CatRaggedSpan span(active ? ragged_lane_begin<MODE>(ra, s) : 0, active ? ragged_lane_end<MODE>(ra, s) : 0, ra.n_total);
    const uint32_t len = span.len;
    const uint32_t mx = persymbol_wave_max(len);
    // SELECT: where the lane's symbols go, and how many of the decoded ones stay out
    uint64_t out_lo = 0;
    uint32_t skip = 0;
    if constexpr (MODE == kRgSelect) { out_lo = active ? ra.out_lo[s] : 0; skip = active ? ra.skip[s] : 0u; }
    const size_t K = (size_t)a.n_symbols;
    const int P = a.precision;
    const uint32_t total = 1u << P;
    const bool vec = cat_vec_ok(probs, K);
    const F* my = tile + lane * kCatPitch;

    DirectDecoder<W, S, KIND> D;
    D.init(a, se, ragged_lane_raw<MODE>(ra));                 // (JUMP: AnsCoder::seek / RangeDecoder::seek have been done for it)
    int32_t status = D.status;
    for (uint32_t t = 0; t < mx; ++t) {
        const bool here = t < len;
        if (!__any(here && status == CST_STREAM_OK)) break;             // (what follows a failure is unspecified)
        const unsigned long long live = __ballot(here);
        wave_lds_fence();                                               // (the previous position's rows have been staged)
        rows[lane] = here ? span.lo + (uint64_t)t : 0;
        CatSum<F> sum;
        for (size_t c0 = 0; c0 < K; c0 += kCatChunk) {
            const int n_here = (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk);
            wave_lds_fence();
            cat_stage_rows(tile, probs, rows, live, K, c0, n_here, vec, lane);
            wave_lds_fence();
#pragma unroll 8
            for (int j = 0; j < n_here; ++j) sum.add(my[j]);
        }
        bool search = here && status == CST_STREAM_OK;
        if (search && sum.bad()) { status = CST_STREAM_IMPOSSIBLE_SYMBOL; search = false; }
        uint32_t q = 0;
        if (search) {
            q = D.quantile(P);
            if (D.status != CST_STREAM_OK) { status = D.status; search = false; }
        }
        const F scale = cat_scale<F>(P, (uint32_t)K, search ? sum.cum : F(1));
        // entries 0 .. K - 2 have a right boundary of their own; `prev` is the left boundary of the entry looked at
        F cum = F(0);
        uint32_t prev = 0, c = 0, right = total, sym = (uint32_t)K - 1u;
        bool found = !search;
        for (size_t c0 = 0; c0 < K - 1; c0 += kCatChunk) {
            const int n_here = (int)(K - 1 - c0 < (size_t)kCatChunk ? K - 1 - c0 : (size_t)kCatChunk);
            if (K > (size_t)kCatChunk) {
                wave_lds_fence();
                cat_stage_rows(tile, probs, rows, live, K, c0, (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk), vec, lane);
            }
            wave_lds_fence();
#pragma unroll 8
            for (int j = 0; j < n_here; ++j) {
                cum = cum + my[j];
                const uint32_t r = cat_left<F>(cum, scale, (uint32_t)c0 + (uint32_t)j + 1u);
                const bool hit = !found && r > q;
                sym = hit ? (uint32_t)c0 + (uint32_t)j : sym;
                c = hit ? prev : c;
                right = hit ? r : right;
                found = found || hit;
                prev = r;
            }
            if (!__any(!found)) break;
        }
        if (!found) c = prev;                                           // the last symbol: everything up to 2^P
        int32_t decoded = 0;
        if (search) {
            const uint32_t p = right - c;
            if (p == 0 || right < c || right > total) status = CST_STREAM_IMPOSSIBLE_SYMBOL;     // an empty or wrapped interval
            else { decoded = (int32_t)sym; D.advance(q, c, p, P); }
        }
        D.look_ahead();                                                 // (once per symbol, outside any divergent branch)
        if constexpr (MODE == kRgSelect) { if (here && t >= skip) a.symbols[out_lo + (uint64_t)(t - skip)] = decoded; }
        else if (here) a.symbols[span.lo + (uint64_t)t] = decoded;
    }
    if (!active) return;
    a.status[s] = span.status(status);
    D.finish(a, s, false);
}

// ------------------------------------------------------------------------------------------------
// Categorical(perfect=True), decoder: rows in pieces.  The quantiser needs a WAVE per row, so the rows are tabulated
// first -- categorical_perfect_kernel in its ragged mode, K + 1 words each -- and then looked up; a UNIT is a stream (plain) or an entry
// of the jump table (JUMP), and the host codes groups of consecutive unit slots in pieces of positions so that the rows of one step fit
// a budget (decode_perfect_ragged_units below).
// ------------------------------------------------------------------------------------------------
struct CatPerfectPieceCommon {
    PerSymbolDecodeArgs p;           // as CatRaggedDecodeArgs / CatRaggedChunkArgs; n_streams: ALL unit slots
    const uint32_t* rows;            // [units of the group][count][K + 1]
    uint64_t n_total;
    size_t u0, n_units;              // the group: slots [u0, u0 + n_units)
    uint64_t t0, count;              // the piece: positions [t0, t0 + count) of every unit
    uint64_t max_len;                // a longer unit is refused (CST_STREAM_CAPACITY)
    DecodeResume* resume;            // [n_units]: the group's decoders between two pieces
};
struct CatPerfectPieceArgs : CatPerfectPieceCommon {
    const uint64_t* sym_offsets;     // [n_streams + 1]
    const uint32_t* order;           // null, or [n_streams]
};
struct CatPerfectPieceChunkArgs : CatPerfectPieceCommon {
    const uint64_t* sym_lo;          // [n chunks]
    const uint32_t* len;
};
// SELECT: a unit is a piece of a query (CatRaggedSelectArgs' fields); `span` is skip + len per piece, what the quantiser's ragged mode
// takes for a unit's length beside par_lo
struct CatPerfectPieceSelectArgs : CatPerfectPieceCommon {
    const uint64_t* par_lo;
    const uint64_t* out_lo;
    const uint32_t* skip;
    const uint32_t* len;
    const uint32_t* span;
    bool raw;
};
template <int MODE>
using CatPerfectPieceArgsOf =
    std::conditional_t<MODE == kRgSelect, CatPerfectPieceSelectArgs, std::conditional_t<MODE == kRgJump, CatPerfectPieceChunkArgs, CatPerfectPieceArgs>>;

// decode_rows_piece_wave_kernel (cst_persymbol.hip) for units of different lengths: one WAVE per unit, the same search over the
// tabulated rows, symbols to symbols[lo_u + t].  A unit is initialised in the piece with t0 = 0 (JUMP: from the raw state of its jump
// point), parked in `resume` after every piece that does not hold its last position, and FINISHED -- status written -- in the piece that
// does; an empty or refused unit finishes in the first piece.  In the pieces after its last one its wave returns at once.  Everything a
// wave does is uniform over its lanes (the coder's state is), so the ballots and shuffles of the search have every lane.
// MODE == kRgSelect: a unit is a piece of a query, positions [0, skip + len) over rows from par_lo on; position t >= skip goes to
// symbols[out_lo + (t - skip)], the positions in front of it are decoded and dropped; the status goes to the piece's slot.
template <int W, int S, int KIND, int MODE>
__global__ __launch_bounds__(kBlock) void decode_rows_piece_ragged_kernel(const CatPerfectPieceArgsOf<MODE> ra) {
    static_assert(KIND == kAns || KIND == kRange, "a stack or a queue");
    const PerSymbolDecodeArgs& a = ra.p;
    const int lane = threadIdx.x & (kWave - 1);
    const size_t u = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (u >= ra.n_units) return;
    bool active;
    const size_t s = ragged_lane_stream<MODE>(ra, ra.u0 + u, a.n_streams, active);
    if (!active) return;                                                // (a slot whose order entry names no stream)
    const CatRaggedSpan span(ragged_lane_begin<MODE>(ra, s), ragged_lane_end<MODE>(ra, s), ra.n_total);
    const bool over = (uint64_t)span.len > ra.max_len;
    const uint64_t len = over ? 0 : (uint64_t)span.len;
    if (ra.t0 != 0 && ra.t0 >= len) return;                             // finished in an earlier piece
    const uint64_t end = len < ra.t0 + ra.count ? len : ra.t0 + ra.count;
    const bool finishes = end == len;
    const int P = a.precision;
    const uint32_t n = (uint32_t)a.n_symbols;
    uint64_t out_lo = 0, skip = 0;
    if constexpr (MODE == kRgSelect) { out_lo = ra.out_lo[s]; skip = (uint64_t)ra.skip[s]; }

    DirectDecoder<W, S, KIND> D;
    int32_t status;
    if (ra.t0 == 0) { D.init(a, s, ragged_lane_raw<MODE>(ra)); status = D.status; }
    else { const DecodeResume r = ra.resume[u]; D.resume(a, s, r); status = r.status; }
    for (uint64_t t = ra.t0; t < end && status == CST_STREAM_OK; ++t) {
        const uint32_t* row = ra.rows + ((uint64_t)u * ra.count + (t - ra.t0)) * ((uint64_t)n + 1);
        const uint32_t q = D.quantile(P);
        if (D.status != CST_STREAM_OK) { status = D.status; break; }
        uint32_t base = 0, left_over = n;             // invariant: row[base] <= q
        while (left_over > 63) {
            const uint32_t stride = (left_over + 63) / 64;
            const uint32_t off = (uint32_t)lane * stride;
            const bool valid = off < left_over;
            const uint32_t val = valid ? row[base + off] : 0u;
            const unsigned long long m = __ballot(valid && val <= q);
            const uint32_t k = max((uint32_t)__popcll(m), 1u);
            const uint32_t adv = (k - 1) * stride;
            base += adv;
            left_over = min(stride, left_over - adv);
        }
        const uint32_t val = ((uint32_t)lane <= left_over) ? row[base + lane] : 0u;
        const unsigned long long m = __ballot((uint32_t)lane < left_over && val <= q);
        const uint32_t k = (uint32_t)__popcll(m);
        const uint32_t c = __shfl(val, (int)(k > 0 ? k - 1 : 0), 64), nxt = __shfl(val, (int)min(k, 63u), 64);
        const uint32_t p = nxt - c;
        // (a bad or non-converged row starts with 0xffffffff: k == 0 or c > q)
        if (p == 0 || k == 0 || c > q || (uint64_t)c + p > ((uint64_t)1 << P)) { status = CST_STREAM_IMPOSSIBLE_SYMBOL; break; }
        if constexpr (MODE == kRgSelect) { if (lane == 0 && t >= skip) a.symbols[out_lo + (t - skip)] = (int32_t)(base + k - 1); }
        else if (lane == 0) a.symbols[span.lo + t] = (int32_t)(base + k - 1);
        D.advance(q, c, p, P);
        D.look_ahead();
    }
    if (lane != 0) return;
    if (finishes) { a.status[s] = over ? (int32_t)CST_STREAM_CAPACITY : span.status(status); D.finish(a, s, false); }
    else { DecodeResume r{}; D.park(r); r.status = status; ra.resume[u] = r; }
}

// ---- host side: one route whatever the batch ----
static constexpr const char* kCatRaggedEncodeNames[2][2] = {{"ans_encode_categorical_ragged_two_pass", "range_encode_categorical_ragged_two_pass"},
                                                            {"ans_encode_categorical_ragged_two_pass<jump>", "range_encode_categorical_ragged_two_pass<jump>"}};
static constexpr const char* kCatRaggedDecodeNames[2][2] = {{"ans_decode_categorical_ragged_kernel", "range_decode_categorical_ragged_kernel"},
                                                            {"ans_decode_categorical_ragged_kernel<jump>", "range_decode_categorical_ragged_kernel<jump>"}};

static constexpr const char* kCatPerfectRaggedEncodeNames[2][2] = {
    {"ans_encode_categorical_perfect_ragged_two_pass", "range_encode_categorical_perfect_ragged_two_pass"},
    {"ans_encode_categorical_perfect_ragged_two_pass<jump>", "range_encode_categorical_perfect_ragged_two_pass<jump>"}};
static constexpr const char* kCatPerfectRaggedDecodeNames[2][2] = {
    {"ans_decode_categorical_perfect_ragged_by_rows", "range_decode_categorical_perfect_ragged_by_rows"},
    {"ans_decode_categorical_perfect_ragged_by_rows<jump>", "range_decode_categorical_perfect_ragged_by_rows<jump>"}};

// what all sixteen calls refuse before they touch the device (`perfect`: the limits of check_categorical_args, cst_persymbol_categorical.hip)
static cst_status check_categorical_ragged_args(cst_coder_config cfg, const void* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                                const void* d_sym_offsets, const void* d_words, const void* d_word_offsets, size_t stride_words,
                                                const void* d_n_words, const void* d_status, size_t n_streams, bool perfect = false) {
    if (!d_symbols || !d_probs || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (prob_bytes != 4 && prob_bytes != 8) return CST_ERR_INVALID_ARGUMENT;
    if (!config_supported(cfg)) return CST_ERR_INVALID_ARGUMENT;
    if (!d_word_offsets && stride_words == 0) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;          // (a launch has at most 2^31 - 1 blocks; an order names 32-bit indices)
    // from_floating_point_probabilities_fast: room for a nonzero probability each plus one; perfectly_quantized_probabilities: a unit of
    // weight for each, and the quantiser's slots (check_categorical_args)
    const uint64_t total = (uint64_t)1 << cfg.precision;
    const uint64_t limit = !perfect ? total - 2 : total < (uint64_t)kCatPerfectMaxK ? total : (uint64_t)kCatPerfectMaxK;
    if (n_symbols < 2 || (uint64_t)n_symbols > limit) return CST_ERR_MODEL;
    return CST_OK;
}

// PERFECT: pass 1 is the device quantiser in entry mode over the flat matrix (one workgroup per row); pass 2 is the same kernel
template <int KIND, bool JUMP, bool PERFECT = false>
static cst_status encode_categorical_ragged(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                            size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                            uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                            size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_a,
                                            uint64_t* d_jump_b, int32_t* d_status, hipStream_t hs) {
    if constexpr (JUMP)
        if (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b)) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_categorical_ragged_args(cfg, d_symbols, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                      stride_words, d_n_words, d_status, n_streams, PERFECT)) return st;
    // (pass 1: a block per 64 rows; PERFECT: a block per row)
    if (PERFECT ? n_total > 0x7fffffffull : (n_total + kWave - 1) / kWave > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    std::conditional_t<JUMP, EntriesRaggedEncodeJumpArgs, EntriesRaggedEncodeArgs> a{};
    a.n_total = n_total; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.order = d_order; a.precision = cfg.precision;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride_words = stride_words; a.n_words = d_n_words; a.status = d_status;
    if constexpr (JUMP) {
        a.jump_interval = (uint32_t)jump_interval; a.jump_chunk_offsets = d_chunk_offsets; a.jump_pos = d_jump_pos; a.jump_a = d_jump_a;
        a.jump_b = d_jump_b;
    }
    const char* name = (PERFECT ? kCatPerfectRaggedEncodeNames : kCatRaggedEncodeNames)[JUMP][KIND == kRange];
    EncEntry* entries = nullptr;
    if (n_total > 0) {
        // pass 1 over the flat matrix, sized by n_total: no read-back of sym_offsets
        CST_HIP_TRY(scratch_alloc((void**)&entries, n_total * sizeof(EncEntry), hs));
        const dim3 grid((unsigned)((n_total + kWave - 1) / kWave));
        if constexpr (PERFECT) {
            CatPerfectArgs r{};
            r.probs = d_probs; r.prob_bytes = prob_bytes; r.K = (uint32_t)n_symbols; r.P = cfg.precision; r.layout = CST_LAYOUT_STREAM_MAJOR;
            r.n_streams = 1; r.N = n_total; r.t0 = 0; r.count = n_total;
            r.symbols = d_symbols; r.entries = entries;
            const cst_status rc = launch_categorical_perfect(r, hs);     // (it has read its launch error)
            if (rc != CST_OK) { (void)hipFreeAsync(entries, hs); return note_kernel(name, rc); }
        } else if (prob_bytes == 4)
            hipLaunchKernelGGL(categorical_entries_kernel<float>, grid, dim3(kWave), kCatTileBytes<float>, hs, cfg.precision, (uint32_t)n_symbols,
                               d_symbols, reinterpret_cast<const float*>(d_probs), n_total, entries);
        else
            hipLaunchKernelGGL(categorical_entries_kernel<double>, grid, dim3(kWave), kCatTileBytes<double>, hs, cfg.precision, (uint32_t)n_symbols,
                               d_symbols, reinterpret_cast<const double*>(d_probs), n_total, entries);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_hip_error(e, "entry kernel"); (void)hipFreeAsync(entries, hs); return note_kernel(name, CST_ERR_HIP); }
    }
    a.entries = entries;
    const size_t blocks = (n_streams + kBlock - 1) / kBlock;
    const size_t lds = (size_t)(kBlock / kWave) * kRingWords * sizeof(uint32_t);
    const cst_status st = dispatch_word_size(cfg, [&](auto W, auto S) {
        return launch_with_lds(encode_entries_ragged_kernel<W, S, KIND, JUMP>, blocks, kBlock, lds, a, hs);
    });
    if (entries) {
        const hipError_t e = hipFreeAsync(entries, hs);
        if (e != hipSuccess && st == CST_OK) { set_hip_error(e, "hipFreeAsync(entries, hs)"); return note_kernel(name, CST_ERR_HIP); }
    }
    return note_kernel(name, st);
}

template <int KIND, int MODE, class Args>
static cst_status launch_decode_categorical_ragged(cst_coder_config cfg, const Args& a, int32_t prob_bytes, hipStream_t hs) {
    const size_t blocks = (a.p.n_streams + kWave - 1) / kWave;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    return dispatch_word_size(cfg, [&](auto W, auto S) {
        if (prob_bytes == 4) return launch_with_lds(decode_categorical_ragged_kernel<W, S, KIND, float, MODE>, blocks, kWave, kCatRaggedLdsBytes<float>, a, hs);
        return launch_with_lds(decode_categorical_ragged_kernel<W, S, KIND, double, MODE>, blocks, kWave, kCatRaggedLdsBytes<double>, a, hs);
    });
}

template <int KIND>
static cst_status decode_categorical_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                            size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                            int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                            const uint32_t* d_order, int32_t* d_status, hipStream_t hs) {
    if (cst_status st = check_categorical_ragged_args(cfg, d_symbols, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                      stride_words, d_n_words, d_status, n_streams)) return st;
    if (n_streams == 0) return CST_OK;
    CatRaggedDecodeArgs a{};
    a.p.words = d_words; a.p.offsets = d_word_offsets; a.p.stride_words = stride_words; a.p.n_words = d_n_words; a.p.words_capacity = words_capacity;
    a.p.symbols = d_symbols; a.p.n_streams = n_streams; a.p.precision = cfg.precision; a.p.min_symbol = 0; a.p.n_symbols = n_symbols;
    a.p.status = d_status;
    a.probs = d_probs; a.n_total = n_total; a.sym_offsets = d_sym_offsets; a.order = d_order;
    return note_kernel(kCatRaggedDecodeNames[0][KIND == kRange], launch_decode_categorical_ragged<KIND, kRgPlain>(cfg, a, prob_bytes, hs));
}

// the Categorical chunk decoder between the two table kernels (decode_jump_chunks, cst_persymbol_ragged.hpp)
template <int KIND>
static cst_status decode_categorical_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                 size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                 int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                 size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                 const uint32_t* d_jump_pos, const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch,
                                                 int32_t* d_status, hipStream_t hs) {
    const cst_status plain = check_categorical_ragged_args(cfg, d_symbols, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                           stride_words, d_n_words, d_status, n_streams);
    const char* name = kCatRaggedDecodeNames[1][KIND == kRange];
    return decode_jump_chunks<KIND>(cfg, plain, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams,
                                    jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_a, d_jump_b, d_scratch, d_status, name, hs,
                                    [&](const PerSymbolDecodeArgs& p, const PerSymbolJumpScratch& v) {
        // (the chunk decoder bounds the symbol ranges by n_total)
        CatRaggedChunkArgs a{};
        a.p = p; a.p.min_symbol = 0; a.p.n_symbols = n_symbols;
        a.probs = d_probs; a.n_total = n_total; a.sym_lo = v.sym_lo; a.len = v.len;
        const cst_status rc = launch_decode_categorical_ragged<KIND, kRgJump>(cfg, a, prob_bytes, hs);
        return rc == CST_OK ? rc : note_kernel(name, rc);
    });
}

// ---- Categorical(perfect=True): rows in pieces, for groups of units ----
// The rows of one step -- `units` consecutive unit slots times `piece` positions, K + 1 words each -- stay within the budget (64 MiB of
// rows, CST_PERFECT_RAGGED_BUDGET words): units = clamp(budget / (K + 1), 1, n_units), piece = clamp(budget / (units (K + 1)), 1, bound),
// `bound` the longest unit there may be.  For every group, for every piece: tabulate, then decode; the decoders of a group are parked in
// `resume` between its pieces.  Without the groups a table of many chunks at large K would not fit: one position of ALL units is
// n_units (K + 1) words.  `pa`: everything but the group, the piece, the rows and the resume scratch.
template <int KIND, int MODE, class PieceArgs>
static cst_status decode_perfect_ragged_units(cst_coder_config cfg, PieceArgs pa, const void* d_probs, int32_t prob_bytes, uint64_t bound, hipStream_t hs) {
    const size_t n_units = pa.p.n_streams, pitch = (size_t)pa.p.n_symbols + 1;
    const size_t budget = knobs().perfect_ragged_budget;
    size_t units = budget / pitch;
    units = units < 1 ? 1 : units > n_units ? n_units : units;
    const uint64_t last = bound ? bound : 1;                            // (no symbols at all: one piece initialises and finishes the decoders)
    uint64_t piece = budget / (units * pitch);
    piece = piece < 1 ? 1 : piece > last ? last : piece;
    uint32_t* rows = nullptr;
    DecodeResume* resume = nullptr;
    CST_HIP_TRY(scratch_alloc((void**)&rows, units * (size_t)piece * pitch * sizeof(uint32_t), hs));
    hipError_t err = scratch_alloc((void**)&resume, units * sizeof(DecodeResume), hs);
    cst_status rc = CST_OK;
    CatPerfectRaggedArgs r{};
    r.probs = d_probs; r.prob_bytes = prob_bytes; r.K = (uint32_t)pa.p.n_symbols; r.P = cfg.precision; r.rows = rows; r.pitch = pitch;
    r.n_total = pa.n_total; r.n_all = n_units; r.max_len = pa.max_len;
    if constexpr (MODE == kRgSelect) { r.sym_lo = pa.par_lo; r.len = pa.span; }
    else if constexpr (MODE == kRgJump) { r.sym_lo = pa.sym_lo; r.len = pa.len; }
    else { r.sym_offsets = pa.sym_offsets; r.order = pa.order; }
    pa.rows = rows; pa.resume = resume;
    for (size_t u0 = 0; u0 < n_units && err == hipSuccess && rc == CST_OK; u0 += units) {
        const size_t n_here = n_units - u0 < units ? n_units - u0 : units;
        for (uint64_t t0 = 0; t0 < last && err == hipSuccess && rc == CST_OK; t0 += piece) {
            const uint64_t count = last - t0 < piece ? last - t0 : piece;
            r.u0 = u0; r.n_streams = n_here; r.t0 = (size_t)t0; r.count = (size_t)count;
            rc = launch_categorical_perfect_ragged(r, hs);
            if (rc != CST_OK) break;
            pa.u0 = u0; pa.n_units = n_here; pa.t0 = t0; pa.count = count;
            const dim3 grid((unsigned)((n_here * kWave + kBlock - 1) / kBlock));
            dispatch_word_size(cfg, [&](auto W, auto S) {
                hipLaunchKernelGGL((decode_rows_piece_ragged_kernel<W, S, KIND, MODE>), grid, dim3(kBlock), 0, hs, pa);
                return 0;
            });
            err = hipGetLastError();
        }
    }
    if (resume) (void)hipFreeAsync(resume, hs);
    (void)hipFreeAsync(rows, hs);
    CST_HIP_TRY(err);
    return rc;
}

template <int KIND>
static cst_status decode_categorical_perfect_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_total, size_t max_len, int32_t* d_symbols,
                                                    const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, int32_t* d_status,
                                                    hipStream_t hs) {
    if (cst_status st = check_categorical_ragged_args(cfg, d_symbols, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                      stride_words, d_n_words, d_status, n_streams, true)) return st;
    if (n_streams == 0) return CST_OK;
    CatPerfectPieceArgs a{};
    a.p.words = d_words; a.p.offsets = d_word_offsets; a.p.stride_words = stride_words; a.p.n_words = d_n_words; a.p.words_capacity = words_capacity;
    a.p.symbols = d_symbols; a.p.n_streams = n_streams; a.p.precision = cfg.precision; a.p.min_symbol = 0; a.p.n_symbols = n_symbols;
    a.p.status = d_status;
    a.n_total = n_total; a.sym_offsets = d_sym_offsets; a.order = d_order;
    a.max_len = max_len > 0xffffffffull ? 0xffffffffull : (uint64_t)max_len;          // (a coder has at most 2^32 - 1 symbols)
    return note_kernel(kCatPerfectRaggedDecodeNames[0][KIND == kRange], decode_perfect_ragged_units<KIND, kRgPlain>(cfg, a, d_probs, prob_bytes, a.max_len, hs));
}

// the piece decoder over the table's entries, between the two table kernels (decode_jump_chunks): an entry has at most jump_interval symbols
template <int KIND>
static cst_status decode_categorical_perfect_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                         size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_probs,
                                                         int32_t prob_bytes, int32_t n_symbols, size_t n_total, int32_t* d_symbols,
                                                         const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                                         const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint32_t* d_jump_pos,
                                                         const uint64_t* d_jump_a, const uint64_t* d_jump_b, void* d_scratch, int32_t* d_status,
                                                         hipStream_t hs) {
    const cst_status plain = check_categorical_ragged_args(cfg, d_symbols, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                           stride_words, d_n_words, d_status, n_streams, true);
    const char* name = kCatPerfectRaggedDecodeNames[1][KIND == kRange];
    return decode_jump_chunks<KIND>(cfg, plain, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams,
                                    jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos, d_jump_a, d_jump_b, d_scratch, d_status, name, hs,
                                    [&](const PerSymbolDecodeArgs& p, const PerSymbolJumpScratch& v) {
        CatPerfectPieceChunkArgs a{};
        a.p = p; a.p.min_symbol = 0; a.p.n_symbols = n_symbols;
        a.n_total = n_total; a.sym_lo = v.sym_lo; a.len = v.len; a.max_len = (uint64_t)jump_interval;
        const cst_status rc = decode_perfect_ragged_units<KIND, kRgJump>(cfg, a, d_probs, prob_bytes, (uint64_t)jump_interval, hs);
        return rc == CST_OK ? rc : note_kernel(name, rc);
    });
}

// ---- random access: the SELECT forms of the two decoders between the kernels of cst_ragged_select.hpp ----
static constexpr const char* kCatRaggedSelectNames[2][2] = {
    {"ans_decode_categorical_ragged_kernel<select>", "range_decode_categorical_ragged_kernel<select>"},
    {"ans_decode_categorical_perfect_ragged_by_rows<select>", "range_decode_categorical_perfect_ragged_by_rows<select>"}};

// What the Categorical calls refuse of a query that ragged_select_queries_kernel has accepted, as a WHOLE and before it gets a piece:
//   - a stream whose rows reach beyond the n_total rows there are: CatRaggedSpan over the stream, as the plain decoders judge it (a
//     piece's own span, inside the decoders, then always lies inside the matrix);
//   - the perfect quantiser: a piece longer than max_len, CST_STREAM_CAPACITY.  The longest piece of a query is its first: without a
//     table first + count, with one first % I + count, or I where the query goes on into the next chunk.
__global__ void cat_select_queries_kernel(const RaggedSelect b, uint64_t n_total, uint64_t max_len, int32_t* __restrict__ status) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= b.n_queries || status[q] != CST_STREAM_OK) return;
    const SelectQuery r = select_query(b, q);                             // (passed once already)
    if (r.status != CST_STREAM_OK) return;
    int32_t st = CatRaggedSpan(b.sym_offsets[r.s], b.sym_offsets[r.s + 1], n_total).status(CST_STREAM_OK);
    const uint64_t longest = r.count == 0 ? 0                             // (an empty query has no piece)
                             : b.interval == 0 ? r.first + r.count : min(r.first % b.interval + r.count, (uint64_t)b.interval);
    if (st == CST_STREAM_OK && longest > max_len) st = CST_STREAM_CAPACITY;
    status[q] = st;
}

// the perfect quantiser's ragged mode takes a unit's rows as (first row, length): a piece's length there is skip + len
__global__ void cat_select_spans_kernel(const uint32_t* __restrict__ skip, const uint32_t* __restrict__ len, size_t n_pieces,
                                        uint32_t* __restrict__ span) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_pieces) span[p] = skip[p] + len[p];                         // (<= 2^32 - 1: inside one document)
}
// (the spans lie behind the piece records, in the four bytes per piece that cst_persymbol_ragged_select_scratch_bytes rounds up by)
static_assert(sizeof(cst_range_state) + 4 * 8 + 6 * 4 <= kPsSelectPieceBytes, "a piece record and its span");

// decode_ragged_select (cst_persymbol_ragged_select.hip) with rows for parameters.  PERFECT: the pieces are the units of
// decode_perfect_ragged_units, none longer than max_piece_len (with a table: than the interval).
template <int KIND, bool PERFECT>
static cst_status decode_categorical_ragged_select(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                   size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                   int32_t n_symbols, size_t n_total, size_t max_piece_len, const uint64_t* d_sym_offsets,
                                                   size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                   const uint32_t* d_jump_pos, const uint64_t* d_jump_a, const uint64_t* d_jump_b,
                                                   const uint32_t* d_query_stream, const uint64_t* d_query_first, const uint64_t* d_query_count,
                                                   size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                   const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, hipStream_t hs) {
    // a table is an interval and ALL its arrays (jump_table_bad: the jump decoders' rule), or nothing at all
    const bool table = jump_interval != 0 || d_chunk_offsets || d_jump_pos || d_jump_a || d_jump_b;
    if (table && (jump_table_bad<KIND>(jump_interval, d_chunk_offsets, d_jump_pos, d_jump_a, d_jump_b) || n_chunks_total > 0xffffffffull))
        return CST_ERR_INVALID_ARGUMENT;
    if (n_pieces_total > 0xffffffffull || (d_query_first == nullptr) != (d_query_count == nullptr)) return CST_ERR_INVALID_ARGUMENT;
    // (every CST_ERR_INVALID_ARGUMENT in front of the plain call's CST_ERR_MODEL)
    const cst_status plain = check_categorical_ragged_args(cfg, d_symbols_out, d_probs, prob_bytes, n_symbols, d_sym_offsets, d_words, d_word_offsets,
                                                           stride_words, d_n_words, d_status, n_streams, PERFECT);
    if (plain == CST_ERR_INVALID_ARGUMENT) return plain;
    if (n_queries > 0 && (!d_query_stream || !d_piece_offsets || !d_out_offsets || !d_scratch)) return CST_ERR_INVALID_ARGUMENT;
    if (n_queries > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    if (plain != CST_OK) return plain;
    if (n_queries == 0) return CST_OK;
    const char* name = kCatRaggedSelectNames[PERFECT][KIND == kRange];
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
    // (a coder has at most 2^32 - 1 symbols; with a table no piece is longer than the interval)
    uint64_t max_len = !PERFECT || max_piece_len > 0xffffffffull ? 0xffffffffull : (uint64_t)max_piece_len;
    if (PERFECT && jump_interval != 0 && max_len > (uint64_t)jump_interval) max_len = (uint64_t)jump_interval;
    hipLaunchKernelGGL(cat_select_queries_kernel, dim3(q_grid), dim3(256), 0, hs, b, (uint64_t)n_total, max_len, d_status);
    CST_HIP_TRY(hipGetLastError());
    if (n_pieces_total > 0) {
        const unsigned p_grid = (unsigned)((n_pieces_total + 255) / 256);
        dispatch_word_size(cfg, [&](auto W, auto S) {
            hipLaunchKernelGGL((persymbol_select_pieces_kernel<W, S, KIND>), dim3(p_grid), dim3(256), 0, hs, b, d_words, d_jump_a, d_jump_b, d_status, v);
            return 0;
        });
        CST_HIP_TRY(hipGetLastError());
        // (the slices handed on are absolute offsets that passed the check, or empty: the capacity bounds them once more)
        PerSymbolDecodeArgs p{};
        p.words = d_words; p.offsets = v.word_off; p.stride_words = 0; p.n_words = v.n_words; p.words_capacity = b.words_capacity;
        p.symbols = d_symbols_out; p.n_streams = n_pieces_total; p.precision = cfg.precision; p.min_symbol = 0; p.n_symbols = n_symbols;
        p.status = v.status; p.state = v.state; p.rstate = v.rstate;
        cst_status rc;
        if constexpr (PERFECT) {
            uint32_t* span = reinterpret_cast<uint32_t*>(v.status + n_pieces_total);
            hipLaunchKernelGGL(cat_select_spans_kernel, dim3(p_grid), dim3(256), 0, hs, v.skip, v.len, n_pieces_total, span);
            CST_HIP_TRY(hipGetLastError());
            CatPerfectPieceSelectArgs a{};
            a.p = p; a.n_total = n_total; a.par_lo = v.par_lo; a.out_lo = v.out_lo; a.skip = v.skip; a.len = v.len; a.span = span;
            a.raw = jump_interval != 0;
            a.max_len = max_len;
            rc = decode_perfect_ragged_units<KIND, kRgSelect>(cfg, a, d_probs, prob_bytes, a.max_len, hs);
        } else {
            CatRaggedSelectArgs a{};
            a.p = p; a.probs = d_probs; a.n_total = n_total; a.par_lo = v.par_lo; a.out_lo = v.out_lo; a.skip = v.skip; a.len = v.len;
            a.raw = jump_interval != 0;
            rc = launch_decode_categorical_ragged<KIND, kRgSelect>(cfg, a, prob_bytes, hs);
        }
        if (rc != CST_OK) return note_kernel(name, rc);
    }
    hipLaunchKernelGGL(ragged_select_status_kernel<0>, dim3(q_grid), dim3(256), 0, hs, b, v.folded(), d_status);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(name, CST_OK);
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_ans_encode_categorical_ragged(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                             size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                             uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words,
                                             int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kAns, false>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order, d_words,
                                                  d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr, d_status,
                                                  (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_ragged(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                               int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                               const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                               uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kRange, false>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order, d_words,
                                                    d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr, d_status,
                                                    (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                             size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                             int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                             const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_categorical_ragged<kAns>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols, n_total,
                                           d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                               size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                               int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                               size_t n_streams, const uint32_t* d_order, int32_t* d_status, void* stream) {
    return decode_categorical_ragged<kRange>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols,
                                             n_total, d_symbols, d_sym_offsets, n_streams, d_order, d_status, (hipStream_t)stream);
}

// ---- jump points: the plain calls' arguments, then the interval and the table ----

cst_status cst_ans_encode_categorical_ragged_jump(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                  int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                  const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                  uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos,
                                                  uint64_t* d_jump_state, int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kAns, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order, d_words,
                                                 d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_state,
                                                 nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_ragged_jump(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                    const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                    uint32_t* d_n_words, size_t jump_interval, const uint64_t* d_chunk_offsets,
                                                    uint32_t* d_jump_pos, uint64_t* d_jump_lower, uint64_t* d_jump_range, int32_t* d_status,
                                                    void* stream) {
    return encode_categorical_ragged<kRange, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order, d_words,
                                                   d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos, d_jump_lower,
                                                   d_jump_range, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                  size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                  int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                  size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                  const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch, int32_t* d_status,
                                                  void* stream) {
    return decode_categorical_ragged_jump<kAns>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols,
                                                n_total, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos,
                                                d_jump_state, nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_total, int32_t* d_symbols, const uint64_t* d_sym_offsets,
                                                    size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                    const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                    void* d_scratch, int32_t* d_status, void* stream) {
    return decode_categorical_ragged_jump<kRange>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols,
                                                  n_total, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total, d_jump_pos,
                                                  d_jump_lower, d_jump_range, d_scratch, d_status, (hipStream_t)stream);
}

// ---- Categorical(perfect=True): the same argument lists; the plain decoders take max_len after n_total ----

cst_status cst_ans_encode_categorical_perfect_ragged(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                     int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                     const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                     uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kAns, false, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order,
                                                        d_words, d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr,
                                                        d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_perfect_ragged(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                       int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                       const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets,
                                                       size_t stride_words, uint32_t* d_n_words, int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kRange, false, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order,
                                                          d_words, d_word_offsets, stride_words, d_n_words, 0, nullptr, nullptr, nullptr, nullptr,
                                                          d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_perfect_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                     size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_probs,
                                                     int32_t prob_bytes, int32_t n_symbols, size_t n_total, size_t max_len, int32_t* d_symbols,
                                                     const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order, int32_t* d_status,
                                                     void* stream) {
    return decode_categorical_perfect_ragged<kAns>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                   n_symbols, n_total, max_len, d_symbols, d_sym_offsets, n_streams, d_order, d_status,
                                                   (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_perfect_ragged(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                       size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_probs,
                                                       int32_t prob_bytes, int32_t n_symbols, size_t n_total, size_t max_len, int32_t* d_symbols,
                                                       const uint64_t* d_sym_offsets, size_t n_streams, const uint32_t* d_order,
                                                       int32_t* d_status, void* stream) {
    return decode_categorical_perfect_ragged<kRange>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                     n_symbols, n_total, max_len, d_symbols, d_sym_offsets, n_streams, d_order, d_status,
                                                     (hipStream_t)stream);
}

cst_status cst_ans_encode_categorical_perfect_ragged_jump(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                          int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                          const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets,
                                                          size_t stride_words, uint32_t* d_n_words, size_t jump_interval,
                                                          const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_state,
                                                          int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kAns, true, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order,
                                                       d_words, d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos,
                                                       d_jump_state, nullptr, d_status, (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_perfect_ragged_jump(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                            int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                            const uint32_t* d_order, uint32_t* d_words, const uint64_t* d_word_offsets,
                                                            size_t stride_words, uint32_t* d_n_words, size_t jump_interval,
                                                            const uint64_t* d_chunk_offsets, uint32_t* d_jump_pos, uint64_t* d_jump_lower,
                                                            uint64_t* d_jump_range, int32_t* d_status, void* stream) {
    return encode_categorical_ragged<kRange, true, true>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_total, d_sym_offsets, n_streams, d_order,
                                                         d_words, d_word_offsets, stride_words, d_n_words, jump_interval, d_chunk_offsets, d_jump_pos,
                                                         d_jump_lower, d_jump_range, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_perfect_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                          size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                          const void* d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                          int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                                          size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                          const uint32_t* d_jump_pos, const uint64_t* d_jump_state, void* d_scratch,
                                                          int32_t* d_status, void* stream) {
    return decode_categorical_perfect_ragged_jump<kAns>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                        n_symbols, n_total, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets,
                                                        n_chunks_total, d_jump_pos, d_jump_state, nullptr, d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_perfect_ragged_jump(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                            size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                            const void* d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                            int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                                                            size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                            const uint32_t* d_jump_pos, const uint64_t* d_jump_lower,
                                                            const uint64_t* d_jump_range, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_categorical_perfect_ragged_jump<kRange>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                          n_symbols, n_total, d_symbols, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets,
                                                          n_chunks_total, d_jump_pos, d_jump_lower, d_jump_range, d_scratch, d_status,
                                                          (hipStream_t)stream);
}

// ---- random access: the words, the plain decode's model arguments (the perfect pair: max_piece_len after n_total), the streams, the
// table (all zero / NULL: none), the queries ----

cst_status cst_ans_decode_categorical_ragged_select(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets, size_t n_streams,
                                                    size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                    const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                                    const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                    const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                    const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_categorical_ragged_select<kAns, false>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                         n_symbols, n_total, 0, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets, n_chunks_total,
                                                         d_jump_pos, d_jump_state, nullptr, d_query_stream, d_query_first, d_query_count, n_queries,
                                                         d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status,
                                                         (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_ragged_select(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                      size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_probs,
                                                      int32_t prob_bytes, int32_t n_symbols, size_t n_total, const uint64_t* d_sym_offsets,
                                                      size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                      const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                      const uint32_t* d_query_stream, const uint64_t* d_query_first, const uint64_t* d_query_count,
                                                      size_t n_queries, const uint64_t* d_piece_offsets, size_t n_pieces_total,
                                                      int32_t* d_symbols_out, const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status,
                                                      void* stream) {
    return decode_categorical_ragged_select<kRange, false>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                           n_symbols, n_total, 0, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets,
                                                           n_chunks_total, d_jump_pos, d_jump_lower, d_jump_range, d_query_stream, d_query_first,
                                                           d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets,
                                                           d_scratch, d_status, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_perfect_ragged_select(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                            size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                            const void* d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                            size_t max_piece_len, const uint64_t* d_sym_offsets, size_t n_streams,
                                                            size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                            const uint32_t* d_jump_pos, const uint64_t* d_jump_state, const uint32_t* d_query_stream,
                                                            const uint64_t* d_query_first, const uint64_t* d_query_count, size_t n_queries,
                                                            const uint64_t* d_piece_offsets, size_t n_pieces_total, int32_t* d_symbols_out,
                                                            const uint64_t* d_out_offsets, void* d_scratch, int32_t* d_status, void* stream) {
    return decode_categorical_ragged_select<kAns, true>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                        n_symbols, n_total, max_piece_len, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets,
                                                        n_chunks_total, d_jump_pos, d_jump_state, nullptr, d_query_stream, d_query_first, d_query_count,
                                                        n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets, d_scratch, d_status,
                                                        (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_perfect_ragged_select(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                                              size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                              const void* d_probs, int32_t prob_bytes, int32_t n_symbols, size_t n_total,
                                                              size_t max_piece_len, const uint64_t* d_sym_offsets, size_t n_streams,
                                                              size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                                              const uint32_t* d_jump_pos, const uint64_t* d_jump_lower, const uint64_t* d_jump_range,
                                                              const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                                              const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets,
                                                              size_t n_pieces_total, int32_t* d_symbols_out, const uint64_t* d_out_offsets,
                                                              void* d_scratch, int32_t* d_status, void* stream) {
    return decode_categorical_ragged_select<kRange, true>(cfg, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes,
                                                          n_symbols, n_total, max_piece_len, d_sym_offsets, n_streams, jump_interval, d_chunk_offsets,
                                                          n_chunks_total, d_jump_pos, d_jump_lower, d_jump_range, d_query_stream, d_query_first,
                                                          d_query_count, n_queries, d_piece_offsets, n_pieces_total, d_symbols_out, d_out_offsets,
                                                          d_scratch, d_status, (hipStream_t)stream);
}

} // extern "C"
