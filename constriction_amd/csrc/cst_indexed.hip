// cst_indexed.hip -- indexed table coding: every symbol names one of K tabulated models that share a support and a
// precision, the way a learned codec drives an entropy coder (a hyperprior's scale quantised to one of K levels):
//   coder.encode_symbols_reverse(symbols.zip(indices.map(|k| &tables[k])))      src/stream/stack.rs:784-849 (ANS)
//   encoder.encode_symbols(...) / decoder.decode_symbols(...)                   src/stream/queue.rs:612-705, 968-1033 (range)
// with tables[k] a ContiguousCategoricalEntropyModel (src/stream/model/categorical/contiguous.rs:673-700).
// One lane per stream in the geometry of the shared-table kernels (cst_ans_kernels.hpp, cst_range_kernels.hpp): the set's image is
// staged into LDS once per workgroup, symbols and indices travel through wave-private LDS tiles, words through the per-lane rings,
// and the end of a stream is EncLane::finish / RangeEncLane::finish -- the container is the other kernels' by construction.
//   image   rows[K][n + 1] of left cumulatives, 16-bit entries for P <= 16 and 32-bit above, the last one (2^P) modulo the entry
//           width: p = (c[i + 1] - c[i]) mod 2^P needs no special case for the last symbol;
//           buckets[K][2^b + 1] (decoders only): the symbol that holds quantile j 2^(P - b), and n - 1 behind them
//   encode  two row reads, then the exact state / p through floor(2^64 / p) from two f64 quotients (make_entry_f64: off the
//           state's chain, a quad ahead) resp. the range step
//   decode  bucket[q >> (P - b)] and its successor bound a binary search of the row (no step for most quantiles)
// An index >= K or a symbol outside the support is clamped before any address is formed and fails its stream alone.
#include <new>
#include <vector>

#include "cst_indexed.hpp"

namespace cst {

struct IndexedEncodeArgs {
    const unsigned char* image; uint32_t rows_bytes;
    int32_t pitch, n_symbols, n_tables, min_symbol, precision;
    const int32_t* symbols; const void* indices;
    size_t n_streams, n_per_stream;
    uint32_t* words; size_t stride_words; uint32_t* n_words;
    uint64_t* state; cst_range_state* rstate;                 // the coder's state in front of its seal, or null
    int32_t* status;
};

struct IndexedDecodeArgs {
    const unsigned char* image; uint32_t rows_bytes, image_bytes;
    int32_t pitch, n_symbols, n_tables, min_symbol, precision, bucket_bits, bucket_wide;
    const uint32_t* words; const uint64_t* offsets; size_t stride_words; uint64_t words_capacity; const uint32_t* n_words;
    const void* indices; int32_t* symbols;
    size_t n_streams, n_per_stream;
    uint64_t* state; uint32_t* n_words_out; cst_range_state* rstate;      // what is left of the coder, or null
    int32_t* status;
};

// global -> registers for a tile of indices, in tile_fetch's lane mapping (uint8: a row's 32 indices are 32 bytes, four per lane)
template <class IDX>
__device__ __forceinline__ void index_tile_fetch(const IDX* __restrict__ idx, bool vec, size_t n_streams, size_t N, size_t s0, size_t t0,
                                                 int lane, int32_t (&r)[kTileSyms]) {
    if constexpr (sizeof(IDX) == 4) {
        if (vec) tile_fetch<true>(reinterpret_cast<const int32_t*>(idx), n_streams, N, s0, t0, lane, r);
        else tile_fetch<false>(reinterpret_cast<const int32_t*>(idx), n_streams, N, s0, t0, lane, r);
    } else if (vec) {
        const int chunk = lane & 7;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const size_t s = s0 + (size_t)((lane >> 3) + 8 * k);
            uint32_t w = 0;
            if (s < n_streams) w = *reinterpret_cast<const uint32_t*>(idx + s * N + t0 + 4 * chunk);
            r[4 * k + 0] = (int32_t)(w & 0xffu); r[4 * k + 1] = (int32_t)((w >> 8) & 0xffu);
            r[4 * k + 2] = (int32_t)((w >> 16) & 0xffu); r[4 * k + 3] = (int32_t)(w >> 24);
        }
    } else {
        const int col = lane & 31;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const size_t s = s0 + (size_t)((lane >> 5) + 2 * k);
            r[k] = (s < n_streams) ? (int32_t)idx[s * N + t0 + col] : 0;
        }
    }
}

__device__ __forceinline__ void symbol_tile_fetch(const int32_t* __restrict__ sym, bool vec, size_t n_streams, size_t N, size_t s0, size_t t0,
                                                  int lane, int32_t (&r)[kTileSyms]) {
    if (vec) tile_fetch<true>(sym, n_streams, N, s0, t0, lane, r);
    else tile_fetch<false>(sym, n_streams, N, s0, t0, lane, r);
}

// LDS: [word rings, one per wave][tiles, one per wave][rows of the image]
template <int KIND, class IDX, bool WIDE>
__global__ __launch_bounds__(kBlock) void indexed_encode_kernel(const IndexedEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Lane = std::conditional_t<KIND == kAns, EncLane<32, 64, kIxRingSlots>, RangeEncLane<32, 64, kIxRingSlots>>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_in_block = threadIdx.x >> 6;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + wave_in_block * (kIxRingSlots * kWave);
    int32_t* tile = reinterpret_cast<int32_t*>(smem + kIxRingBytes) + wave_in_block * (kWave * kTileStride);
    const unsigned char* rows = smem + kIxFixedLds;
    stage_image(smem + kIxFixedLds, a.image, a.rows_bytes);
    __syncthreads();

    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t s0 = wave * kWave;
    if (s0 >= a.n_streams) return;                              // whole wave idle (after the only barrier)
    const size_t s = s0 + lane;
    const bool active = s < a.n_streams;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols, K = (uint32_t)a.n_tables, pitch = (uint32_t)a.pitch, pmask = (1u << P) - 1u;
    const IDX* indices = reinterpret_cast<const IDX*>(a.indices);
    const bool vec = N % 4 == 0 && (reinterpret_cast<uintptr_t>(a.symbols) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(indices) & (sizeof(IDX) == 4 ? 15 : 3)) == 0;
    const int gmask = P <= 12 ? 3 : 1;                          // a memory point every 16 symbols (at most 7 words), or every 8 (7)

    Lane L;
    L.init(a.words + (active ? s : 0) * a.stride_words,
           active ? (uint32_t)(a.stride_words > 0xffffffffull ? 0xffffffffull : a.stride_words) : 0u, ring, lane);

    // (c, p) of a packed position; the ANS coder's entry carries floor(2^64 / p) as well
    auto entry = [&](uint32_t packed) -> EncEntry {
        const uint32_t i = packed & 0xffffu, k = packed >> 16;
        L.bad = max(L.bad, (i >= nsym || k >= K) ? nsym : 0u);
        const uint32_t e = min(k, K - 1u) * pitch + min(i, nsym - 1u);
        const uint32_t c = row_at<WIDE>(rows, e), p = (row_at<WIDE>(rows, e + 1u) - c) & pmask;
        if constexpr (KIND == kAns) return make_entry_f64(c, p);
        else return EncEntry{c, p, 0u, 0u};
    };
    auto flush = [&]() { L.out.flush_chunks(); };
    const int32_t* row = a.symbols + (active ? s : 0) * N;
    const IDX* irow = indices + (active ? s : 0) * N;
    auto direct = [&](size_t t) {                               // the ragged end of a row: at most 31 symbols
        const EncEntry e = entry(active ? pack_position(row[t], (int32_t)irow[t], a.min_symbol, nsym, K) : 0u);
        if constexpr (KIND == kAns) L.template step<false>(e, P);
        else L.step(e.c, e.p, P);
        flush();
    };

    const size_t n_full = N / kTileSyms;
    int32_t rs[kTileSyms], rx[kTileSyms];
    auto fetch = [&](size_t tb) {
        symbol_tile_fetch(a.symbols, vec, a.n_streams, N, s0, tb * kTileSyms, lane, rs);
        index_tile_fetch<IDX>(indices, vec, a.n_streams, N, s0, tb * kTileSyms, lane, rx);
    };
    auto to_lds = [&]() {
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < kTileSyms; ++k) rs[k] = (int32_t)pack_position(rs[k], rx[k], a.min_symbol, nsym, K);
        if (vec) tile_to_lds<true>(tile, lane, rs);
        else tile_to_lds<false>(tile, lane, rs);
        wave_lds_fence();
    };
    const int32_t* my = tile + lane * kTileStride;

    if constexpr (KIND == kAns) {
        // the stack codes a row last symbol first
        for (size_t t = N; t > n_full * kTileSyms;) direct(--t);
        if (n_full > 0) {
            fetch(n_full - 1);
            for (size_t tb = n_full; tb-- > 0;) {
                to_lds();
                if (tb > 0) fetch(tb - 1);
                constexpr int NG = kTileSyms / 4;
                int4 v = *reinterpret_cast<const int4*>(my + 4 * (NG - 1));
                EncEntry e3 = entry((uint32_t)v.w), e2 = entry((uint32_t)v.z), e1 = entry((uint32_t)v.y), e0 = entry((uint32_t)v.x);
#pragma unroll
                for (int j = NG - 1; j >= 0; --j) {
                    EncEntry n3 = e3, n2 = e2, n1 = e1, n0 = e0;
                    if (j > 0) {
                        v = *reinterpret_cast<const int4*>(my + 4 * (j - 1));
                        n3 = entry((uint32_t)v.w); n2 = entry((uint32_t)v.z); n1 = entry((uint32_t)v.y); n0 = entry((uint32_t)v.x);
                    }
                    L.template step<false>(e3, P); L.template step<false>(e2, P); L.template step<false>(e1, P); L.template step<false>(e0, P);
                    e3 = n3; e2 = n2; e1 = n1; e0 = n0;
                    if ((j & gmask) == 0) flush();
                }
            }
        }
    } else {
        if (n_full > 0) {
            fetch(0);
            for (size_t tb = 0; tb < n_full; ++tb) {
                to_lds();
                if (tb + 1 < n_full) fetch(tb + 1);
                int4 v = *reinterpret_cast<const int4*>(my);
                EncEntry e0 = entry((uint32_t)v.x), e1 = entry((uint32_t)v.y), e2 = entry((uint32_t)v.z), e3 = entry((uint32_t)v.w);
#pragma unroll
                for (int j = 0; j < kTileSyms / 4; ++j) {
                    EncEntry n0 = e0, n1 = e1, n2 = e2, n3 = e3;
                    if (j + 1 < kTileSyms / 4) {
                        v = *reinterpret_cast<const int4*>(my + 4 * (j + 1));
                        n0 = entry((uint32_t)v.x); n1 = entry((uint32_t)v.y); n2 = entry((uint32_t)v.z); n3 = entry((uint32_t)v.w);
                    }
                    // the branch-free step; a quad in which some lane leaves a long Inverted run is repeated with the general one
                    const auto lower0 = L.lower, range0 = L.range;
                    const uint32_t wr0 = L.out.wr, inv_n0 = L.inv_n, inv_first0 = L.inv_first;
                    bool slow = false;
                    L.step_inline(e0.c, e0.p, P, slow); L.step_inline(e1.c, e1.p, P, slow);
                    L.step_inline(e2.c, e2.p, P, slow); L.step_inline(e3.c, e3.p, P, slow);
                    if (__any(slow)) {
                        L.lower = lower0; L.range = range0; L.out.wr = wr0; L.inv_n = inv_n0; L.inv_first = inv_first0;
                        L.step(e0.c, e0.p, P); L.step(e1.c, e1.p, P); L.step(e2.c, e2.p, P); L.step(e3.c, e3.p, P);
                    }
                    e0 = n0; e1 = n1; e2 = n2; e3 = n3;
                    if (((j + 1) & gmask) == 0) flush();
                }
            }
        }
        for (size_t t = n_full * kTileSyms; t < N; ++t) direct(t);
    }

    uint32_t n_words = 0;
    int32_t status;
    uint64_t end_state = 0;
    cst_range_state end_rstate{};
    if constexpr (KIND == kAns) {
        end_state = (uint64_t)L.state;
        status = L.finish(true, nsym, n_words);
    } else {
        end_rstate.lower = (uint64_t)L.lower; end_rstate.range = (uint64_t)L.range;
        end_rstate.inverted_n = L.inv_n; end_rstate.inverted_first = L.inv_first;
        status = L.finish(nsym, n_words);
    }
    if (!active) return;
    if constexpr (KIND == kAns) { if (a.state) a.state[s] = end_state; }
    else { if (a.rstate) a.rstate[s] = end_rstate; }
    a.status[s] = status;
    a.n_words[s] = (status == CST_STREAM_OK) ? n_words : 0u;
}

// LDS: [word rings, one per wave][tiles, one per wave: the indices of a tile, overwritten by its symbols][rows and buckets of the image]
template <int KIND, class IDX, bool WIDE>
__global__ __launch_bounds__(kBlock) void indexed_decode_kernel(const IndexedDecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Lane = std::conditional_t<KIND == kAns, DecLane<32, 64, kIxRingSlots, kIxAhead>, RangeDecLane<32, 64, kIxRingSlots, kIxAhead>>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_in_block = threadIdx.x >> 6;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + wave_in_block * (kIxRingSlots * kWave);
    int32_t* tile = reinterpret_cast<int32_t*>(smem + kIxRingBytes) + wave_in_block * (kWave * kTileStride);
    const unsigned char* rows = smem + kIxFixedLds;
    const unsigned char* buckets = rows + a.rows_bytes;
    stage_image(smem + kIxFixedLds, a.image, a.image_bytes);
    __syncthreads();

    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t s0 = wave * kWave;
    if (s0 >= a.n_streams) return;
    const size_t s = s0 + lane;
    const bool active = s < a.n_streams;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const uint32_t K = (uint32_t)a.n_tables, pitch = (uint32_t)a.pitch, pmask = (1u << P) - 1u;
    const uint32_t bstride = (1u << a.bucket_bits) + 1u;
    const int shift = P - a.bucket_bits;
    const bool bucket_wide = a.bucket_wide != 0;
    const IDX* indices = reinterpret_cast<const IDX*>(a.indices);
    const bool vec = N % 4 == 0 && (reinterpret_cast<uintptr_t>(a.symbols) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(indices) & (sizeof(IDX) == 4 ? 15 : 3)) == 0;
    const int gmask = P <= 12 ? 3 : 1;                          // the window moves every 16 symbols (at most 7 words), or every 8 (7)

    Lane L;
    const WordSlice ws = active ? word_slice(a.offsets, a.stride_words, a.n_words, s, a.words_capacity) : WordSlice{0, 0u, false};
    L.init(a.words + ws.off, ws.n, ring, lane);
    if constexpr (KIND == kAns) L.read_initial_state();
    L.in.prime();
    wave_lds_fence();
    bool bad_index = false;

    auto next_symbol = [&](uint32_t k_raw) -> int32_t {
        bad_index |= k_raw >= K;
        const uint32_t k = min(k_raw, K - 1u);
        uint32_t idx, c, p;
        if constexpr (KIND == kAns) {
            const uint32_t q = (uint32_t)L.state & pmask;
            const uint32_t next_word = *L.in.slot(L.in.rd - 1u + L.in.shift);      // (ignored unless the state refills)
            indexed_lookup<WIDE>(rows, buckets, bucket_wide, bstride, pitch, k, q, shift, pmask, idx, c, p);
            const uint64_t st = (L.state >> P) * (uint64_t)p + (uint64_t)(q - c);           // stack.rs:1086-1097
            const bool refill = st < (1ull << 32) && L.in.rd > 0;
            L.state = refill ? ((st << 32) | (uint64_t)next_word) : st;
            L.in.rd -= refill ? 1u : 0u;
        } else {
            const uint32_t q = L.peek_quantile(P);
            const uint32_t next_word = L.in.peek();
            indexed_lookup<WIDE>(rows, buckets, bucket_wide, bstride, pitch, k, q, shift, pmask, idx, c, p);
            L.in.pos += L.advance(c, p, P, next_word, L.in.pos < L.in.len) ? 1u : 0u;
        }
        return a.min_symbol + (int32_t)idx;
    };

    const size_t n_full = N / kTileSyms;
    int32_t* my = tile + lane * kTileStride;
    if (n_full > 0) {
        int32_t rx[kTileSyms];
        index_tile_fetch<IDX>(indices, vec, a.n_streams, N, s0, 0, lane, rx);
        for (size_t tb = 0; tb < n_full; ++tb) {
            wave_lds_fence();
            if (vec) tile_to_lds<true>(tile, lane, rx);
            else tile_to_lds<false>(tile, lane, rx);
            wave_lds_fence();
            if (tb + 1 < n_full) index_tile_fetch<IDX>(indices, vec, a.n_streams, N, s0, (tb + 1) * kTileSyms, lane, rx);
#pragma unroll
            for (int j = 0; j < kTileSyms / 4; ++j) {
                const int4 k4 = *reinterpret_cast<const int4*>(my + 4 * j);
                int4 v;
                v.x = next_symbol((uint32_t)k4.x); v.y = next_symbol((uint32_t)k4.y);
                v.z = next_symbol((uint32_t)k4.z); v.w = next_symbol((uint32_t)k4.w);
                *reinterpret_cast<int4*>(my + 4 * j) = v;
                if (((j + 1) & gmask) == 0) L.in.advance_window();
            }
            wave_lds_fence();
            if (vec) tile_store<true>(a.symbols, a.n_streams, N, s0, tb * kTileSyms, lane, tile);
            else tile_store<false>(a.symbols, a.n_streams, N, s0, tb * kTileSyms, lane, tile);
        }
    }
    {
        int32_t* row = a.symbols + (active ? s : 0) * N;
        const IDX* irow = indices + (active ? s : 0) * N;
        for (size_t t = n_full * kTileSyms; t < N; ++t) {
            const int32_t v = next_symbol(active ? (uint32_t)(int32_t)irow[t] : 0u);
            if (active) row[t] = v;
            L.in.advance_window();
        }
    }
    if (!active) return;
    a.status[s] = (ws.bad || bad_index) ? (int32_t)CST_STREAM_INVALID_DATA : L.status;
    if constexpr (KIND == kAns) {
        if (a.state) a.state[s] = (uint64_t)L.state;
        if (a.n_words_out) a.n_words_out[s] = L.in.rd;
    } else if (a.rstate) {
        cst_range_state r{};
        r.lower = (uint64_t)L.lower; r.range = (uint64_t)L.range; r.point = (uint64_t)L.point; r.position = L.in.pos;
        a.rstate[s] = r;
    }
}

// ---- host side ----
static constexpr const char* kIxNames[2][2] = {{"ans_encode_indexed_kernel", "ans_decode_indexed_kernel"},
                                               {"range_encode_indexed_kernel", "range_decode_indexed_kernel"}};

// everything that can be said about a call without the device; `tables` is read last, and only once it is known to be a handle
static cst_status check_indexed_args(const cst_table_set* tables, cst_coder_config cfg, const void* d_symbols, const void* d_indices,
                                     int32_t index_bytes, size_t n_per_stream, cst_layout layout, const void* d_words, const void* d_n_words,
                                     const void* d_status, uint32_t flags) {
    if (!tables || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (n_per_stream > 0 && (!d_symbols || !d_indices)) return CST_ERR_INVALID_ARGUMENT;
    if (index_bytes != 1 && index_bytes != 4) return CST_ERR_INVALID_ARGUMENT;
    if (cfg.word_bits != 32 || cfg.state_bits != 64) return CST_ERR_INVALID_ARGUMENT;      // the (32, 64) preset only
    if (layout != CST_LAYOUT_STREAM_MAJOR || flags != CST_FLAG_NONE) return CST_ERR_INVALID_ARGUMENT;
    if (!table_set_alive(tables) || cfg.precision != tables->precision) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

static cst_status check_indexed_device(const cst_table_set* tables, size_t n_streams) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != tables->device) return CST_ERR_INVALID_ARGUMENT;
    if ((n_streams + kBlock - 1) / kBlock > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

template <int KIND>
static cst_status encode_indexed(const cst_table_set* tables, cst_coder_config cfg, const int32_t* d_symbols, const void* d_indices,
                                 int32_t index_bytes, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                 size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, cst_range_state* d_rstate, int32_t* d_status,
                                 uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_indexed_args(tables, cfg, d_symbols, d_indices, index_bytes, n_per_stream, layout, d_words, d_n_words, d_status, flags))
        return st;
    if (n_streams == 0) return CST_OK;
    if (cst_status st = check_indexed_device(tables, n_streams)) return st;
    IndexedEncodeArgs a{};
    a.image = tables->d_image; a.rows_bytes = tables->rows_bytes;
    a.pitch = tables->pitch; a.n_symbols = tables->n_symbols; a.n_tables = tables->n_tables; a.min_symbol = tables->min_symbol;
    a.precision = tables->precision;
    a.symbols = d_symbols; a.indices = d_indices; a.n_streams = n_streams; a.n_per_stream = n_per_stream;
    a.words = d_words; a.stride_words = stride_words; a.n_words = d_n_words; a.state = d_state; a.rstate = d_rstate; a.status = d_status;
    const size_t blocks = (n_streams + kBlock - 1) / kBlock, lds = kIxFixedLds + tables->rows_bytes;
    cst_status rc;
    if (tables->wide) rc = index_bytes == 1 ? launch_with_lds(indexed_encode_kernel<KIND, uint8_t, true>, blocks, kBlock, lds, a, hs)
                                            : launch_with_lds(indexed_encode_kernel<KIND, int32_t, true>, blocks, kBlock, lds, a, hs);
    else rc = index_bytes == 1 ? launch_with_lds(indexed_encode_kernel<KIND, uint8_t, false>, blocks, kBlock, lds, a, hs)
                               : launch_with_lds(indexed_encode_kernel<KIND, int32_t, false>, blocks, kBlock, lds, a, hs);
    return note_kernel(kIxNames[KIND == kRange][0], rc);
}

template <int KIND>
static cst_status decode_indexed(const cst_table_set* tables, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets,
                                 size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices, int32_t index_bytes,
                                 int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t* d_state,
                                 uint32_t* d_n_words_out, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_indexed_args(tables, cfg, d_symbols, d_indices, index_bytes, n_per_stream, layout, d_words, d_n_words, d_status, flags))
        return st;
    if (n_streams == 0) return CST_OK;
    if (cst_status st = check_indexed_device(tables, n_streams)) return st;
    IndexedDecodeArgs a{};
    a.image = tables->d_image; a.rows_bytes = tables->rows_bytes; a.image_bytes = tables->image_bytes;
    a.pitch = tables->pitch; a.n_symbols = tables->n_symbols; a.n_tables = tables->n_tables; a.min_symbol = tables->min_symbol;
    a.precision = tables->precision; a.bucket_bits = tables->bucket_bits; a.bucket_wide = tables->bucket_wide;
    a.words = d_words; a.offsets = d_offsets; a.stride_words = stride_words; a.words_capacity = words_capacity; a.n_words = d_n_words;
    a.indices = d_indices; a.symbols = d_symbols; a.n_streams = n_streams; a.n_per_stream = n_per_stream;
    a.state = d_state; a.n_words_out = d_n_words_out; a.rstate = d_rstate; a.status = d_status;
    const size_t blocks = (n_streams + kBlock - 1) / kBlock, lds = kIxFixedLds + tables->image_bytes;
    cst_status rc;
    if (tables->wide) rc = index_bytes == 1 ? launch_with_lds(indexed_decode_kernel<KIND, uint8_t, true>, blocks, kBlock, lds, a, hs)
                                            : launch_with_lds(indexed_decode_kernel<KIND, int32_t, true>, blocks, kBlock, lds, a, hs);
    else rc = index_bytes == 1 ? launch_with_lds(indexed_decode_kernel<KIND, uint8_t, false>, blocks, kBlock, lds, a, hs)
                               : launch_with_lds(indexed_decode_kernel<KIND, int32_t, false>, blocks, kBlock, lds, a, hs);
    return note_kernel(kIxNames[KIND == kRange][1], rc);
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_table_set_create(int32_t precision, int32_t min_symbol, int32_t n_symbols, int32_t n_tables, const uint32_t* h_cdfs,
                                void** out) {
    if (!out || !h_cdfs) return CST_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (precision < 1 || precision > 24 || n_tables < 1 || n_tables > 256) return CST_ERR_INVALID_ARGUMENT;
    // (the rules of cst_model_create_table from here on)
    if (n_symbols < 2 || (int64_t)n_symbols > ((int64_t)1 << precision) || n_symbols > 65536) return CST_ERR_MODEL;
    if ((int64_t)min_symbol + n_symbols - 1 > INT32_MAX) return CST_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)n_symbols, K = (size_t)n_tables, pitch = n + 1;
    for (size_t k = 0; k < K; ++k)
        if (!cdf_valid(h_cdfs + k * pitch, n_symbols, precision)) return CST_ERR_MODEL;
    // the image: rows, then the largest bucket index that still fits beside them
    const bool wide = precision > 16, bucket_wide = n_symbols > 256;
    const size_t rows_bytes = (K * pitch * (wide ? 4 : 2) + 15) & ~(size_t)15;
    const int most_bits = knobs().indexed_bucket_bits < 0 ? 0 : knobs().indexed_bucket_bits < kIxMaxBucketBits ? knobs().indexed_bucket_bits : kIxMaxBucketBits;
    int bucket_bits = precision < most_bits ? precision : most_bits;
    size_t bucket_bytes = 0;
    for (;; --bucket_bits) {
        if (bucket_bits < 0) return CST_ERR_MODEL;              // does not fit beside the rings and tiles
        bucket_bytes = (K * (((size_t)1 << bucket_bits) + 1) * (bucket_wide ? 2 : 1) + 15) & ~(size_t)15;
        if (rows_bytes + bucket_bytes <= kIxMaxImage) break;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return CST_ERR_NO_DEVICE;

    std::vector<unsigned char> image(rows_bytes + bucket_bytes, 0);
    const size_t nb = (size_t)1 << bucket_bits;
    const int shift = precision - bucket_bits;
    for (size_t k = 0; k < K; ++k) {
        const uint32_t* cdf = h_cdfs + k * pitch;
        for (size_t i = 0; i <= n; ++i) {
            if (wide) reinterpret_cast<uint32_t*>(image.data())[k * pitch + i] = cdf[i];
            else reinterpret_cast<uint16_t*>(image.data())[k * pitch + i] = (uint16_t)cdf[i];       // (2^16 is stored as 0)
        }
        size_t i = 0;
        for (size_t b = 0; b <= nb; ++b) {
            const uint64_t q = (uint64_t)b << shift;
            while (i + 1 < n && cdf[i + 1] <= q) ++i;           // (entry nb: the last symbol)
            const size_t at = k * (nb + 1) + b;
            if (bucket_wide) reinterpret_cast<uint16_t*>(image.data() + rows_bytes)[at] = (uint16_t)i;
            else image[rows_bytes + at] = (unsigned char)i;
        }
    }
    cst_table_set* t = new (std::nothrow) cst_table_set();
    if (!t) return CST_ERR_OUT_OF_MEMORY;
    t->precision = precision; t->min_symbol = min_symbol; t->n_symbols = n_symbols; t->n_tables = n_tables;
    t->pitch = (int32_t)pitch; t->wide = wide; t->bucket_bits = bucket_bits; t->bucket_wide = bucket_wide;
    t->rows_bytes = (uint32_t)rows_bytes; t->image_bytes = (uint32_t)image.size();
    hipGetDevice(&t->device);
    hipError_t e = hipMalloc(&t->d_image, image.size());
    if (e == hipSuccess) e = hipMemcpy(t->d_image, image.data(), image.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_hip_error(e, "table set upload");
        if (t->d_image) (void)hipFree(t->d_image);
        delete t;
        return CST_ERR_HIP;
    }
    t->magic = kIxMagic;
    *out = t;
    return CST_OK;
}

cst_status cst_table_set_destroy(void* handle) {
    cst_table_set* tables = reinterpret_cast<cst_table_set*>(handle);
    if (!tables) return CST_OK;
    if (!table_set_alive(tables)) return CST_ERR_INVALID_ARGUMENT;
    tables->magic = 0;
    if (tables->d_image) (void)hipFree(tables->d_image);
    delete tables;
    return CST_OK;
}

int32_t cst_table_set_precision(const void* tables) { return table_set_alive(as_table_set(tables)) ? as_table_set(tables)->precision : 0; }
int32_t cst_table_set_min_symbol(const void* tables) { return table_set_alive(as_table_set(tables)) ? as_table_set(tables)->min_symbol : 0; }
int32_t cst_table_set_n_symbols(const void* tables) { return table_set_alive(as_table_set(tables)) ? as_table_set(tables)->n_symbols : 0; }
int32_t cst_table_set_n_tables(const void* tables) { return table_set_alive(as_table_set(tables)) ? as_table_set(tables)->n_tables : 0; }

cst_status cst_ans_encode_indexed_batch(const void* tables, cst_coder_config cfg, const int32_t* d_symbols, const void* d_indices,
                                        int32_t index_bytes, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                        size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status, uint32_t flags,
                                        void* stream) {
    return encode_indexed<kAns>(as_table_set(tables), cfg, d_symbols, d_indices, index_bytes, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words,
                                d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_encode_indexed_batch(const void* tables, cst_coder_config cfg, const int32_t* d_symbols, const void* d_indices,
                                          int32_t index_bytes, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                          size_t stride_words, uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags,
                                          void* stream) {
    return encode_indexed<kRange>(as_table_set(tables), cfg, d_symbols, d_indices, index_bytes, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words,
                                  nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

cst_status cst_ans_decode_indexed_batch(const void* tables, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets,
                                        size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                        int32_t index_bytes, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                        uint64_t* d_state, uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_indexed<kAns>(as_table_set(tables), cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_indices, index_bytes, d_symbols, n_streams,
                                n_per_stream, layout, d_state, d_n_words_out, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_decode_indexed_batch(const void* tables, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets,
                                          size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const void* d_indices,
                                          int32_t index_bytes, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                          cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_indexed<kRange>(as_table_set(tables), cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_indices, index_bytes, d_symbols,
                                  n_streams, n_per_stream, layout, nullptr, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

} // extern "C"
