// cst_range_ps.hip -- batched range coder with ONE MODEL PER STREAM (config C3's tables under config C4's coder): every
// lane codes its stream as a queue with its own 16-bit cdf row.
//
// The rows, their staging and the decoder's search are those of the per-stream ANS coder (cst_per_stream_rows.hpp: rows
// transposed per wave in LDS, a 64-bucket index where 6 <= P <= 15, a branch-free 4-ary search); the coder steps are the
// model-agnostic ones of cst_range_kernels.hpp (RangeEncLane::step(c, p, P), RangeDecLane::peek_quantile / advance).  The
// range encoder needs (c, p) = (row[i], row[i+1] - row[i]) only: no reciprocal table.  Words are written and read front to
// back through the per-lane LDS rings.  Presets (32,64) and (16,32), P <= 16 (what a 16-bit row holds).
//
// Jump points (RangeEncoder::pos / RangeDecoder::seek, queue.rs:172-196, 911-926): the encoder's <ckpt> form notes
// (words so far, lower, range) in front of every chunk; the decoder's <chunks> form runs over virtual streams
// v = (stream v / k, chunk v % k) and continues each at its jump point.  A stream's row is staged once per chunk lane.
#include "cst_range_kernels.hpp"
#include "cst_per_stream_rows.hpp"

namespace cst {

struct RangePsArgs {
    const int32_t* symbols_in;
    int32_t* symbols_out;
    size_t n_streams, n_per_stream;   // lanes with work, symbols per lane (<chunks>: virtual streams, symbols per chunk)
    int32_t layout, precision, n_symbols, min_symbol;
    const uint16_t* cdf16;            // [n_tables][L]
    int32_t L;                        // row length (power of two)
    uint32_t* words_out;
    const uint32_t* words_in;
    const uint64_t* offsets;
    size_t stride_words;
    uint32_t* n_words_out;
    const uint32_t* n_words_in;
    int32_t* status;
    uint64_t words_capacity;          // decode: uint32 slots behind `words_in` (0 = unknown): see word_slice
    RangeCkptOut ck;                  // encode <ckpt>: [n_streams][n_chunks]
    const uint32_t* ckpt_pos;         // decode <chunks>: [n_streams / n_chunks][n_chunks]
    const uint64_t* ckpt_lower;
    const uint64_t* ckpt_range;
    size_t n_chunks;
};

template <int W, int S, bool CKPT>
__global__ __launch_bounds__(kBlock) void range_encode_ps_kernel(const RangePsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_in_block = threadIdx.x >> 6;
    const size_t block_s0 = (size_t)blockIdx.x * blockDim.x;
    uint16_t* rows = reinterpret_cast<uint16_t*>(smem);
    const size_t rows_bytes = (size_t)blockDim.x * a.L * 2;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem + rows_bytes) + wave_in_block * kRingWords;
    int32_t* tile = reinterpret_cast<int32_t*>(smem + rows_bytes + (size_t)(blockDim.x / kWave) * kRingWords * 4) + wave_in_block * (kWave * kTileStride);
    stage_rows(rows, a, block_s0);
    __syncthreads();

    const size_t s0 = block_s0 + (size_t)wave_in_block * kWave;
    if (s0 >= a.n_streams) return;
    const size_t s = s0 + lane;
    const bool active = s < a.n_streams;     // (a lane without a stream codes min_symbol into a slab of no words)
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const uint32_t nsym = (uint32_t)a.n_symbols;
    const int G = groups_per_point(W, P);
    LaneRow R{rows + (size_t)wave_in_block * a.L * kWave + lane};

    RangeEncLane<W, S> L;
    L.init(a.words_out + (active ? s : 0) * a.stride_words,
           active ? (uint32_t)(a.stride_words > 0xffffffffull ? 0xffffffffull : a.stride_words) : 0u, ring, lane);

    struct CP { uint32_t c, p; };
    auto entry = [&](int32_t v) {
        const uint32_t i = enc_index(v, a.min_symbol, nsym, L.bad);
        const uint32_t c = R.at(i);
        return CP{c, (R.at(i + 1) - c) & 0xffffu};      // (P = 16: the row stores 2^16 as 0)
    };
    int countdown = 4 * G;
    size_t until_point = 0, chunk = 0;                  // <ckpt>: symbols until the next jump point, its number
    auto note_if_due = [&]() {                          // RangeEncoder::pos() in front of a chunk, queue.rs:182-196
        if (until_point == 0) {
            if (active) {
                const size_t k = s * a.ck.n_chunks + chunk;
                a.ck.pos[k] = L.out.wr + L.inv_n; a.ck.lower[k] = (uint64_t)L.lower; a.ck.range[k] = (uint64_t)L.range;
            }
            ++chunk;
            until_point = a.ck.interval;
        }
    };
    auto code = [&](int32_t v) {
        if constexpr (CKPT) { note_if_due(); --until_point; }
        const CP e = entry(v);
        L.step(e.c, e.p, P);
        if (--countdown == 0) { countdown = 4 * G; L.out.flush_chunks(); }
    };

    if (a.layout == CST_LAYOUT_SYMBOL_MAJOR) {
        // four symbols per request, one group ahead of their use (as range_encode_kernel reads its column)
        const int32_t* col = a.symbols_in + (active ? s : 0);
        size_t t = 0;
        int32_t nxt[4] = {a.min_symbol, a.min_symbol, a.min_symbol, a.min_symbol};
        if (N >= 4 && active) {
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[j] = col[(size_t)j * a.n_streams];
        }
        for (; t + 4 <= N; t += 4) {
            int32_t cur[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
            if (t + 8 <= N && active) {
#pragma unroll
                for (int j = 0; j < 4; ++j) nxt[j] = col[(t + 4 + j) * a.n_streams];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) code(cur[j]);
        }
        for (; t < N; ++t) code(active ? col[t * a.n_streams] : a.min_symbol);
    } else {
        // whole 32-symbol tiles through the wave's LDS tile (16-byte row chunks where N % 4 == 0 and the base is aligned,
        // words otherwise), then the tail of the rows one symbol at a time
        const int32_t* row = a.symbols_in + (active ? s : 0) * N;
        const bool vec = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.symbols_in) & 15) == 0);
        const size_t n_full = N / kTileSyms;
        if (n_full > 0) {
            int32_t r[kTileSyms];
            auto fetch = [&](size_t t0) {
                if (vec) tile_fetch<true>(a.symbols_in, a.n_streams, N, s0, t0, lane, r);
                else tile_fetch<false>(a.symbols_in, a.n_streams, N, s0, t0, lane, r);
            };
            fetch(0);
            const int32_t* my = tile + lane * kTileStride;
            for (size_t tb = 0; tb < n_full; ++tb) {
                wave_lds_fence();
                if (vec) tile_to_lds<true>(tile, lane, r);
                else tile_to_lds<false>(tile, lane, r);
                wave_lds_fence();
                if (tb + 1 < n_full) fetch((tb + 1) * kTileSyms);
                for (int j = 0; j < kTileSyms / 4; ++j) {
                    int4 v = *reinterpret_cast<const int4*>(my + 4 * j);
                    if (!active) v = make_int4(a.min_symbol, a.min_symbol, a.min_symbol, a.min_symbol);
                    // <ckpt>: a quad with a jump point inside it goes symbol by symbol (wave-uniform: the points depend on t alone)
                    bool whole_quad = true;
                    if constexpr (CKPT) {
                        note_if_due();
                        whole_quad = until_point >= 4;
                    }
                    if (whole_quad) {
                        // the branch-free step; a quad in which some lane leaves a long Inverted run is rolled back and
                        // repeated with the general step (rare), as in range_encode_kernel
                        const CP e0 = entry(v.x), e1 = entry(v.y), e2 = entry(v.z), e3 = entry(v.w);
                        const auto lower0 = L.lower, range0 = L.range;
                        const uint32_t wr0 = L.out.wr, inv_n0 = L.inv_n, inv_first0 = L.inv_first;
                        bool slow = false;
                        L.step_inline(e0.c, e0.p, P, slow); L.step_inline(e1.c, e1.p, P, slow);
                        L.step_inline(e2.c, e2.p, P, slow); L.step_inline(e3.c, e3.p, P, slow);
                        if (__any(slow)) {
                            L.lower = lower0; L.range = range0; L.out.wr = wr0; L.inv_n = inv_n0; L.inv_first = inv_first0;
                            L.step(e0.c, e0.p, P); L.step(e1.c, e1.p, P); L.step(e2.c, e2.p, P); L.step(e3.c, e3.p, P);
                        }
                        if constexpr (CKPT) until_point -= 4;
                    } else {
                        code(v.x); code(v.y); code(v.z); code(v.w);
                    }
                    if ((j + 1) % G == 0) L.out.flush_chunks();     // (every G quads whichever way they went; code() adds its own points)
                }
            }
        }
        for (size_t t = n_full * kTileSyms; t < N; ++t) code(active ? row[t] : a.min_symbol);
    }

    uint32_t n_words = 0;
    const int32_t status = L.finish(nsym, n_words);
    if (!active) return;
    a.status[s] = status;
    a.n_words_out[s] = (status == CST_STREAM_OK) ? n_words : 0u;
}

template <int W, int S, bool CHUNKS>
__global__ __launch_bounds__(kBlock) void range_decode_ps_kernel(const RangePsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using st_t = typename StateT<S>::type;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_in_block = threadIdx.x >> 6;
    const size_t block_s0 = (size_t)blockIdx.x * blockDim.x;
    const int P = a.precision;
    const bool indexed = ps_indexed(P);
    uint16_t* rows = reinterpret_cast<uint16_t*>(smem);
    const size_t rows_bytes = (size_t)blockDim.x * a.L * 2;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem + rows_bytes) + wave_in_block * kRingWords;
    uint16_t* bidx = reinterpret_cast<uint16_t*>(smem + rows_bytes + (size_t)(blockDim.x / kWave) * kRingWords * 4) +
                     (size_t)wave_in_block * kPsIdxStride * kWave + lane;           // [wave][bucket][lane]
    stage_rows(rows, a, block_s0, indexed, CHUNKS ? a.n_chunks : (size_t)1);
    __syncthreads();

    if (block_s0 + (size_t)wave_in_block * kWave >= a.n_streams) return;
    const size_t v = block_s0 + threadIdx.x;            // this lane's (virtual) stream
    const bool active = v < a.n_streams;
    const size_t s = CHUNKS ? (active ? v / a.n_chunks : 0) : v;
    const size_t N = a.n_per_stream;
    const uint32_t n = (uint32_t)a.n_symbols;
    const int G4 = 4 * groups_per_point(W, P);
    LaneRow R{rows + (size_t)wave_in_block * a.L * kWave + lane};

    RangeDecLane<W, S> L;
    const WordSlice ws = active ? word_slice(a.offsets, a.stride_words, a.n_words_in, s, a.words_capacity) : WordSlice{0, 0u, false};
    bool bad = ws.bad;
    uint32_t pos0 = 0;
    st_t lower0 = 0, range0 = (st_t)~(st_t)0;           // RangeCoderState::default: from_compressed is seek(0, default)
    if (CHUNKS && active) {
        pos0 = a.ckpt_pos[v]; lower0 = (st_t)a.ckpt_lower[v]; range0 = (st_t)a.ckpt_range[v];
        bad = bad || pos0 > ws.n;                       // a jump point beyond its stream's words: caller data gone wrong
    }
    L.init_at(a.words_in + ws.off, ws.n, pos0, lower0, range0, ring, lane);
    L.in.prime();
    wave_lds_fence();
    if (indexed) ps_build_bucket_index(R, bidx, P, n);

    auto decode_one = [&]() -> int32_t {
        const uint32_t q = L.peek_quantile(P);
        const uint32_t next_word = L.in.peek();
        const uint32_t i = ps_search(R, bidx, indexed, q, P, n);
        const uint32_t c = R.at(i);
        const uint32_t p = (R.at(i + 1) - c) & 0xffffu;
        L.in.pos += L.advance(c, p, P, next_word, L.in.pos < L.in.len) ? 1u : 0u;
        return a.min_symbol + (int32_t)i;
    };

    const size_t stride_t = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? a.n_streams : 1;
    int32_t* my = a.symbols_out + (active ? (a.layout == CST_LAYOUT_SYMBOL_MAJOR ? v : v * N) : 0);
    const bool vec = a.layout == CST_LAYOUT_STREAM_MAJOR && (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.symbols_out) & 15) == 0);
    // Symbols leave 16 bytes per lane per four steps, not through an LDS tile: the per-stream ANS decoder measured the tile
    // 1.7x slower (it costs a wave of occupancy, and the kernel is bound by the latency of its row search, not by HBM), and
    // this decoder has the same rows and search plus the quotient in front of them.
    int countdown = G4;
    size_t t = 0;
    if (vec) {
        for (; t + 4 <= N; t += 4) {
            int4 o;
            o.x = decode_one(); o.y = decode_one(); o.z = decode_one(); o.w = decode_one();
            if (active) *reinterpret_cast<int4*>(my + t) = o;
            countdown -= 4;
            if (countdown <= 0) { countdown = G4; L.in.advance_window(); }
        }
    }
    for (; t < N; ++t) {
        const int32_t o = decode_one();
        if (active) my[t * stride_t] = o;
        if (--countdown <= 0) { countdown = G4; L.in.advance_window(); }
    }
    if (!active) return;
    a.status[v] = bad ? (int32_t)CST_STREAM_INVALID_DATA : L.status;
}

static bool range_ps_model_ok(const cst_model* model, cst_coder_config cfg, size_t n_streams) {
    return model->per_stream && model->n_tables == n_streams && model->d_cdf16 && model->precision <= 16 &&
           ((cfg.word_bits == 32 && cfg.state_bits == 64) || (cfg.word_bits == 16 && cfg.state_bits == 32));
}

static RangePsArgs range_ps_args(const cst_model* model, size_t n_streams, size_t n_per_stream, cst_layout layout, int32_t* d_status) {
    RangePsArgs a{};
    a.n_streams = n_streams; a.n_per_stream = n_per_stream; a.layout = layout; a.precision = model->precision;
    a.n_symbols = model->n_symbols; a.min_symbol = model->min_symbol; a.cdf16 = model->d_cdf16; a.L = model->cdf16_stride;
    a.status = d_status; a.n_chunks = 1;
    return a;
}

cst_status range_encode_per_stream(const cst_model* model, cst_coder_config cfg, const int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                   cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, int32_t* d_status,
                                   const RangeCkptOut* ck, hipStream_t hs) {
    if (!range_ps_model_ok(model, cfg, n_streams)) return CST_ERR_INVALID_ARGUMENT;
    if (ck && layout != CST_LAYOUT_STREAM_MAJOR) return CST_ERR_INVALID_ARGUMENT;
    RangePsArgs a = range_ps_args(model, n_streams, n_per_stream, layout, d_status);
    a.symbols_in = d_symbols; a.words_out = d_words; a.stride_words = stride_words; a.n_words_out = d_n_words;
    if (ck) {
        a.ck = *ck;
        if (cfg.word_bits == 32) return launch_ps(range_encode_ps_kernel<32, 64, true>, a, true, hs);
        return launch_ps(range_encode_ps_kernel<16, 32, true>, a, true, hs);
    }
    if (cfg.word_bits == 32) return launch_ps(range_encode_ps_kernel<32, 64, false>, a, true, hs);
    return launch_ps(range_encode_ps_kernel<16, 32, false>, a, true, hs);
}

// interval == 0: one lane per stream; otherwise n_per_stream / interval lanes per stream, each continued at its jump point
// (d_status then has one entry per chunk)
cst_status range_decode_per_stream(const cst_model* model, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                   size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                   cst_layout layout, int32_t* d_status, size_t interval, const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_lower,
                                   const uint64_t* d_ckpt_range, hipStream_t hs) {
    if (!range_ps_model_ok(model, cfg, n_streams)) return CST_ERR_INVALID_ARGUMENT;
    RangePsArgs a = range_ps_args(model, n_streams, n_per_stream, layout, d_status);
    a.symbols_out = d_symbols; a.words_in = d_words; a.offsets = d_offsets; a.stride_words = stride_words; a.n_words_in = d_n_words;
    a.words_capacity = words_capacity;
    if (interval == 0) {
        if (cfg.word_bits == 32) return launch_ps(range_decode_ps_kernel<32, 64, false>, a, false, hs);
        return launch_ps(range_decode_ps_kernel<16, 32, false>, a, false, hs);
    }
    if (layout != CST_LAYOUT_STREAM_MAJOR || n_per_stream % interval != 0) return CST_ERR_INVALID_ARGUMENT;
    a.n_chunks = n_per_stream / interval;
    if (a.n_chunks == 0 || n_streams > 0x7fffffffull / a.n_chunks) return CST_ERR_INVALID_ARGUMENT;
    a.n_streams = n_streams * a.n_chunks; a.n_per_stream = interval;      // the virtual streams: rows of `interval` symbols
    a.ckpt_pos = d_ckpt_pos; a.ckpt_lower = d_ckpt_lower; a.ckpt_range = d_ckpt_range;
    if (cfg.word_bits == 32) return launch_ps(range_decode_ps_kernel<32, 64, true>, a, false, hs);
    return launch_ps(range_decode_ps_kernel<16, 32, true>, a, false, hs);
}

} // namespace cst
