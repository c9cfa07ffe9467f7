// cst_persymbol_categorical.hip -- per-symbol Categorical models given as matrices of floating-point probabilities
// (cst_persymbol.hpp has the map of the per-symbol files): the kernels of the fast quantiser, Categorical(perfect=False), and the
// host paths of both quantisers -- Categorical(perfect=True) is quantised by categorical_perfect_kernel (cst_categorical_perfect.hip).
// Pass 2 of the encoders and the rows-in-pieces decoders are cst_persymbol.hip's; the row tile and categorical_entries_kernel are in
// cst_persymbol_categorical.hpp, shared with the ragged forms (cst_persymbol_categorical_ragged.hip).
#include "cst_persymbol.hpp"
#include "cst_categorical.hpp"
#include "cst_persymbol_categorical.hpp"
#include "cst_categorical_perfect.hpp"

// ------------------------------------------------------------------------------------------------
// Per-symbol Categorical models given as a matrix of floating-point probabilities: the reference's
//   coder.encode_reverse(symbols, Categorical(perfect=False), probabilities) / coder.decode(Categorical(lazy=True), probabilities)
// (src/pybindings/stream/model/internals.rs:399-514) with one probability vector of K entries per coded symbol.  The table of a
// row comes from ONE sequential sum in the dtype of the input (cst_categorical.hpp), so one LANE walks a row, and the parallelism
// is rows side by side: a wave owns 64 rows, loads them together -- coalesced, in chunks of kCatChunk columns -- into a
// wave-private LDS tile, and every lane then walks its own row of the tile in order.  The running sum is carried across the
// chunks, so any 2 <= K < 2^P - 1 goes through the same code.
//   categorical_entries_kernel      encoder pass 1: one walk picks up the sums at `symbol` and `symbol + 1` and the total
//   categorical_rows_kernel         the whole quantised row (tabulation; the rows-in-pieces route of few-stream decodes)
//   decode_categorical_lane_kernel  one lane per stream: a walk for the normalisation, a second one until right > quantile
// One wave per workgroup: a workgroup's LDS is its wave's tile, and few waves still spread over the chip.
// ------------------------------------------------------------------------------------------------
namespace cst {

// a left cumulative parked in the tile slot of the entry it belongs to (f32: its bits; f64: its value, exact)
__device__ __forceinline__ float cat_park(uint32_t v, float) { return __uint_as_float(v); }
__device__ __forceinline__ double cat_park(uint32_t v, double) { return (double)v; }
__device__ __forceinline__ uint32_t cat_parked(float f) { return __float_as_uint(f); }
__device__ __forceinline__ uint32_t cat_parked(double f) { return (uint32_t)f; }

// Output row o = s * count + (t - t0) <- the probabilities of (stream s, position t), t0 <= t < t0 + count; a wave takes 64
// positions of one stream.  A row is `pitch` >= K + 1 words: the K left cumulatives, then 2^P up to the pitch (the 256-entry rows
// of decode_rows_wave_kernel).  A bad model's row is 0xffffffff followed by 2^P -- no quantile lies in it -- and bad[o] = 1.
struct CatRowsArgs {
    const void* probs;
    uint32_t K; int32_t P, layout;
    size_t n_streams, N, t0, count;
    uint32_t* rows; size_t pitch;
    int32_t* bad;               // or null
};

template <class F>
__global__ __launch_bounds__(kWave) void categorical_rows_kernel(const CatRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    F* tile = reinterpret_cast<F*>(smem);
    const F* probs = reinterpret_cast<const F*>(a.probs);
    const int lane = threadIdx.x;
    const size_t K = a.K;
    const size_t blocks_per_stream = (a.count + kWave - 1) / kWave;
    const size_t s = (size_t)blockIdx.x / blocks_per_stream, tb = ((size_t)blockIdx.x % blocks_per_stream) * kWave;
    if (s >= a.n_streams) return;
    const int n_rows = (int)(a.count - tb < (size_t)kWave ? a.count - tb : (size_t)kWave);
    const bool symbol_major = a.layout == CST_LAYOUT_SYMBOL_MAJOR;
    const size_t first = symbol_major ? (a.t0 + tb) * a.n_streams + s : s * a.N + a.t0 + tb, step = symbol_major ? a.n_streams : 1;
    const size_t o0 = s * a.count + tb;
    const bool vec = cat_vec_ok(probs, K);
    const uint32_t total = 1u << a.P;
    F* my = tile + lane * kCatPitch;

    CatSum<F> sum;
    for (size_t c0 = 0; c0 < K; c0 += kCatChunk) {
        const int n_here = (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk);
        wave_lds_fence();
        cat_stage(tile, probs, first, step, n_rows, K, c0, n_here, vec, lane);
        wave_lds_fence();
#pragma unroll 8
        for (int j = 0; j < n_here; ++j) sum.add(my[j]);
    }
    const bool bad = sum.bad();
    const unsigned long long bad_rows = __ballot(bad);
    if (a.bad && lane < n_rows) a.bad[o0 + lane] = bad ? 1 : 0;
    const F scale = cat_scale<F>(a.P, (uint32_t)K, bad ? F(1) : sum.cum);

    // second walk: every left cumulative, parked where its entry was; then the chunk leaves row by row, a column per lane
    F cum = F(0);
    for (size_t c0 = 0; c0 < a.pitch; c0 += kCatChunk) {
        const int n_here = c0 < K ? (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk) : 0;
        if (n_here > 0) {
            wave_lds_fence();                                           // (the previous chunk has been stored)
            if (K > (size_t)kCatChunk) cat_stage(tile, probs, first, step, n_rows, K, c0, n_here, vec, lane);    // (else: still there)
            wave_lds_fence();
#pragma unroll 8
            for (int j = 0; j < n_here; ++j) {
                const F p = my[j];
                my[j] = cat_park(cat_left<F>(cum, scale, (uint32_t)c0 + (uint32_t)j), F(0));
                cum = cum + p;
            }
            wave_lds_fence();
        }
        const size_t col = c0 + (size_t)lane;
        if (col < a.pitch) {
#pragma unroll 8
            for (int r = 0; r < n_rows; ++r) {
                uint32_t v = col < K ? cat_parked(tile[r * kCatPitch + lane]) : total;
                if ((bad_rows >> r) & 1ull) v = col == 0 ? 0xffffffffu : total;
                a.rows[(o0 + (size_t)r) * a.pitch + col] = v;
            }
        }
    }
}

struct CatDecodeArgs {
    PerSymbolDecodeArgs a;      // min_symbol = 0, n_symbols = K
    const void* probs;          // [the symbols' shape][K]
};

// One LANE per stream, 64 streams per wave, in the geometry of the Gaussian lane decoder: for every position the wave stages its
// streams' 64 rows (contiguous memory in symbol-major layout) and every lane walks its own.  The first walk gives the
// normalisation.  The second goes from the start until right > quantile, and the last symbol is the fall-through
// (lazy_contiguous.rs:300-330).  A row of at most kCatChunk entries is staged once for both walks; a longer one is streamed twice,
// the second time only as far as the slowest lane of the wave has to look.
template <int W, int S, int KIND, class F>
__global__ __launch_bounds__(kWave) void decode_categorical_lane_kernel(const CatDecodeArgs ca) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    F* tile = reinterpret_cast<F*>(smem);
    const PerSymbolDecodeArgs& a = ca.a;
    const F* probs = reinterpret_cast<const F*>(ca.probs);
    const int lane = threadIdx.x;
    const size_t s0 = (size_t)blockIdx.x * kWave, s = s0 + lane;
    if (s0 >= a.n_streams) return;
    const int n_rows = (int)(a.n_streams - s0 < (size_t)kWave ? a.n_streams - s0 : (size_t)kWave);
    const bool active = lane < n_rows;
    const size_t se = active ? s : a.n_streams - 1;          // idle lanes of a partial wave repeat its last stream (and write nothing)
    const size_t N = a.n_per_stream, K = (size_t)a.n_symbols;
    const int P = a.precision;
    const uint32_t total = 1u << P;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const bool symbol_major = a.layout == CST_LAYOUT_SYMBOL_MAJOR;
    const bool vec = cat_vec_ok(probs, K);
    const F* my = tile + lane * kCatPitch;

    DirectDecoder<W, S, KIND> D;
    D.init(a, se, raw);
    int32_t status = D.status;
    for (size_t t = 0; t < N; ++t) {
        if (!__any(active && status == CST_STREAM_OK)) break;           // (what follows a failure is unspecified)
        const size_t first = symbol_major ? t * a.n_streams + s0 : s0 * N + t, step = symbol_major ? 1 : N;
        CatSum<F> sum;
        for (size_t c0 = 0; c0 < K; c0 += kCatChunk) {
            const int n_here = (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk);
            wave_lds_fence();
            cat_stage(tile, probs, first, step, n_rows, K, c0, n_here, vec, lane);
            wave_lds_fence();
#pragma unroll 8
            for (int j = 0; j < n_here; ++j) sum.add(my[j]);
        }
        bool search = status == CST_STREAM_OK;
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
                cat_stage(tile, probs, first, step, n_rows, K, c0, (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk), vec, lane);
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
        if (active) a.symbols[symbol_major ? t * a.n_streams + s : s * N + t] = decoded;
    }
    if (!active) return;
    a.status[s] = status;
    D.finish(a, s, raw);
}

// ---- host side ----
// everything that can be said about the arguments without the device, the same for all eight coder calls
static cst_status check_categorical_args(cst_coder_config cfg, cst_layout layout, const void* d_symbols, const void* d_probs, int32_t prob_bytes,
                                         int32_t n_symbols, bool perfect, const void* d_words, const void* d_n_words, const void* d_status,
                                         const void* raw_state, uint32_t flags) {
    if (!d_symbols || !d_probs || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (prob_bytes != 4 && prob_bytes != 8) return CST_ERR_INVALID_ARGUMENT;
    if ((flags & CST_FLAG_RAW_STATE) && !raw_state) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_common(cfg, layout)) return st;
    // the largest support.  from_floating_point_probabilities_fast: room for a nonzero probability each plus one;
    // perfectly_quantized_probabilities: a unit of weight for each, and the kernel's slots
    const uint64_t total = (uint64_t)1 << cfg.precision;
    const uint64_t limit = !perfect ? total - 2 : total < (uint64_t)kCatPerfectMaxK ? total : (uint64_t)kCatPerfectMaxK;
    if (n_symbols < 2 || (uint64_t)n_symbols > limit) return CST_ERR_MODEL;
    return CST_OK;
}

static cst_status launch_categorical_rows(const CatRowsArgs& r, int32_t prob_bytes, hipStream_t hs) {
    const size_t blocks = r.n_streams * ((r.count + kWave - 1) / kWave);
    if (blocks == 0) return CST_OK;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (prob_bytes == 4) hipLaunchKernelGGL(categorical_rows_kernel<float>, dim3((unsigned)blocks), dim3(kWave), kCatTileBytes<float>, hs, r);
    else hipLaunchKernelGGL(categorical_rows_kernel<double>, dim3((unsigned)blocks), dim3(kWave), kCatTileBytes<double>, hs, r);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

static constexpr const char* kCatEncodeNames[2] = {"ans_encode_categorical_two_pass", "range_encode_categorical_two_pass"};
static constexpr const char* kCatLaneNames[2] = {"ans_decode_categorical_lane_kernel", "range_decode_categorical_lane_kernel"};
static constexpr const char* kCatRowsName = "decode_categorical_by_rows";

template <int KIND>
static cst_status encode_categorical(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                     size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                                     uint32_t* d_n_words, uint64_t* d_state, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags,
                                     hipStream_t hs) {
    if (cst_status st = check_categorical_args(cfg, layout, d_symbols, d_probs, prob_bytes, n_symbols, false, d_words, d_n_words, d_status,
                                               KIND == kAns ? (const void*)d_state : (const void*)d_rstate, flags)) return st;
    if ((n_streams * n_per_stream + kWave - 1) / kWave > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    note_kernel(kCatEncodeNames[KIND == kRange], CST_OK);
    return encode_two_pass<KIND>(cfg, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words, d_state, d_rstate, d_status, flags, hs,
                                 [&](EncEntry* out, size_t n) {
        const dim3 grid((unsigned)((n + kWave - 1) / kWave));
        if (prob_bytes == 4)
            hipLaunchKernelGGL(categorical_entries_kernel<float>, grid, dim3(kWave), kCatTileBytes<float>, hs, cfg.precision, (uint32_t)n_symbols,
                               d_symbols, reinterpret_cast<const float*>(d_probs), n, out);
        else
            hipLaunchKernelGGL(categorical_entries_kernel<double>, grid, dim3(kWave), kCatTileBytes<double>, hs, cfg.precision, (uint32_t)n_symbols,
                               d_symbols, reinterpret_cast<const double*>(d_probs), n, out);
    });
}

// few streams (one long stream is the drop-in coder's case): the rows at full occupancy, then a lookup per symbol, in pieces of at
// most 64 MiB of rows (K < 256: decode_rows_wave_kernel's 256-entry rows, at least 64 positions a piece; longer rows: K + 1 words)
template <int KIND>
static cst_status decode_categorical_by_rows(cst_coder_config cfg, const PerSymbolDecodeArgs& a, const void* d_probs, int32_t prob_bytes,
                                             hipStream_t hs) {
    const size_t N = a.n_per_stream, K = (size_t)a.n_symbols;
    const bool packed = K < (size_t)kRowEntries;
    const size_t pitch = packed ? (size_t)kRowEntries : K + 1;
    size_t piece = ((size_t)16 << 20) / (a.n_streams * pitch);
    if (piece >= 64) piece &= ~(size_t)63;
    else piece = packed ? 64 : (piece ? piece : 1);
    if (piece > N) piece = N;
    return decode_in_pieces<KIND>(cfg, a, packed, pitch, piece, [&](size_t t0, size_t count, uint32_t* rows) -> cst_status {
        CatRowsArgs r{d_probs, (uint32_t)K, a.precision, a.layout, a.n_streams, N, t0, count, rows, pitch, nullptr};
        return launch_categorical_rows(r, prob_bytes, hs);
    }, hs);
}

template <int KIND>
static cst_status decode_categorical(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                     size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                     int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t* d_state,
                                     uint32_t* d_n_words_out, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_categorical_args(cfg, layout, d_symbols, d_probs, prob_bytes, n_symbols, false, d_words, d_n_words, d_status,
                                               KIND == kAns ? (const void*)d_state : (const void*)d_rstate, flags)) return st;
    CatDecodeArgs ca{};
    if (cst_status st = fill_decode_args(ca.a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream,
                                         layout, 0, n_symbols, d_status, flags)) return st;
    ca.a.state = d_state; ca.a.n_words_out = d_n_words_out; ca.a.rstate = d_rstate;
    ca.probs = d_probs;
    if (n_streams == 0) return CST_OK;
    const size_t blocks = (n_streams + kWave - 1) / kWave;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    // a lane per stream from a wave of streams on; fewer: a walk per symbol on one lane would leave the chip idle
    const int route = knobs().categorical_route;
    const bool fused = n_per_stream == 0 || (route ? route == 1 : n_streams >= (size_t)kWave);
    if (!fused) return note_kernel(kCatRowsName, decode_categorical_by_rows<KIND>(cfg, ca.a, d_probs, prob_bytes, hs));
    const dim3 grid((unsigned)blocks);
    dispatch_word_size(cfg, [&](auto W, auto S) {                        // (the launch error is read below)
        if (prob_bytes == 4) hipLaunchKernelGGL((decode_categorical_lane_kernel<W, S, KIND, float>), grid, dim3(kWave), kCatTileBytes<float>, hs, ca);
        else hipLaunchKernelGGL((decode_categorical_lane_kernel<W, S, KIND, double>), grid, dim3(kWave), kCatTileBytes<double>, hs, ca);
    });
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(kCatLaneNames[KIND == kRange], CST_OK);
}

// ---- Categorical(perfect=True): the quantiser is categorical_perfect_kernel (cst_categorical_perfect.hip); host glue only ----

static constexpr const char* kCatPerfectEncodeNames[2] = {"ans_encode_categorical_perfect_two_pass", "range_encode_categorical_perfect_two_pass"};
static constexpr const char* kCatPerfectRowsName = "decode_categorical_perfect_by_rows";

template <int KIND>
static cst_status encode_categorical_perfect(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                             int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                             size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, cst_range_state* d_rstate,
                                             int32_t* d_status, uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_categorical_args(cfg, layout, d_symbols, d_probs, prob_bytes, n_symbols, true, d_words, d_n_words, d_status,
                                               KIND == kAns ? (const void*)d_state : (const void*)d_rstate, flags)) return st;
    if (n_streams * n_per_stream > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    note_kernel(kCatPerfectEncodeNames[KIND == kRange], CST_OK);
    return encode_two_pass<KIND>(cfg, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words, d_state, d_rstate, d_status, flags, hs,
                                 [&](EncEntry* out, size_t) {
        CatPerfectArgs r{};
        r.probs = d_probs; r.prob_bytes = prob_bytes; r.K = (uint32_t)n_symbols; r.P = cfg.precision; r.layout = layout;
        r.n_streams = n_streams; r.N = n_per_stream; r.t0 = 0; r.count = n_per_stream;
        r.symbols = d_symbols; r.entries = out;
        (void)launch_categorical_perfect(r, hs);                         // (its launch error is read by encode_two_pass)
    });
}

// the route of decode_categorical_by_rows with the perfect tabulator: rows in pieces of at most 64 MiB, then a lookup per symbol
template <int KIND>
static cst_status decode_categorical_perfect(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                             size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                             int32_t n_symbols, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                             uint64_t* d_state, uint32_t* d_n_words_out, cst_range_state* d_rstate, int32_t* d_status,
                                             uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_categorical_args(cfg, layout, d_symbols, d_probs, prob_bytes, n_symbols, true, d_words, d_n_words, d_status,
                                               KIND == kAns ? (const void*)d_state : (const void*)d_rstate, flags)) return st;
    PerSymbolDecodeArgs a{};
    if (cst_status st = fill_decode_args(a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream,
                                         layout, 0, n_symbols, d_status, flags)) return st;
    a.state = d_state; a.n_words_out = d_n_words_out; a.rstate = d_rstate;
    if (n_streams == 0) return CST_OK;
    if (n_streams > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    const size_t N = n_per_stream, K = (size_t)n_symbols;
    // Every batch comes this way, not only the few-stream ones: decode_rows_wave_kernel's 256-entry rows (K < 256) are taken
    // while the 64 positions per stream that its pieces are made of fit the 64 MiB, the K + 1 word rows of the piece decoder
    // otherwise (and for N == 0, where one empty piece initialises and finishes the decoders).
    const size_t budget = (size_t)16 << 20;
    const bool packed = K < (size_t)kRowEntries && N > 0 && n_streams * 64 * (size_t)kRowEntries <= budget;
    const size_t pitch = packed ? (size_t)kRowEntries : K + 1;
    size_t piece = budget / (n_streams * pitch);
    if (packed) piece &= ~(size_t)63;
    else if (piece == 0) piece = 1;
    if (piece > N) piece = N;
    if (piece == 0) piece = 1;
    return decode_in_pieces<KIND>(cfg, a, packed, pitch, piece, [&](size_t t0, size_t count, uint32_t* rows) -> cst_status {
        CatPerfectArgs r{};
        r.probs = d_probs; r.prob_bytes = prob_bytes; r.K = (uint32_t)K; r.P = cfg.precision; r.layout = layout;
        r.n_streams = n_streams; r.N = N; r.t0 = t0; r.count = count; r.rows = rows; r.pitch = pitch;
        return launch_categorical_perfect(r, hs);
    }, hs, kCatPerfectRowsName);
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_categorical_fast_cdf_rows(int32_t precision, const void* d_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                         uint32_t* d_rows, int32_t* d_bad, void* stream) {
    if (!d_probs || !d_rows || (prob_bytes != 4 && prob_bytes != 8) || precision < 1 || precision > 31) return CST_ERR_INVALID_ARGUMENT;
    if (n_symbols < 2 || (uint64_t)n_symbols >= ((uint64_t)1 << precision) - 1) return CST_ERR_MODEL;
    CatRowsArgs r{d_probs, (uint32_t)n_symbols, precision, CST_LAYOUT_STREAM_MAJOR, 1, n_rows, 0, n_rows, d_rows, (size_t)n_symbols + 1, d_bad};
    return launch_categorical_rows(r, prob_bytes, (hipStream_t)stream);
}

cst_status cst_categorical_fast_cdf_host(int32_t precision, const void* h_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                         uint32_t* h_rows, int32_t* h_bad) {
    if (!h_probs || !h_rows || (prob_bytes != 4 && prob_bytes != 8) || precision < 1 || precision > 31) return CST_ERR_INVALID_ARGUMENT;
    if (n_symbols < 2 || (uint64_t)n_symbols >= ((uint64_t)1 << precision) - 1) return CST_ERR_MODEL;
    const size_t K = (size_t)n_symbols;
    for (size_t i = 0; i < n_rows; ++i) {
        const bool ok = prob_bytes == 4 ? cat_fast_cdf_row<float>(precision, reinterpret_cast<const float*>(h_probs) + i * K, (uint32_t)K, h_rows + i * (K + 1))
                                        : cat_fast_cdf_row<double>(precision, reinterpret_cast<const double*>(h_probs) + i * K, (uint32_t)K, h_rows + i * (K + 1));
        if (h_bad) h_bad[i] = ok ? 0 : 1;
    }
    return CST_OK;
}

cst_status cst_ans_encode_categorical_batch(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                            size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                                            uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status, uint32_t flags, void* stream) {
    return encode_categorical<kAns>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words,
                                    d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_batch(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                              size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                                              uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return encode_categorical<kRange>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words,
                                      nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                            size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                            int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t* d_state,
                                            uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_categorical<kAns>(cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols, d_symbols, n_streams,
                                    n_per_stream, layout, d_state, d_n_words_out, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                              size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes, int32_t n_symbols,
                                              int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, cst_range_state* d_rstate,
                                              int32_t* d_status, uint32_t flags, void* stream) {
    return decode_categorical<kRange>(cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols, d_symbols, n_streams,
                                      n_per_stream, layout, nullptr, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

cst_status cst_ans_encode_categorical_perfect_batch(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                                    size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status, uint32_t flags,
                                                    void* stream) {
    return encode_categorical_perfect<kAns>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_streams, n_per_stream, layout, d_words, stride_words,
                                            d_n_words, d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_encode_categorical_perfect_batch(cst_coder_config cfg, const int32_t* d_symbols, const void* d_probs, int32_t prob_bytes,
                                                      int32_t n_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                                      size_t stride_words, uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status,
                                                      uint32_t flags, void* stream) {
    return encode_categorical_perfect<kRange>(cfg, d_symbols, d_probs, prob_bytes, n_symbols, n_streams, n_per_stream, layout, d_words, stride_words,
                                              d_n_words, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

cst_status cst_ans_decode_categorical_perfect_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                                    size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                    int32_t n_symbols, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                                    uint64_t* d_state, uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_categorical_perfect<kAns>(cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols, d_symbols,
                                            n_streams, n_per_stream, layout, d_state, d_n_words_out, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_decode_categorical_perfect_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                                      size_t words_capacity, const uint32_t* d_n_words, const void* d_probs, int32_t prob_bytes,
                                                      int32_t n_symbols, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                                      cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_categorical_perfect<kRange>(cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_probs, prob_bytes, n_symbols, d_symbols,
                                              n_streams, n_per_stream, layout, nullptr, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

} // extern "C"
