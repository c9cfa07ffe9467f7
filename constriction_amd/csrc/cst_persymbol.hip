// cst_persymbol.hip -- coders driven by PER-SYMBOL entropy models (SURVEY.md 8f-1 and the single-coder drop-in).
//
//   * per-symbol quantized Gaussians: the reference's flagship call
//       coder.encode_reverse(symbols, QuantizedGaussian(lo, hi), means, stds) / coder.decode(family, means, stds)
//     (src/pybindings/stream/stack.rs:567-588, 733-751): every symbol gets its own
//     LeakilyQuantizedDistribution (src/stream/model/quantize.rs:525-568), i.e. two bit-exact f64 erf on device
//     per encoded symbol and a search over left cumulatives per decoded symbol;
//   * per-symbol quantized Laplace and Cauchy distributions: the same call with another family, the same kernels over another
//     policy (cst_family_policy.hpp; cst_*_family_batch);
//   * per-symbol Categorical models given as a matrix of floating-point probabilities, quantised inside the kernels by one
//     sequential sum per row (cst_categorical.hpp; cst_persymbol_categorical.hip);
//   * explicit per-symbol models: (left, prob) pairs for encoding and cdf rows for decoding.
//
// Encoding is two passes: a fully parallel pass turns every symbol into a coder entry (c, p, 2^64/p), then one
// LANE per stream runs the sequential recurrence over those entries.  Decoding uses one WAVE per stream:
// 64 lanes evaluate 64 candidate left cumulatives at once (two erf rounds / two coalesced row reads for a 201-symbol
// support).
// This file: what every family shares (encode_entries_kernel, pass 2 of every two-pass encoder; the rows-in-pieces decoders; the scratch
// pool), the explicit models, and every rectangular decoder but the Categorical ones; cst_persymbol.hpp has the map of the other files.
// (The kernels named "gaussian" are generic: FAM is a policy of cst_family_policy.hpp, and only the Gaussian stages the erf tables.)
#include <cstdlib>
#include <mutex>

#include "cst_persymbol.hpp"

namespace cst {

__global__ void cp_entries_kernel(const uint32_t* __restrict__ left, const uint32_t* __restrict__ prob, size_t n, int P,
                                  EncEntry* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c = left[i], p = prob[i];
    if ((uint64_t)c + p > ((uint64_t)1 << P)) p = 0;   // not a sub-interval of [0, 2^P): treat as impossible
    out[i] = make_entry(c, p);
}

// one lane per stream over precomputed entries; ANS walks backwards, the range coder forwards
template <int W, int S, int KIND>
__global__ __launch_bounds__(kBlock) void encode_entries_kernel(const EntriesEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * kRingWords;
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = s < a.n_streams;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const int G4 = 4 * groups_per_point(W, P);
    const size_t stride_t = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? a.n_streams : 1;
    const EncEntry* my = a.entries + (active ? (a.layout == CST_LAYOUT_SYMBOL_MAJOR ? s : s * N) : 0);
    uint32_t* slab = a.words + (active ? s : 0) * a.stride_words;
    const uint32_t cap = active ? (uint32_t)(a.stride_words > 0xffffffffull ? 0xffffffffull : a.stride_words) : 0u;
    uint32_t bad = 0, n_words = 0;
    int32_t status;
    int countdown = G4;

    if constexpr (KIND == kChain) {
        // ChainCoder::encode_symbol (src/stream/chain.rs:1140-1209), symbols last to first.  Not a hot path of the
        // library: plain per-lane loads and stores.
        using st_t = typename StateT<S>::type;
        constexpr uint32_t wmask = W == 32 ? 0xffffffffu : ((1u << (W % 32)) - 1u);
        status = CST_STREAM_OK;
        if (active) {
            cst_chain_heads h = a.heads[s];
            st_t rh = (st_t)h.remainders_head;
            uint32_t ch = h.compressed_head;
            const uint32_t* pop = a.pop_words + (a.pop_offsets ? a.pop_offsets[s] : s * a.pop_stride);
            uint32_t rd = a.n_pop[s];
            // entries kEntryGroup at a time, one group ahead of their use, and the next word of the popped stack one symbol
            // ahead (see the ANS branch)
            const uint32_t* idle = a.n_pop + s;
            uint32_t ahead = *(rd > 0 ? pop + (rd - 1) : idle);
            auto one = [&](const EncEntry e) {
                if (status != CST_STREAM_OK || bad) return;
                if (e.p == 0) { bad = 1; return; }
                bool refill = rh < ((st_t)e.p << (S - W - P));                  // refill_remainders_head, chain.rs:799-815
                if (refill && rd == 0) { status = CST_STREAM_OUT_OF_DATA; return; }
                rh = refill ? (st_t)((rh << (W % S)) | (st_t)(ahead & wmask)) : rh;
                rd -= refill ? 1u : 0u;
                st_t q;
                if constexpr (S == 64) q = mulhi64(rh, e.m_lo, e.m_hi);         // floor(rh / p) or one less
                else q = __umulhi(rh, e.m_hi);
                uint32_t r = (uint32_t)rh - (uint32_t)q * e.p;
                if (r >= e.p) { r -= e.p; q += 1; }
                const uint32_t quantile = e.c + r;
                rh = q;
                if (P != W && ch < (1u << (W - P))) ch = (ch << P) | quantile;
                else {
                    const uint32_t word = P == W ? quantile : (((ch << P) | quantile) & wmask);
                    if (P != W) ch >>= (W - P);
                    if (n_words < cap) slab[n_words] = word;
                    ++n_words;
                }
            };
            const size_t tail = N % kEntryGroup;
            for (size_t t = N; t-- > N - tail;) { one(my[t * stride_t]); ahead = *(rd > 0 ? pop + (rd - 1) : idle); }
            EncEntry cur[kEntryGroup], nxt[kEntryGroup];
            size_t g = N - tail;
            if (g > 0) {
#pragma unroll
                for (int k = 0; k < kEntryGroup; ++k) nxt[k] = my[(g - 1 - k) * stride_t];
            }
            while (g > 0 && status == CST_STREAM_OK && !bad) {
#pragma unroll
                for (int k = 0; k < kEntryGroup; ++k) cur[k] = nxt[k];
                g -= kEntryGroup;
                if (g > 0) {
#pragma unroll
                    for (int k = 0; k < kEntryGroup; ++k) nxt[k] = my[(g - 1 - k) * stride_t];
                }
#pragma unroll
                for (int k = 0; k < kEntryGroup; ++k) { one(cur[k]); ahead = *(rd > 0 ? pop + (rd - 1) : idle); }
            }
            if (n_words > cap) status = CST_STREAM_CAPACITY;
            h.remainders_head = (uint64_t)rh; h.compressed_head = ch;
            a.heads[s] = h;
            a.n_pop[s] = rd;
        }
    } else if constexpr (KIND == kAns) {
        EncLane<W, S> L;
        L.init(slab, cap, ring, lane);
        if (raw && active) L.state = (typename StateT<S>::type)a.state[s];
        // entries come kEntryGroup at a time, one group ahead of their use: a lone wave per SIMD has no other wave to
        // hide a load behind, and the address of every entry is known from the start
        const size_t tail = N % kEntryGroup;
        for (size_t t = N; t-- > N - tail;) {
            if (active) {
                const EncEntry e = my[t * stride_t];
                if (e.p == 0) bad = 1;
                else if (!bad) L.template step<false>(e, P);
            }
            if (--countdown == 0) { countdown = G4; L.flush_chunks(); }
        }
        EncEntry cur[kEntryGroup], nxt[kEntryGroup];
        size_t g = N - tail;                       // entries [g - kEntryGroup, g) are the next group
        if (g > 0 && active) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) nxt[j] = my[(g - 1 - j) * stride_t];
        }
        while (g > 0) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) cur[j] = nxt[j];
            g -= kEntryGroup;
            if (g > 0 && active) {
#pragma unroll
                for (int j = 0; j < kEntryGroup; ++j) nxt[j] = my[(g - 1 - j) * stride_t];
            }
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) {
                if (active) {
                    if (cur[j].p == 0) bad = 1;
                    else if (!bad) L.template step<false>(cur[j], P);
                }
                if (--countdown == 0) { countdown = G4; L.flush_chunks(); }
            }
        }
        status = L.finish(!raw, 1u, n_words);
        if (active && raw) a.state[s] = (uint64_t)L.state;
    } else {
        RangeEncLane<W, S> L;
        L.init(slab, cap, ring, lane);
        if (raw && active) {
            const cst_range_state r = a.rstate[s];
            L.lower = (typename StateT<S>::type)r.lower; L.range = (typename StateT<S>::type)r.range;
            L.inv_n = r.inverted_n; L.inv_first = r.inverted_first;
        }
        EncEntry cur[kEntryGroup], nxt[kEntryGroup];
        const size_t n_grouped = N - N % kEntryGroup;
        size_t g = 0;                              // entries [g, g + kEntryGroup) are the next group
        if (n_grouped > 0 && active) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) nxt[j] = my[j * stride_t];
        }
        while (g < n_grouped) {
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) cur[j] = nxt[j];
            g += kEntryGroup;
            if (g < n_grouped && active) {
#pragma unroll
                for (int j = 0; j < kEntryGroup; ++j) nxt[j] = my[(g + j) * stride_t];
            }
#pragma unroll
            for (int j = 0; j < kEntryGroup; ++j) {
                if (active) {
                    if (cur[j].p == 0) bad = 1;
                    else if (!bad) L.step(cur[j].c, cur[j].p, P);
                }
                if (--countdown == 0) { countdown = G4; L.out.flush_chunks(); }
            }
        }
        for (size_t t = n_grouped; t < N; ++t) {
            if (active) {
                const EncEntry e = my[t * stride_t];
                if (e.p == 0) bad = 1;
                else if (!bad) L.step(e.c, e.p, P);
            }
            if (--countdown == 0) { countdown = G4; L.out.flush_chunks(); }
        }
        if (raw) {
            L.out.drain();
            n_words = L.out.wr;
            status = L.out.wr > L.out.cap ? CST_STREAM_CAPACITY : CST_STREAM_OK;
            if (active) {
                cst_range_state r = a.rstate[s];
                r.lower = (uint64_t)L.lower; r.range = (uint64_t)L.range; r.inverted_n = L.inv_n; r.inverted_first = L.inv_first;
                a.rstate[s] = r;
            }
        } else {
            status = L.finish(1u, n_words);
        }
    }
    if (!active) return;
    if (bad) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
    a.status[s] = status;
    a.n_words[s] = (status == CST_STREAM_OK || KIND == kChain) ? n_words : 0u;
}

// One WAVE per stream.  Every lane carries the same coder state; the search for quantile_function (semantics of
// quantize.rs:580-779 / lookup_contiguous.rs:564-605: the unique symbol with left(sym) <= q < left(sym+1)) evaluates up
// to 64 candidate left cumulatives per round: two rounds for a 201-symbol support.  MODEL supplies left(element, i).
template <class PT = double>
struct GaussianLeftOf {
    static constexpr int32_t kBadModel = CST_STREAM_IMPOSSIBLE_SYMBOL;   // degenerate distribution (quantize.rs:562-565)
    static constexpr bool kErfTab = true;
    const PerSymbolDecodeArgs& a;
    const double2* erf_tab;
    double mu, sd;
    __device__ __forceinline__ bool load(size_t e) {
        mu = load_param(params_as<PT>(a.means) + e); sd = load_param(params_as<PT>(a.stds) + e);
        // the reference panics on an invalid model (pybindings/stream/model.rs:654-657)
        return sd > 0.0 && sd <= 1.7976931348623157e308 && mu == mu && mu <= 1.7976931348623157e308 && mu >= -1.7976931348623157e308;
    }
    __device__ __forceinline__ uint32_t left(uint32_t i) const {
        return leaky_gaussian_left_quick((int32_t)i, a.min_symbol, a.n_symbols, a.precision, 32, mu, sd, erf_tab);
    }
};
using GaussianLeft = GaussianLeftOf<double>;
// QuantizedLaplace / QuantizedCauchy (a = mean / loc in `means`, b = scale in `stds`): 64 exact CDFs per round
template <class FAM, class PT = double>
struct FamilyLeft {
    static constexpr int32_t kBadModel = CST_STREAM_IMPOSSIBLE_SYMBOL;
    static constexpr bool kErfTab = false;
    const PerSymbolDecodeArgs& a;
    const double2* unused;
    double pa, pb;
    __device__ __forceinline__ bool load(size_t e) { pa = load_param(params_as<PT>(a.means) + e); pb = load_param(params_as<PT>(a.stds) + e); return FAM::valid(pa, pb); }
    __device__ __forceinline__ uint32_t left(uint32_t i) const {
        return FAM::template left<false>((int32_t)i, a.min_symbol, a.n_symbols, a.precision, pa, pb, nullptr);
    }
};
using LaplaceLeft = FamilyLeft<LaplaceFamily>;
using CauchyLeft = FamilyLeft<CauchyFamily>;
struct RowLeft {                       // explicit cdf rows [n + 1] per coded symbol: 64 coalesced entries per round
    static constexpr int32_t kBadModel = CST_STREAM_INVALID_DATA;          // a row that is not a cdf for this quantile
    static constexpr bool kErfTab = true;                                  // (unused by the rows; as staged since the kernel was written)
    const PerSymbolDecodeArgs& a;
    const double2* unused;
    const uint32_t* row;
    __device__ __forceinline__ bool load(size_t e) { row = a.cdf_rows + e * a.row_stride; return true; }
    __device__ __forceinline__ uint32_t left(uint32_t i) const { return row[i]; }
};

template <int W, int S, int KIND, class MODEL>
__global__ __launch_bounds__(kBlock) void decode_wave_kernel(const PerSymbolDecodeArgs a) {
    const double2* erf_tab = nullptr;
    if constexpr (MODEL::kErfTab) {
        __shared__ double2 erf_lds[kErfTabEntries];
        erf_tab_fill(erf_lds, threadIdx.x, blockDim.x);
        __syncthreads();
        erf_tab = erf_lds;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (s >= a.n_streams) return;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const uint32_t n = (uint32_t)a.n_symbols;
    const size_t stride_t = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? a.n_streams : 1;
    const size_t e0 = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? s : s * N;

    DirectDecoder<W, S, KIND> D;
    D.init(a, s, raw);
    MODEL M{a, erf_tab};
    int32_t status = D.status;
    for (size_t t = 0; t < N && status == CST_STREAM_OK; ++t) {
        if (!M.load(e0 + t * stride_t)) { status = CST_STREAM_IMPOSSIBLE_SYMBOL; break; }
        const uint32_t q = D.quantile(P);
        if (D.status != CST_STREAM_OK) { status = D.status; break; }
        uint32_t base = 0, count = n;                 // invariant: left(base) <= q
        while (count > 63) {
            const uint32_t stride = (count + 63) / 64;
            const uint32_t off = (uint32_t)lane * stride;
            const bool valid = off < count;
            const uint32_t val = valid ? M.left(base + off) : 0u;
            const unsigned long long m = __ballot(valid && val <= q);
            const uint32_t k = max((uint32_t)__popcll(m), 1u);   // (lane 0 always qualifies for a valid table)
            const uint32_t adv = (k - 1) * stride;
            base += adv;
            count = min(stride, count - adv);
        }
        const uint32_t val = ((uint32_t)lane <= count) ? M.left(base + lane) : 0u;
        const unsigned long long m = __ballot((uint32_t)lane < count && val <= q);
        const uint32_t k = (uint32_t)__popcll(m);
        const uint32_t c = __shfl(val, (int)(k > 0 ? k - 1 : 0), 64), nxt = __shfl(val, (int)min(k, 63u), 64);
        const uint32_t p = nxt - c;
        if (p == 0 || k == 0 || c > q || (uint64_t)c + p > ((uint64_t)1 << P)) { status = MODEL::kBadModel; break; }
        if (lane == 0) a.symbols[e0 + t * stride_t] = a.min_symbol + (int32_t)(base + k - 1);
        D.advance(q, c, p, P);
        D.look_ahead();
    }
    if (lane == 0) {
        a.status[s] = status;
        D.finish(a, s, raw);
    }
}

// One LANE per stream (batches of at least a wave of streams): the search starts from an inverse-normal guess of the
// symbol and brackets the quantile with EXACT left cumulatives -- typically two erf evaluations per symbol instead of
// the 64 to 128 of a wave-wide search.  Any search returns the same symbol: the one with left(sym) <= q < left(sym + 1)
// (quantize.rs:580-779).

// Out of line ON PURPOSE: inlined, the compiler hoists the 32 + 8 row addresses of both variants out of the symbol loop
// into 130 VGPRs and then spills the erf's registers around every call of it.
__device__ __noinline__ void store_symbol_tile(int32_t* sym, size_t n_streams, size_t N, size_t s0, size_t t0, int lane, const int32_t* tile, bool vec) {
    if (vec) tile_store<true>(sym, n_streams, N, s0, t0, lane, tile);
    else tile_store<false>(sym, n_streams, N, s0, t0, lane, tile);
}

// 16-symbol output tile of the SMALL geometry -> HBM: piece (lane & 3) of rows (lane >> 2) + 16 k, 64-byte row segments
__device__ __noinline__ void store_symbol_tile16(int32_t* sym, size_t n_streams, size_t N, size_t s0, size_t t0, int lane, const int32_t* tile, bool vec) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t r = (size_t)(lane >> 2) + 16 * k;
        if (s0 + r >= n_streams) continue;
        const int32_t* src = tile + r * 20 + 4 * (lane & 3);
        int32_t* dst = sym + (s0 + r) * N + t0 + 4 * (lane & 3);
        if (vec) {
            const int4 v = *reinterpret_cast<const int4*>(src);
            v4i t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
            __builtin_nontemporal_store(t, reinterpret_cast<v4i*>(dst));
        } else {
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
        }
    }
}

// The row length as a request at the matrix's edges sees it.  Float kernels: an opaque copy, so that the rows' starts are formed THERE and
// not kept in registers through every tile -- the small geometry has none to spare (they cost it 16 bytes of scratch per lane).
template <class PT> __device__ __forceinline__ size_t edge_row_length(size_t n) {
    if constexpr (kParamF32<PT>) asm volatile("" : "+s"(n));
    return n;
}

template <int W, int S, int KIND, bool SMALL = false, class FAM = GaussianFamily, class PT = double>
__global__ __launch_bounds__(LaneGeo<SMALL>::kThreads) void decode_gaussian_lane_kernel(const PerSymbolDecodeArgs a) {
    using G = LaneGeo<SMALL>;
    constexpr int kParTile = G::kParTile, kWordWindow = G::kWordWindow, kOutSyms = G::kOutSyms, kOutStride = G::kOutStride;
    constexpr size_t kLaneDecWaveBytes = G::kWaveBytes;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* erf_tab = reinterpret_cast<double2*>(smem);
    if constexpr (FAM::kErfTab) {
        erf_tab_fill(erf_tab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int lane = threadIdx.x & (kWave - 1);
    unsigned char* mine = smem + (FAM::kErfTab ? kErfTabBytes : 0) + (size_t)(threadIdx.x >> 6) * kLaneDecWaveBytes;
    int32_t* tile = reinterpret_cast<int32_t*>(mine);
    double* par_mu = reinterpret_cast<double*>(mine + (size_t)kWave * kOutStride * 4);
    double* par_sd = par_mu + kParTile * kParStride;
    uint32_t* win = reinterpret_cast<uint32_t*>(par_sd + kParTile * kParStride);
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t s0 = s - lane;
    if (s0 >= a.n_streams) return;
    const bool active = s < a.n_streams;
    const size_t se = active ? s : a.n_streams - 1;          // idle lanes of a partial wave repeat its last stream
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const uint32_t n = (uint32_t)a.n_symbols;
    const bool symbol_major = a.layout == CST_LAYOUT_SYMBOL_MAJOR;
    const size_t stride_t = symbol_major ? a.n_streams : 1;
    const size_t e0 = symbol_major ? se : se * N;
    const double free_weight = (double)((P >= 32 ? 0xffffffffu : ((1u << P) - 1u)) - (n - 1u));
    const float total_f = (float)(1ull << P), free_f = (float)free_weight, inv_total_f = 1.0f / total_f, inv_free_f = 1.0f / free_f;
    const double guess_shift = 0.5 - (double)a.min_symbol;            // symbol index of the real number x: x - min_symbol + 0.5
    const bool vec = !symbol_major && (N % 4 == 0) && (reinterpret_cast<uintptr_t>(a.symbols) & 15) == 0;
    const bool two_step_guess = (double)n * 64.0 > free_weight;      // the leak moves the guess by more than 1/64 quantile

    DirectDecoder<W, S, KIND> D;
    D.init(a, se, raw);
    int32_t status = D.status;
    int32_t* sym_p = a.symbols + e0;

    // ---- parameter tiles: item w = it * 64 + lane of a tile is (stream j, symbol tl), consecutive lanes on consecutive
    // addresses in either layout ----
    // SMALL geometry, stream-major: a tile is 8 symbols = HALF a 128-byte line of doubles per stream.  Requested tile by tile, every
    // line of means and stds came in twice, ~16 000 cycles apart (round 5's counters: 10.24 GB per launch against 5.49 GB
    // algorithmic).  So a request there covers a PAIR of tiles -- whole lines, the big geometry's item mapping -- and the second
    // tile's half waits in the registers it arrived in: landed when its tile begins (mode 1 -> 2 -> 0 below).
    // PT = float: a line is 32 symbols -- two tiles of the big geometry, four of the small one.  The same scheme with kReqTile = 32: a
    // request covers kReqParts tiles, in as many registers as the doubles took (32 floats for 16 doubles), and mode counts 1 .. kReqParts.
    // A lane takes kVec consecutive floats of a line in one load -- kReqTile / kVec lanes to a line and as many loads per matrix: 64
    // single loads next to the word window's are more than a wave may have in flight (the load counter holds 63), and the request then
    // waits for its own first answers.  The small geometry loads PAIRS -- the loads, lanes and register pairs of its
    // double kernel exactly.  The big geometry loads quadruples, but for its RANGE decoders, which keep single loads (their registers
    // are the tightest: quadruples measured slower there).  Vector loads need rows that start on their size; others take the
    // single-tile requests below.
    constexpr int kVec = !kParamF32<PT> ? 1 : SMALL ? 2 : KIND != kRange ? 4 : 1;
    constexpr int kReqTile = kParamsPerLine<PT>;              // symbols a request can cover: one line (doubles: kParTile of the big geometry)
    constexpr int kReqParts = kReqTile / kParTile;            // tiles to a request: 1 (doubles, big), 2 (doubles, small; floats, big), 4 (floats, small)
    constexpr bool kMulti = kReqParts > 1;
    PT mu_r[kReqTile], sd_r[kReqTile];
    const PT* const means = params_as<PT>(a.means);
    const PT* const stds = params_as<PT>(a.stds);
    int mode = 0;                                             // (wave-uniform) 0: the registers hold ONE tile (or nothing); m >= 1: a line, its m-th part lands next
    // item `it` of a tile that lies wholly inside the matrix: element base_e + t0 * t_stride + it * item_stride (stream-major:
    // stream s0 + lane / 16 + 4 it, symbol t0 + lane % 16; symbol-major: symbol t0 + it, stream s0 + lane), LDS slot
    // base_l + it * l_stride -- pointer increments; tiles that stick out (last streams, last symbols) take the general form
    const size_t base_e = symbol_major ? s0 + (size_t)lane : (s0 + (size_t)(lane / kParTile)) * N + (size_t)(lane % kParTile);
    const size_t t_stride = symbol_major ? a.n_streams : 1, item_stride = symbol_major ? a.n_streams : (size_t)(kWave / kParTile) * N;
    const int base_l = symbol_major ? lane : (lane % kParTile) * kParStride + lane / kParTile;
    const int l_stride = symbol_major ? kParStride : kWave / kParTile;
    const bool vec_ok = kVec == 1 || (N % kVec == 0 && ((reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(stds)) & (4 * kVec - 1)) == 0);
    const bool pairs = kMulti && !symbol_major && s0 + kWave <= a.n_streams && vec_ok;
    constexpr int kLanesPerRow = kReqTile / kVec;             // (vector loads) lanes to a stream's kReqTile symbols = loads per matrix
    typedef float vec_t __attribute__((ext_vector_type(kVec > 1 ? kVec : 2)));
    auto par_request = [&](size_t t0) {
        if (kMulti && pairs && t0 % kReqTile == 0 && t0 + kReqTile <= N) {
            if constexpr (kVec > 1) {
                // item `it`: stream s0 + lane / kLanesPerRow + (64 / kLanesPerRow) it, symbols t0 + kVec (lane % kLanesPerRow) .. + kVec - 1,
                // in registers [kVec it, kVec it + kVec)
                const size_t ev = (s0 + (size_t)(lane / kLanesPerRow)) * N + (size_t)(kVec * (lane % kLanesPerRow)) + t0;
#pragma unroll
                for (int it = 0; it < kLanesPerRow; ++it) {
                    const vec_t mv = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(means + ev + (size_t)it * (kWave / kLanesPerRow) * N));
                    const vec_t sv = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(stds + ev + (size_t)it * (kWave / kLanesPerRow) * N));
#pragma unroll
                    for (int c = 0; c < kVec; ++c) { mu_r[kVec * it + c] = mv[c]; sd_r[kVec * it + c] = sv[c]; }
                }
                mode = 1;
                return;
            }
            const size_t e = (s0 + (size_t)(lane / kReqTile)) * N + (size_t)(lane % kReqTile) + t0;
            const PT* pm = means + e;
            const PT* ps = stds + e;
#pragma unroll
            for (int it = 0; it < kReqTile; ++it) {
                mu_r[it] = __builtin_nontemporal_load(pm + (size_t)it * (size_t)(kWave / kReqTile) * N);
                sd_r[it] = __builtin_nontemporal_load(ps + (size_t)it * (size_t)(kWave / kReqTile) * N);
            }
            mode = 1;
            return;
        }
        mode = 0;
        if (s0 + kWave <= a.n_streams && t0 + kParTile <= N) {
            const PT* pm = means + base_e + t0 * t_stride;
            const PT* ps = stds + base_e + t0 * t_stride;
#pragma unroll
            for (int it = 0; it < kParTile; ++it) {
                mu_r[it] = __builtin_nontemporal_load(pm + (size_t)it * item_stride);
                sd_r[it] = __builtin_nontemporal_load(ps + (size_t)it * item_stride);
            }
            return;
        }
#pragma unroll
        for (int it = 0; it < kParTile; ++it) {
            const int w = it * kWave + lane;
            const size_t j = symbol_major ? w % kWave : w / kParTile, tl = symbol_major ? w / kWave : w % kParTile;
            // (idle lanes of a partial wave repeat its last stream -- with that stream's parameters: the chain coder's lanes
            // write their remainders as they go)
            const size_t sj = s0 + j < a.n_streams ? s0 + j : a.n_streams - 1;
            const size_t e = t0 + tl < N ? (symbol_major ? (t0 + tl) * a.n_streams + sj : sj * edge_row_length<PT>(N) + t0 + tl) : 0;
            mu_r[it] = __builtin_nontemporal_load(means + e);
            sd_r[it] = __builtin_nontemporal_load(stds + e);
        }
    };
    auto par_land = [&]() {
        if (kMulti && mode != 0) {
            if constexpr (kVec > 1) {
                // part (mode - 1) of the request: the lanes whose kVec symbols lie in it write theirs, rows sub .. sub + kVec - 1 of the tile
                const int sub = kVec * (lane % kLanesPerRow) - kParTile * (mode - 1);
                if (sub >= 0 && sub < kParTile) {
#pragma unroll
                    for (int it = 0; it < kLanesPerRow; ++it) {
#pragma unroll
                        for (int c = 0; c < kVec; ++c) {
                            par_mu[(sub + c) * kParStride + lane / kLanesPerRow + (kWave / kLanesPerRow) * it] = (double)mu_r[kVec * it + c];
                            par_sd[(sub + c) * kParStride + lane / kLanesPerRow + (kWave / kLanesPerRow) * it] = (double)sd_r[kVec * it + c];
                        }
                    }
                }
                mode = mode < kReqParts ? mode + 1 : 0;
                return;
            }
            // part (mode - 1) of the line: the lanes that hold symbols kParTile (mode - 1) .. + kParTile - 1 of it write theirs
            const int sub = (lane % kReqTile) - kParTile * (mode - 1);
            if (sub >= 0 && sub < kParTile) {
#pragma unroll
                for (int it = 0; it < kReqTile; ++it) {
                    par_mu[sub * kParStride + lane / kReqTile + (kWave / kReqTile) * it] = (double)mu_r[it];
                    par_sd[sub * kParStride + lane / kReqTile + (kWave / kReqTile) * it] = (double)sd_r[it];
                }
            }
            mode = mode < kReqParts ? mode + 1 : 0;
            return;
        }
#pragma unroll
        for (int it = 0; it < kParTile; ++it) {
            par_mu[base_l + it * l_stride] = (double)mu_r[it];
            par_sd[base_l + it * l_stride] = (double)sd_r[it];
        }
    };
    // ---- word window: a tile of 16 symbols takes at most 16 words, so with the 16 words behind the read position in
    // LDS at the start of a tile the NEXT 16 can be on their way during it ----
    uint32_t w_r[kParTile];
    int64_t w_first = 0;                                      // index of w_r[0]
    auto win_request = [&](int64_t first) {
        w_first = first;
        const int64_t len = (int64_t)D.length();
        if (!__any(first < 0 || first + kParTile > len)) {    // every lane's 16 words exist: one pointer, sixteen offsets
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
    };
    auto win_land = [&]() {
#pragma unroll
        for (int i = 0; i < kParTile; ++i) win[(((uint32_t)(w_first + i)) & (kWordWindow - 1)) * kWave + lane] = w_r[i];
    };
    const auto window_of = [&](int ahead_tiles) -> int64_t {  // first index of the 16 words `ahead_tiles` tiles ahead
        return D.kDownward ? (int64_t)D.position() - (int64_t)kParTile * (ahead_tiles + 1) : (int64_t)D.position() + (int64_t)kParTile * ahead_tiles;
    };

    if (N > 0) {
        par_request(0);
        win_request(window_of(0));
    }
    for (size_t t0 = 0; t0 < N; t0 += kParTile) {
        wave_lds_fence();                                     // (the previous tile's parameters have been read)
        par_land();
        win_land();
        if (t0 + kParTile < N && mode == 0) par_request(t0 + kParTile);      // (mode >= 2: the next tile's parameters are here already)
        win_request(window_of(1));                            // (the words one tile further: used from the next tile on)
        wave_lds_fence();
        const int n_here = (int)(N - t0 < (size_t)kParTile ? N - t0 : (size_t)kParTile);
#pragma unroll 1
        for (int tl = 0; tl < n_here; ++tl) {
            const size_t t = t0 + (size_t)tl;
            int32_t sym = 0;
            const double mu = par_mu[tl * kParStride + lane], sd = par_sd[tl * kParStride + lane];
            D.ahead = win[(((uint32_t)D.next_index()) & (kWordWindow - 1)) * kWave + lane];
            if (status == CST_STREAM_OK) {
                // the reference panics on an invalid model (pybindings/stream/model.rs:654-657)
                const bool model_ok = FAM::valid(mu, sd);
                const uint32_t q = model_ok ? D.quantile(P) : 0u;
                if (!model_ok) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
                else if (D.status != CST_STREAM_OK) status = D.status;
                else {
                    // guess: ignore the leak (one quantile per symbol) first, then account for the guessed symbol's share of it
                    const float below = (float)q + 0.5f, above = total_f - below;
                    const bool coarse = FAM::kGaussian && !__any(sd >= 200.0);          // (wave-uniform: the cheap quantile is good enough)
                    float z = coarse ? FAM::guess_z_coarse(fminf(below, above) * inv_total_f) : FAM::guess_z(fminf(below, above) * inv_total_f);
                    double x = mu + sd * (double)(below < above ? z : -z) + guess_shift;
                    if (two_step_guess) {
                        const float b1 = below - (float)fmin(fmax(x, 0.0), (double)(n - 1u)), a1 = free_f - b1;
                        z = FAM::guess_z(fmaxf(fminf(b1, a1), 0.25f) * inv_free_f);
                        x = mu + sd * (double)(b1 < a1 ? z : -z) + guess_shift;
                    }
                    // first probe: the bin BOUNDARY nearest to the guess (boundary i lies at x = i) -- whichever side of it the
                    // quantile falls, the second probe closes the bracket as long as the guess is within half a symbol; probing
                    // floor(x) first cost a third evaluation whenever the guess was a hair low, and a wave runs as many
                    // evaluations as its worst lane
                    const uint32_t g = (uint32_t)fmin(fmax(x + 0.5, 1.0), (double)(n - 1u));
                    // bracket [lo_i, hi_i): left(lo_i) = lo_v <= q < hi_v = left(hi_i)
                    uint32_t lo_i = 0, hi_i = n, lo_v = 0, hi_v = P >= 32 ? 0u : (1u << P);
                    uint32_t probe = g, step = 1;
                    bool up = false, down = false;
                    {
                        // ... and its two neighbours in the same breath: the three evaluations share their LDS latency, and a
                        // guess within half a symbol -- almost every one -- is bracketed without a second look
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
            if (symbol_major) {
                if (active) *sym_p = sym;
                sym_p += stride_t;
            } else {
                tile[lane * kOutStride + (t % kOutSyms)] = sym;
                if (t % kOutSyms == kOutSyms - 1) {
                    wave_lds_fence();
                    if constexpr (SMALL) store_symbol_tile16(a.symbols, a.n_streams, N, s0, t - (kOutSyms - 1), lane, tile, vec);
                    else store_symbol_tile(a.symbols, a.n_streams, N, s0, t - (kOutSyms - 1), lane, tile, vec);
                    wave_lds_fence();
                }
            }
        }
    }
    if (!symbol_major) {
        const size_t done = N - N % kOutSyms;
        if (active) for (size_t t = done; t < N; ++t) a.symbols[se * N + t] = tile[lane * kOutStride + (t % kOutSyms)];
    }
    if (!active) return;
    a.status[s] = status;
    D.finish(a, s, raw);
}

// FEWER streams than a wave has lanes -- down to the reference's own usage, ONE coder and a long message.  Decoding a
// stream is sequential, and with the model search inside the chain every symbol costs an erf latency (1.7 us).  But
// only the QUANTILE depends on the coder state, the models do not: a first kernel tabulates every symbol's whole cdf row
// at full occupancy (256 erf per symbol: 2.4 ms per million symbols), and the sequential kernel is left with a lookup.
// A row is 256 left cumulatives (supports up to 255 symbols, padded with 2^P); lane l of the stream's wave holds
// entries 4l..4l+3 of the current row in registers, straight from one coalesced 1-KiB load issued eight symbols
// earlier.  One ballot finds the lane, three compares the entry: ~45 instructions per symbol instead of ~600.
constexpr int kRowsAhead = 16;

template <class FAM = GaussianFamily, class PT = double>
__global__ __launch_bounds__(kRowEntries) void gaussian_rows_kernel(int P, int32_t lo, int32_t n, const PT* __restrict__ means,
                                                                   const PT* __restrict__ stds, int32_t layout, size_t n_streams,
                                                                   size_t N, size_t t0, size_t count, uint32_t* __restrict__ rows) {
    const double2* erf_tab = nullptr;
    if constexpr (FAM::kErfTab) {
        __shared__ double2 erf_lds[kErfTabEntries];
        erf_tab_fill(erf_lds, threadIdx.x, blockDim.x);
        __syncthreads();
        erf_tab = erf_lds;
    }
    const size_t row = blockIdx.x;                     // = stream * count + (t - t0)
    const size_t s = row / count, t = t0 + row % count;
    const size_t e = layout == CST_LAYOUT_SYMBOL_MAJOR ? t * n_streams + s : s * N + t;
    const double mu = load_param(means + e), sd = load_param(stds + e);
    const int32_t i = (int32_t)threadIdx.x;
    const uint32_t total = 1u << P;
    uint32_t v;
    if (FAM::valid(mu, sd))
        v = i <= n ? FAM::template left<false>(i, lo, n, P, mu, sd, erf_tab) : total;
    else v = i == 0 ? 0xffffffffu : total;             // invalid model (a valid row starts with 0)
    rows[row * kRowEntries + i] = v;
}

struct RowsDecodeArgs {
    PerSymbolDecodeArgs a;
    const uint4* rows;          // [stream][count][64 lanes] x 4 entries
    size_t t0, count;
    DecodeResume* resume;       // [stream]
    int32_t first, last;
};

// The row queue and the word blocks below are plain loads: the compiler's own counter bookkeeping waits, at the use of a
// row, for exactly the loads older than the fifteen youngest -- as long as NO other load sits in the loop (a per-symbol
// look-ahead of the next compressed word, waited for every symbol, drags the whole in-order queue with it and collapses
// the 16-deep queue to depth one; measured 340 ns per symbol).  Hand-issued loads in inline asm are not an option in a
// C++ loop: the compiler copies loop-carried registers at the bottom of the loop, in flight or not.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// The stream's compressed words, 64 at a time in one register across the wave (lane l: the l-th word from the block's
// origin in reading direction).  A symbol consumes at most one word, so a block fetched at the start of a 64-symbol
// group lasts for the whole group.
template <int KIND>
struct WordBlock {
    uint32_t cur;
    uint32_t origin;                    // read position the block starts at (ANS: counts down, range: up)
    __device__ __forceinline__ void fetch(const uint32_t* in, uint32_t len, uint32_t position, int lane) {
        origin = position;
        const uint32_t i = KIND == kAns ? position - 1u - (uint32_t)lane : position + (uint32_t)lane;      // (ANS: wraps below 0)
        cur = in[i < len ? i : 0u];
    }
    // the word at read position `position` (ANS: the next word to pop is in[position - 1])
    __device__ __forceinline__ uint32_t at(uint32_t position) const {
        const uint32_t off = KIND == kAns ? origin - position : position - origin;
        return (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(off & 63u));
    }
};

// one symbol of decode_rows_wave_kernel: `r` = this lane's four entries of the symbol's row
template <int W, int S, int KIND>
__device__ __forceinline__ void rows_step(DirectDecoder<W, S, KIND>& D, const WordBlock<KIND>& words, const v4u r, uint32_t slot, int lane,
                                          uint32_t n, int32_t min_symbol, int P, int32_t& status, int32_t& mine) {
    const uint32_t q = D.quantile(P);
    const bool le = r.x <= q;
    const unsigned long long m = __ballot(le);
    const uint32_t cnt = (le ? 1u : 0u) + (r.y <= q ? 1u : 0u) + (r.z <= q ? 1u : 0u) + (r.w <= q ? 1u : 0u);
    const uint32_t my_c = cnt >= 4 ? r.w : cnt == 3 ? r.z : cnt == 2 ? r.y : r.x;
    const uint32_t my_n = cnt == 3 ? r.w : cnt == 2 ? r.z : r.y;
    const uint32_t k = ((uint32_t)__popcll(m) - 1u) & 63u;   // the last lane whose first entry is <= q
    const uint32_t ck = (uint32_t)__builtin_amdgcn_readlane((int)cnt, (int)k);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)my_c, (int)k);
    const uint32_t n_in = (uint32_t)__builtin_amdgcn_readlane((int)my_n, (int)k);
    const uint32_t n_out = (uint32_t)__builtin_amdgcn_readlane((int)r.x, (int)min(k + 1u, 63u));
    const uint32_t nxt = ck >= 4 ? n_out : n_in;
    const uint32_t idx = 4u * k + ck - 1u, p = nxt - c;
    // an invalid model marks entry 0 (then no lane's first entry is <= q, or lane 0's is not); a degenerate distribution
    // (quantize.rs:562-565) has p == 0; a quantile beyond the support cannot happen for a valid row
    const bool bad = (m & 1) == 0 || idx >= n || p == 0;
    const int32_t fail = D.status != CST_STREAM_OK ? D.status : bad ? CST_STREAM_IMPOSSIBLE_SYMBOL : CST_STREAM_OK;
    if (status == CST_STREAM_OK) {
        status = fail;
        if (fail == CST_STREAM_OK) {
            if ((uint32_t)lane == slot) mine = min_symbol + (int32_t)idx;
            if constexpr (KIND == kAns) D.ahead = words.at(D.rd);
            else D.ahead = words.at(D.pos);
            D.advance(q, c, p, P);
        }
    }
}

template <int W, int S, int KIND>
__global__ __launch_bounds__(kWave) void decode_rows_wave_kernel(const RowsDecodeArgs ra) {
    const PerSymbolDecodeArgs& a = ra.a;
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const uint32_t n = (uint32_t)a.n_symbols;
    const size_t stride_t = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? a.n_streams : 1;
    int32_t* out = a.symbols + (a.layout == CST_LAYOUT_SYMBOL_MAJOR ? s : s * N) + ra.t0 * stride_t;
    const v4u* rows = reinterpret_cast<const v4u*>(ra.rows) + s * ra.count * kWave + lane;
    const size_t count = ra.count;

    DirectDecoder<W, S, KIND> D;
    int32_t status;
    if (ra.first) { D.init(a, s, raw); status = D.status; }
    else { const DecodeResume r = ra.resume[s]; D.resume(a, s, r); status = r.status; }
    WordBlock<KIND> words;
    const uint32_t n_words = max(a.slice(s).n, 1u);
    auto fetch_words = [&]() {
        if constexpr (KIND == kAns) words.fetch(D.in, n_words, D.rd, lane);
        else words.fetch(D.in, n_words, D.pos, lane);
        // waited for HERE, once per 64 symbols: left pending, the compiler waits at every use with a count that drains
        // the row queue to two
        asm volatile("" : "+v"(words.cur));
    };

    v4u ahead[kRowsAhead];
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) ahead[j] = __builtin_nontemporal_load(rows + min((size_t)j, count - 1) * kWave);
    int32_t mine = 0;                                  // lane l keeps the symbol of position 64 g + l until the group is stored
    size_t tl = 0;
    // whole blocks whose rows ahead all exist: no bounds checks
    for (; tl + 2 * kRowsAhead <= count && status == CST_STREAM_OK; tl += kRowsAhead) {
        if ((tl & 63) == 0) fetch_words();
        const uint32_t slot0 = (uint32_t)(tl & 63);
        const v4u* next = rows + (tl + kRowsAhead) * kWave;
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j) {
            const v4u r = ahead[j];
            ahead[j] = __builtin_nontemporal_load(next + j * kWave);
            rows_step<W, S, KIND>(D, words, r, slot0 + j, lane, n, a.min_symbol, P, status, mine);
        }
        if (slot0 == 64 - kRowsAhead) out[(tl + kRowsAhead - 64 + lane) * stride_t] = mine;     // (also the group an error stopped in)
    }
    // the last one or two blocks
    for (; tl < count && status == CST_STREAM_OK; tl += kRowsAhead) {
        if ((tl & 63) == 0) fetch_words();
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j) {
            const size_t t = tl + j;
            const v4u r = ahead[j];
            if (t + kRowsAhead < count) ahead[j] = __builtin_nontemporal_load(rows + (t + kRowsAhead) * kWave);
            if (t < count) rows_step<W, S, KIND>(D, words, r, (uint32_t)(t & 63), lane, n, a.min_symbol, P, status, mine);
            if (t < count && (t & 63) == 63) out[(t - 63 + lane) * stride_t] = mine;
        }
    }
    // the last, partial group (or the group an error stopped in: its remaining symbols are unspecified)
    const size_t reached = min(tl, count);
    if ((reached & 63) != 0 && (reached & ~(size_t)63) + lane < count) out[((reached & ~(size_t)63) + lane) * stride_t] = mine;
    if (lane != 0) return;
    if (ra.last) { a.status[s] = status; D.finish(a, s, raw); }
    else { DecodeResume r; D.park(r); r.status = status; ra.resume[s] = r; }
}

// ------------------------------------------------------------------------------------------------
// A FEW CHAINS (down to the reference's own usage: one).  A chain coder's quantiles do not depend on the models: symbol
// t's P bits sit at a position of `compressed` that only the head's fill level decides.  So decoding is three kernels:
//   1. per chain, sequential but trivial: cut the quantiles out of the words (no model in the loop);
//   2. per SYMBOL, in parallel over the whole chip: the model search (exact erf brackets / binary search of a cdf row);
//   3. per chain, sequential but trivial: fold (quantile - left, probability) into the remainders head, flush words.
// One wave per chain for 1 and 3, with the coder state uniform (the compiler keeps it in scalar registers) and the
// inputs fetched 64 at a time.  Against one wave per chain searching inside the loop: ~1.7 us -> ~0.1 us per symbol.
// ------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(kWave) void chain_quantiles_kernel(const PerSymbolDecodeArgs a, uint32_t* __restrict__ quantiles,
                                                                uint32_t* __restrict__ n_cut) {
    constexpr uint32_t wmask = W == 32 ? 0xffffffffu : ((1u << (W % 32)) - 1u);
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x, N = a.n_per_stream;
    const int P = a.precision;
    const WordSlice ws = a.slice(s);
    const uint32_t* in = a.words + ws.off;
    const uint32_t n_words = max(ws.n, 1u);
    uint32_t rd = ws.n;
    uint32_t ch = a.heads[s].compressed_head;
    WordBlock<kAns> words;
    uint32_t mine = 0;
    size_t t = 0;
    for (; t < N; ++t) {
        if ((t & 63) == 0) { words.fetch(in, n_words, rd, lane); asm volatile("" : "+v"(words.cur)); }
        uint32_t word;
        if (P == W || ch < (1u << P)) {                         // decode_symbol, chain.rs:1060-1098
            if (rd == 0) break;                                 // DecoderFrontendError::OutOfCompressedData
            word = words.at(rd) & wmask; --rd;
            if (P != W) ch = ((ch << (W - P)) | (word >> P)) & wmask;
        } else {
            word = ch; ch >>= P;
        }
        const uint32_t q = P == W ? word : (word & ((1u << P) - 1u));
        if ((uint32_t)lane == (uint32_t)(t & 63)) mine = q;
        if ((t & 63) == 63) quantiles[s * N + t - 63 + lane] = mine;
    }
    if ((t & 63) != 0 && (uint32_t)lane < (uint32_t)(t & 63)) quantiles[s * N + (t & ~(size_t)63) + lane] = mine;
    if (lane == 0) {
        n_cut[s] = (uint32_t)t;
        a.heads[s].compressed_head = ch;
        a.n_words_out[s] = rd;
    }
}

// (symbol, quantile - left, probability) of every cut quantile; probability 0 marks an invalid model
template <bool GAUSSIAN>
__global__ __launch_bounds__(kBlock) void chain_lookup_kernel(const PerSymbolDecodeArgs a, const uint32_t* __restrict__ quantiles,
                                                              const uint32_t* __restrict__ n_cut, uint2* __restrict__ pairs) {
    __shared__ double2 erf_tab[kErfTabEntries];
    erf_tab_fill(erf_tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const size_t N = a.n_per_stream;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_streams * N) return;
    const size_t s = i / N, t = i - s * N;
    if (t >= n_cut[s]) return;
    const size_t e = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? t * a.n_streams + s : i;
    const uint32_t q = quantiles[i];
    const int P = a.precision;
    const uint32_t n = (uint32_t)a.n_symbols;
    uint32_t lo_i = 0, hi_i = n, lo_v = 0, hi_v = P >= 32 ? 0u : (1u << P);     // left(lo_i) = lo_v <= q < hi_v = left(hi_i)
    bool ok = true;
    if constexpr (GAUSSIAN) {
        const double mu = params_as<double>(a.means)[e], sd = params_as<double>(a.stds)[e];     // (the chain coder takes doubles only)
        ok = sd > 0.0 && sd <= 1.7976931348623157e308 && fabs(mu) <= 1.7976931348623157e308;
        if (ok) {
            // the guess and the bracketing of decode_gaussian_lane_kernel
            const double free_weight = (double)((P >= 32 ? 0xffffffffu : ((1u << P) - 1u)) - (n - 1u));
            const float total_f = (float)(1ull << P), free_f = (float)free_weight;
            const double guess_shift = 0.5 - (double)a.min_symbol;
            const float below = (float)q + 0.5f, above = total_f - below;
            float z = ndtri_lower_f32(fminf(below, above) / total_f);
            double x = mu + sd * (double)(below < above ? z : -z) + guess_shift;
            if ((double)n * 64.0 > free_weight) {
                const float b1 = below - (float)fmin(fmax(x, 0.0), (double)(n - 1u)), a1 = free_f - b1;
                z = ndtri_lower_f32(fmaxf(fminf(b1, a1), 0.25f) / free_f);
                x = mu + sd * (double)(b1 < a1 ? z : -z) + guess_shift;
            }
            uint32_t probe = (uint32_t)fmin(fmax(x, 1.0), (double)(n - 1u)), step = 1;
            bool up = false, down = false;
            while (hi_i - lo_i > 1) {
                const uint32_t v = leaky_gaussian_left_quick((int32_t)probe, a.min_symbol, (int32_t)n, P, 32, mu, sd, erf_tab);
                if (v <= q) { lo_i = probe; lo_v = v; up = true; } else { hi_i = probe; hi_v = v; down = true; }
                if (up && down) probe = lo_i + (hi_i - lo_i) / 2;
                else if (up) probe = min(lo_i + step, hi_i - 1u);
                else probe = max(hi_i - min(step, hi_i - 1u), lo_i + 1u);
                step *= 2;
            }
        }
    } else {
        const uint32_t* row = a.cdf_rows + e * a.row_stride;
        while (hi_i - lo_i > 1) {                               // lookup_contiguous.rs:564-605: any search finds the same entry
            const uint32_t mid = lo_i + (hi_i - lo_i) / 2, v = row[mid];
            if (v <= q) { lo_i = mid; lo_v = v; } else { hi_i = mid; hi_v = v; }
        }
        lo_v = row[lo_i]; hi_v = row[lo_i + 1];
        ok = lo_v <= q && hi_v > lo_v && ((uint64_t)hi_v <= ((uint64_t)1 << P)) && q < hi_v;
    }
    const uint32_t p = hi_v - lo_v;
    ok = ok && p != 0 && lo_v <= q && (uint64_t)lo_v + p <= ((uint64_t)1 << P);
    a.symbols[e] = a.min_symbol + (int32_t)lo_i;
    pairs[i] = ok ? make_uint2(q - lo_v, p) : make_uint2(0u, 0u);
}

template <int W, int S>
__global__ __launch_bounds__(kWave) void chain_fold_kernel(const PerSymbolDecodeArgs a, const uint2* __restrict__ pairs,
                                                           const uint32_t* __restrict__ n_cut, int32_t bad_model_status) {
    using st_t = typename StateT<S>::type;
    constexpr uint32_t wmask = W == 32 ? 0xffffffffu : ((1u << (W % 32)) - 1u);
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x, N = a.n_per_stream;
    const int P = a.precision;
    const uint32_t n = n_cut[s];
    st_t rh = (st_t)a.heads[s].remainders_head;
    uint32_t* out = a.push_words + s * a.push_stride;
    const uint32_t cap = (uint32_t)(a.push_stride > 0xffffffffull ? 0xffffffffull : a.push_stride);
    uint32_t wr = 0, mine = 0;
    int32_t status = CST_STREAM_OK;
    for (uint32_t t0 = 0; t0 < n && status == CST_STREAM_OK; t0 += kWave) {
        const uint2 pr = t0 + lane < n ? pairs[s * N + t0 + lane] : make_uint2(0u, 1u);
        const uint32_t m = min((uint32_t)kWave, n - t0);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t rem = (uint32_t)__builtin_amdgcn_readlane((int)pr.x, (int)j);
            const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pr.y, (int)j);
            if (p == 0) { status = bad_model_status; break; }
            rh = (st_t)(rh * (st_t)p + (st_t)rem);              // decode_symbol, chain.rs:1104-1116
            if (rh >= ((st_t)1 << (S - P))) {
                if ((uint32_t)lane == (wr & 63u)) mine = (uint32_t)rh & wmask;
                if ((wr & 63u) == 63u && wr < cap) out[wr - 63u + lane] = mine;     // (cap is a multiple of 64 or the tail below stores)
                ++wr;
                rh = (st_t)(rh >> (W % S));
            }
        }
    }
    if ((wr & 63u) != 0 && (uint32_t)lane < (wr & 63u) && (wr & ~63u) + lane < cap) out[(wr & ~63u) + lane] = mine;
    if (lane != 0) return;
    if (status == CST_STREAM_OK && n < N) status = CST_STREAM_OUT_OF_DATA;
    if (wr > cap) status = CST_STREAM_CAPACITY;
    a.heads[s].remainders_head = (uint64_t)rh;
    a.n_push[s] = wr;
    a.status[s] = status;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

cst_status check_common(cst_coder_config cfg, cst_layout layout) {
    if (!config_supported(cfg)) return CST_ERR_INVALID_ARGUMENT;
    if (layout != CST_LAYOUT_STREAM_MAJOR && layout != CST_LAYOUT_SYMBOL_MAJOR) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

template <int KIND>
cst_status launch_encode_entries(cst_coder_config cfg, const EntriesEncodeArgs& a, hipStream_t hs) {
    const size_t blocks = (a.n_streams + kBlock - 1) / kBlock;
    const size_t lds = (size_t)(kBlock / kWave) * kRingWords * sizeof(uint32_t);
    dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((encode_entries_kernel<W, S, KIND>), dim3((unsigned)blocks), dim3(kBlock), lds, hs, a); });
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}
template cst_status launch_encode_entries<kAns>(cst_coder_config, const EntriesEncodeArgs&, hipStream_t);
template cst_status launch_encode_entries<kRange>(cst_coder_config, const EntriesEncodeArgs&, hipStream_t);
template cst_status launch_encode_entries<kChain>(cst_coder_config, const EntriesEncodeArgs&, hipStream_t);

// Scratch (encoder entries, cdf rows of few-stream decodes, chain quantiles) comes from a stream-ordered memory pool
// that belongs to THIS LIBRARY -- one per device, created at first use -- whose release threshold is raised so that it
// keeps freed memory: a pool at its defaults hands everything back at the next synchronisation, and allocating 4 GiB
// afresh costs more than coding them (measured: 70 of 88 ms per call at 65 536 x 4096).  The device's DEFAULT pool is
// never touched: a host application's own hipMallocAsync traffic (PyTorch's async allocator, say) keeps its behaviour.
std::mutex g_pool_mutex;
hipMemPool_t g_pools[64] = {};

hipError_t scratch_pool(hipMemPool_t* out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    if (!g_pools[dev]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        e = hipMemPoolCreate(&pool, &props);
        if (e != hipSuccess) return e;
        uint64_t keep = ~0ull;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        g_pools[dev] = pool;
    }
    *out = g_pools[dev];
    return hipSuccess;
}

hipError_t scratch_alloc(void** ptr, size_t bytes, hipStream_t hs) {
    hipMemPool_t pool;
    hipError_t e = scratch_pool(&pool);
    if (e != hipSuccess) return e;
    return hipMallocFromPoolAsync(ptr, bytes, pool, hs);
}

// few streams: cdf rows at full occupancy, then a lookup per symbol; in pieces of at most 64 MiB of rows
template <int KIND, class FAM, class PT>
static cst_status decode_gaussian_by_rows(cst_coder_config cfg, const PerSymbolDecodeArgs& a, hipStream_t hs) {
    const size_t N = a.n_per_stream;
    // 65 536 rows = 64 MiB of rows per piece (the piece size makes no measurable difference from 4096 rows up: the
    // sequential kernel is bound by its dependent instruction chain, not by the rows' memory latency)
    size_t piece = ((size_t)65536 / a.n_streams) & ~(size_t)63;        // (n_streams < 64: at least 1024 symbols)
    if (piece > N) piece = N;
    return decode_in_pieces<KIND>(cfg, a, true, kRowEntries, piece, [&](size_t t0, size_t count, uint32_t* rows) -> cst_status {
        hipLaunchKernelGGL((gaussian_rows_kernel<FAM, PT>), dim3((unsigned)(a.n_streams * count)), dim3(kRowEntries), 0, hs, a.precision, a.min_symbol,
                           a.n_symbols, static_cast<const PT*>(a.means), static_cast<const PT*>(a.stds), a.layout, a.n_streams, N, t0, count, rows);
        return CST_OK;                  // (its launch error is read behind the decoder's launch)
    }, hs);
}

// a few chains: cut the quantiles, search all symbols in parallel, fold the remainders
static cst_status decode_chains_in_three(cst_coder_config cfg, const PerSymbolDecodeArgs& a, bool gaussian, hipStream_t hs) {
    const size_t n = a.n_streams * a.n_per_stream;
    uint32_t* scratch = nullptr;                 // [quantiles n][pairs 2n][n_cut n_streams]
    CST_HIP_TRY(scratch_alloc((void**)&scratch, (3 * n + a.n_streams + 2) * sizeof(uint32_t), hs));
    uint32_t* quantiles = scratch;
    uint2* pairs = reinterpret_cast<uint2*>(scratch + ((n + 1) & ~(size_t)1));
    uint32_t* n_cut = scratch + ((n + 1) & ~(size_t)1) + 2 * n;
    dispatch_word_size(cfg, [&](auto W, auto) { hipLaunchKernelGGL((chain_quantiles_kernel<W>), dim3((unsigned)a.n_streams), dim3(kWave), 0, hs, a, quantiles, n_cut); });
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    if (gaussian) hipLaunchKernelGGL((chain_lookup_kernel<true>), dim3(blocks), dim3(kBlock), 0, hs, a, quantiles, n_cut, pairs);
    else hipLaunchKernelGGL((chain_lookup_kernel<false>), dim3(blocks), dim3(kBlock), 0, hs, a, quantiles, n_cut, pairs);
    const int32_t bad = gaussian ? GaussianLeft::kBadModel : RowLeft::kBadModel;
    dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((chain_fold_kernel<W, S>), dim3((unsigned)a.n_streams), dim3(kWave), 0, hs, a, pairs, n_cut, bad); });
    const hipError_t err = hipGetLastError();
    (void)hipFreeAsync(scratch, hs);
    CST_HIP_TRY(err);
    return CST_OK;
}

// `gaussian`: per-symbol parameters of family FAM in a.means / a.stds, matrices of PT (else explicit cdf rows)
template <int KIND, class FAM = GaussianFamily, class PT = double>
static cst_status decode_per_symbol(cst_coder_config cfg, const PerSymbolDecodeArgs& a, bool gaussian, hipStream_t hs) {
    static_assert(KIND != kChain || !kParamF32<PT>, "the chain coder takes doubles");
    using WaveModel = std::conditional_t<FAM::kGaussian, GaussianLeftOf<PT>, FamilyLeft<FAM, PT>>;
    using Names = FamilyNames<FAM, PT>;
    constexpr size_t kLdsBig = FAM::kErfTab ? LaneGeo<false>::kLdsBytes : LaneGeo<false>::kLdsBytesNoTab;
    constexpr size_t kLdsSmall = FAM::kErfTab ? LaneGeo<true>::kLdsBytes : LaneGeo<true>::kLdsBytesNoTab;
    if (a.n_streams == 0) return CST_OK;
    const size_t blocks = (a.n_streams * kWave + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (KIND == kChain && a.n_streams < (size_t)kWave && a.n_per_stream >= 64 && a.n_streams * a.n_per_stream < ((size_t)1 << 31))
        return decode_chains_in_three(cfg, a, gaussian, hs);
    if (gaussian && a.n_streams >= (size_t)kWave) {      // enough streams to give every lane its own
        // more streams than one wave per SIMD: the small geometry, eight waves per CU (CST_LANE_GEO=big|small forces one: A/B runs)
        int cus = 256;
        { int dev = 0; hipDeviceProp_t prop; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount; }
        const int geo = knobs().lane_geo;
        const bool small = KIND != kChain && (geo ? geo == 2 : a.n_streams > (size_t)cus * kBlock);
        auto go = [&](auto kernel, int threads, size_t lds) -> cst_status {
            const size_t lane_blocks = (a.n_streams + threads - 1) / threads;
            CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kernel, dim3((unsigned)lane_blocks), dim3(threads), lds, hs, a);
            return CST_OK;
        };
        auto lane = [&](auto small_geo) {                         // (std::bool_constant: the geometry)
            constexpr bool kSmall = decltype(small_geo)::value;
            return dispatch_word_size(cfg, [&](auto W, auto S) { return go(decode_gaussian_lane_kernel<W, S, KIND, kSmall, FAM, PT>, LaneGeo<kSmall>::kThreads, kSmall ? kLdsSmall : kLdsBig); });
        };
        cst_status rc;
        if constexpr (KIND != kChain) rc = small ? lane(std::true_type{}) : lane(std::false_type{});
        else rc = lane(std::false_type{});
        if (rc != CST_OK) return rc;
        note_kernel(KIND == kChain || !small ? Names::lane[KIND] : Names::lane_small[KIND == kRange], CST_OK);
    } else if (KIND != kChain && gaussian && a.n_symbols < kRowEntries && a.n_per_stream >= 32) {
        note_kernel(Names::by_rows, CST_OK);
        if constexpr (KIND != kChain) return decode_gaussian_by_rows<KIND, FAM, PT>(cfg, a, hs);
    } else if (gaussian) {
        dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((decode_wave_kernel<W, S, KIND, WaveModel>), dim3((unsigned)blocks), dim3(kBlock), 0, hs, a); });
        if (!FAM::kGaussian || kParamF32<PT>) note_kernel(Names::wave[KIND == kRange], CST_OK);     // (the f64 Gaussian call has never recorded this route)
    } else {
        dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((decode_wave_kernel<W, S, KIND, RowLeft>), dim3((unsigned)blocks), dim3(kBlock), 0, hs, a); });
    }
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

cst_status fill_decode_args(PerSymbolDecodeArgs& a, cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets,
                            size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, int32_t* d_symbols, size_t n_streams,
                            size_t n_per_stream, cst_layout layout, int32_t min_symbol, int64_t n_symbols, int32_t* d_status,
                            uint32_t flags) {
    if (cst_status st = check_common(cfg, layout)) return st;
    if (!d_n_words || !d_status || (n_per_stream > 0 && !d_symbols)) return CST_ERR_INVALID_ARGUMENT;
    // (the same support limit as the encoding entry points: per-symbol models hold no tables, any n <= 2^P works)
    if (n_symbols < 2 || n_symbols > ((int64_t)1 << cfg.precision)) return CST_ERR_MODEL;
    a.words = d_words; a.offsets = d_offsets; a.stride_words = stride_words; a.n_words = d_n_words; a.symbols = d_symbols;
    a.n_streams = n_streams; a.n_per_stream = n_per_stream; a.layout = layout; a.precision = cfg.precision;
    a.min_symbol = min_symbol; a.n_symbols = (int32_t)n_symbols; a.status = d_status; a.flags = flags;
    a.row_stride = (size_t)n_symbols + 1; a.words_capacity = words_capacity;
    return CST_OK;
}

// ---- chain coder: shared parts of the entry points ----
static cst_status chain_decode_common(PerSymbolDecodeArgs& a, cst_coder_config cfg, const uint32_t* d_pop_words, const uint64_t* d_pop_offsets,
                                      size_t pop_stride, uint32_t* d_n_pop, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                      cst_layout layout, int32_t min_symbol, int64_t n_symbols, uint32_t* d_push_words, size_t push_stride,
                                      uint32_t* d_n_push, cst_chain_heads* d_heads, int32_t* d_status) {
    if (cst_status st = fill_decode_args(a, cfg, d_pop_words, d_pop_offsets, pop_stride, 0, d_n_pop, d_symbols, n_streams, n_per_stream, layout,
                                         min_symbol, n_symbols, d_status, 0)) return st;
    // (d_pop_words must be a valid device pointer even when every d_n_pop[s] is 0: the kernels request a stream's next word
    // ahead of knowing whether they will need it)
    if (!d_heads || !d_n_push || !d_pop_words || (n_per_stream > 0 && !d_push_words)) return CST_ERR_INVALID_ARGUMENT;
    a.push_words = d_push_words; a.push_stride = push_stride; a.n_push = d_n_push; a.heads = d_heads; a.n_words_out = d_n_pop;
    return CST_OK;
}

// What cst_{ans,range}_decode_gaussian_batch[_f32] say of their arguments, in their order, without the device -- and `a` filled for the
// launch.  `raw_state`: the coder's raw state (d_state / d_rstate).  The jump-point decoders ask it too, BEFORE their first kernel, with
// the arguments they will hand to the batch call: a refused call launches nothing and is refused with the status it always had.
static cst_status gaussian_decode_args(PerSymbolDecodeArgs& a, cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                       const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                       const void* d_means, const void* d_stds, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                       cst_layout layout, const void* raw_state, int32_t* d_status, uint32_t flags) {
    if (max_symbol <= min_symbol) return CST_ERR_MODEL;
    if (cst_status st = fill_decode_args(a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream, layout,
                                         min_symbol, (int64_t)max_symbol - min_symbol + 1, d_status, flags)) return st;
    if (n_per_stream > 0 && (!d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if ((flags & CST_FLAG_RAW_STATE) && !raw_state) return CST_ERR_INVALID_ARGUMENT;
    a.means = d_means; a.stds = d_stds;
    return CST_OK;
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_release_scratch(void) {
    hipMemPool_t pool;
    CST_HIP_TRY(scratch_pool(&pool));
    CST_HIP_TRY(hipDeviceSynchronize());
    CST_HIP_TRY(hipMemPoolTrimTo(pool, 0));
    return CST_OK;
}

cst_status cst_ans_encode_cp_batch(cst_coder_config cfg, const uint32_t* d_left, const uint32_t* d_prob, size_t n_streams,
                                   size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                                   uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status, uint32_t flags, void* stream) {
    if (n_per_stream > 0 && (!d_left || !d_prob)) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    return encode_two_pass<kAns>(cfg, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words, d_state, nullptr,
                                 d_status, flags, hs, [&](EncEntry* out, size_t n) {
        hipLaunchKernelGGL(cp_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, d_left, d_prob, n, cfg.precision, out);
    });
}

cst_status cst_range_encode_cp_batch(cst_coder_config cfg, const uint32_t* d_left, const uint32_t* d_prob, size_t n_streams,
                                     size_t n_per_stream, cst_layout layout, uint32_t* d_words, size_t stride_words,
                                     uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    if (n_per_stream > 0 && (!d_left || !d_prob)) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    return encode_two_pass<kRange>(cfg, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words, nullptr, d_rstate,
                                   d_status, flags, hs, [&](EncEntry* out, size_t n) {
        hipLaunchKernelGGL(cp_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, d_left, d_prob, n, cfg.precision, out);
    });
}

__global__ void gaussian_ckpt_offsets_kernel(const uint64_t* __restrict__ offsets, size_t stride_words, size_t n_streams, size_t n_chunks,
                                             const uint64_t* __restrict__ state_in, uint64_t* __restrict__ v_offsets, uint64_t* __restrict__ v_state) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_streams * n_chunks) return;
    const size_t s = v / n_chunks;
    v_offsets[v] = offsets ? offsets[s] : s * stride_words;
    v_state[v] = state_in[v];                  // (the raw decode updates its state array)
}

} // extern "C"

// (defined below, with their entry points)
template <class PT>
static cst_status ans_decode_gaussian_batch_impl(cst_coder_config, int32_t, int32_t, const uint32_t*, const uint64_t*, size_t, size_t, const uint32_t*, const PT*,
                                                 const PT*, int32_t*, size_t, size_t, cst_layout, uint64_t*, uint32_t*, int32_t*, uint32_t, void*);
template <class PT>
static cst_status range_decode_gaussian_batch_impl(cst_coder_config, int32_t, int32_t, const uint32_t*, const uint64_t*, size_t, size_t, const uint32_t*, const PT*,
                                                   const PT*, int32_t*, size_t, size_t, cst_layout, cst_range_state*, int32_t*, uint32_t, void*);

template <class PT>
static cst_status ans_decode_gaussian_batch_ckpt_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                      const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, size_t ckpt_interval,
                                                      const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_state, const PT* d_means, const PT* d_stds,
                                                      int32_t* d_symbols, size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    if (!d_ckpt_pos || !d_ckpt_state || !d_scratch || !d_status || ckpt_interval == 0 || n_per_stream % ckpt_interval != 0) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0 || n_per_stream == 0) return CST_OK;
    const size_t n_chunks = n_per_stream / ckpt_interval, n_virtual = n_streams * n_chunks;
    uint64_t* v_offsets = reinterpret_cast<uint64_t*>(d_scratch);
    uint64_t* v_state = v_offsets + n_virtual;
    const size_t capacity = words_capacity ? words_capacity : (d_offsets ? 0 : n_streams * stride_words);
    PerSymbolDecodeArgs judged{};           // (what the decode call below will say of its arguments: before anything is launched)
    if (cst_status st = gaussian_decode_args(judged, cfg, min_symbol, max_symbol, d_words, v_offsets, 0, capacity, d_ckpt_pos, d_means, d_stds, d_symbols,
                                             n_virtual, ckpt_interval, CST_LAYOUT_STREAM_MAJOR, v_state, d_status, CST_FLAG_RAW_STATE)) return st;
    hipLaunchKernelGGL(gaussian_ckpt_offsets_kernel, dim3((unsigned)((n_virtual + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_offsets, stride_words,
                       n_streams, n_chunks, d_ckpt_state, v_offsets, v_state);
    CST_HIP_TRY(hipGetLastError());
    const cst_status rc = ans_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, v_offsets, 0, capacity, d_ckpt_pos, d_means, d_stds, d_symbols,
                                                        n_virtual, ckpt_interval, CST_LAYOUT_STREAM_MAJOR, v_state, nullptr, d_status, CST_FLAG_RAW_STATE, stream);
    if (rc != CST_OK) return rc;
    return flag_bad_jump_points(d_ckpt_pos, n_streams, n_chunks, d_offsets ? 0 : stride_words, d_status, (hipStream_t)stream);
}

extern "C" {

cst_status cst_ans_decode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                              const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, size_t ckpt_interval,
                                              const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_state, const double* d_means, const double* d_stds,
                                              int32_t* d_symbols, size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    return ans_decode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, ckpt_interval,
           d_ckpt_pos, d_ckpt_state, d_means, d_stds, d_symbols, n_streams, n_per_stream, d_scratch, d_status, stream);
}
cst_status cst_ans_decode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                  const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, size_t ckpt_interval,
                                                  const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_state, const void* d_means, const void* d_stds,
                                                  int32_t* d_symbols, size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    return ans_decode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, ckpt_interval,
           d_ckpt_pos, d_ckpt_state, f32(d_means), f32(d_stds), d_symbols, n_streams, n_per_stream, d_scratch, d_status, stream);
}

size_t cst_range_gaussian_ckpt_scratch_bytes(size_t n_streams, size_t n_per_stream, size_t ckpt_interval) {
    if (ckpt_interval == 0) return 0;
    return (sizeof(cst_range_state) + 16) * n_streams * ((n_per_stream + ckpt_interval - 1) / ckpt_interval) + 64;
}

} // extern "C"  (kernels and templates have C++ linkage)

// virtual stream v = (stream v / k, chunk v % k): where its words lie, and the decoder state RangeDecoder::seek leaves (queue.rs:911-926)
template <int W, int S>
__global__ void gaussian_range_virtual_kernel(const uint32_t* __restrict__ words, const uint64_t* __restrict__ offsets, size_t stride_words,
                                              uint64_t capacity, const uint32_t* __restrict__ n_words, const uint32_t* __restrict__ ckpt_pos,
                                              const uint64_t* __restrict__ ckpt_lower, const uint64_t* __restrict__ ckpt_range, size_t n_streams,
                                              size_t n_chunks, uint64_t* __restrict__ v_offsets, uint32_t* __restrict__ v_n,
                                              cst_range_state* __restrict__ v_state) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_streams * n_chunks) return;
    const size_t s = v / n_chunks;
    const WordSlice ws = word_slice(offsets, stride_words, n_words, s, capacity);
    const uint32_t pos0 = ckpt_pos[v] < ws.n ? ckpt_pos[v] : ws.n;
    uint64_t pt = 0;
    uint32_t pos = pos0;
    int num_read = 0;
    const uint64_t mask = S == 64 ? ~0ull : ((1ull << (S % 64)) - 1ull);
    while (pos < ws.n) {                                          // read_point, queue.rs:847-868
        pt = ((pt << (W % 64)) | (uint64_t)words[ws.off + pos++]) & mask;
        if (++num_read == S / W) break;
    }
    if (num_read < S / W && num_read != 0) pt = (pt << (S - num_read * W)) & mask;
    cst_range_state r{};
    r.lower = ckpt_lower[v]; r.range = ckpt_range[v]; r.point = pt; r.position = pos;
    v_state[v] = r;
    v_offsets[v] = offsets ? offsets[s] : (uint64_t)s * stride_words;   // (the decoder checks the slice again: a bad one stays bad)
    v_n[v] = n_words[s];
}

__global__ void gaussian_range_flag_kernel(const uint32_t* __restrict__ n_words, const uint32_t* __restrict__ ckpt_pos, size_t n_streams, size_t n_chunks,
                                           int32_t* __restrict__ status) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_streams * n_chunks) return;
    if (ckpt_pos[v] > n_words[v / n_chunks]) status[v] = CST_STREAM_INVALID_DATA;      // a jump point beyond its stream's words
}

template <class PT>
static cst_status range_decode_gaussian_batch_ckpt_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                        const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                        size_t ckpt_interval, const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_lower,
                                                        const uint64_t* d_ckpt_range, const PT* d_means, const PT* d_stds, int32_t* d_symbols,
                                                        size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    if (!d_n_words || !d_ckpt_pos || !d_ckpt_lower || !d_ckpt_range || !d_scratch || !d_status || ckpt_interval == 0 || n_per_stream % ckpt_interval != 0)
        return CST_ERR_INVALID_ARGUMENT;
    if (cfg.word_bits != 32 && cfg.word_bits != 16) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0 || n_per_stream == 0) return CST_OK;
    if (!d_words) return CST_ERR_INVALID_ARGUMENT;
    const size_t n_chunks = n_per_stream / ckpt_interval, n_virtual = n_streams * n_chunks;
    if (n_virtual > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    const size_t capacity = words_capacity ? words_capacity : (d_offsets ? 0 : n_streams * stride_words);
    cst_range_state* v_state = reinterpret_cast<cst_range_state*>((reinterpret_cast<uintptr_t>(d_scratch) + 15) & ~(uintptr_t)15);
    uint64_t* v_offsets = reinterpret_cast<uint64_t*>(v_state + n_virtual);
    uint32_t* v_n = reinterpret_cast<uint32_t*>(v_offsets + n_virtual);
    PerSymbolDecodeArgs judged{};           // (what the decode call below will say of its arguments: before anything is launched)
    if (cst_status st = gaussian_decode_args(judged, cfg, min_symbol, max_symbol, d_words, v_offsets, 0, capacity, v_n, d_means, d_stds, d_symbols,
                                             n_virtual, ckpt_interval, CST_LAYOUT_STREAM_MAJOR, v_state, d_status, CST_FLAG_RAW_STATE)) return st;
    const dim3 grid((unsigned)((n_virtual + 255) / 256));
    if (cfg.word_bits == 32)
        hipLaunchKernelGGL((gaussian_range_virtual_kernel<32, 64>), grid, dim3(256), 0, hs, d_words, d_offsets, stride_words, capacity, d_n_words, d_ckpt_pos,
                           d_ckpt_lower, d_ckpt_range, n_streams, n_chunks, v_offsets, v_n, v_state);
    else
        hipLaunchKernelGGL((gaussian_range_virtual_kernel<16, 32>), grid, dim3(256), 0, hs, d_words, d_offsets, stride_words, capacity, d_n_words, d_ckpt_pos,
                           d_ckpt_lower, d_ckpt_range, n_streams, n_chunks, v_offsets, v_n, v_state);
    CST_HIP_TRY(hipGetLastError());
    const cst_status rc = range_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, v_offsets, 0, capacity, v_n, d_means, d_stds, d_symbols,
                                                          n_virtual, ckpt_interval, CST_LAYOUT_STREAM_MAJOR, v_state, d_status, CST_FLAG_RAW_STATE, stream);
    if (rc != CST_OK) return rc;
    hipLaunchKernelGGL(gaussian_range_flag_kernel, grid, dim3(256), 0, hs, d_n_words, d_ckpt_pos, n_streams, n_chunks, d_status);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

extern "C" {

cst_status cst_range_decode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                size_t ckpt_interval, const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_lower,
                                                const uint64_t* d_ckpt_range, const double* d_means, const double* d_stds, int32_t* d_symbols,
                                                size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    return range_decode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words,
           ckpt_interval, d_ckpt_pos, d_ckpt_lower, d_ckpt_range, d_means, d_stds, d_symbols, n_streams, n_per_stream, d_scratch, d_status, stream);
}
cst_status cst_range_decode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                    const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                    size_t ckpt_interval, const uint32_t* d_ckpt_pos, const uint64_t* d_ckpt_lower,
                                                    const uint64_t* d_ckpt_range, const void* d_means, const void* d_stds, int32_t* d_symbols,
                                                    size_t n_streams, size_t n_per_stream, void* d_scratch, int32_t* d_status, void* stream) {
    return range_decode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words,
           ckpt_interval, d_ckpt_pos, d_ckpt_lower, d_ckpt_range, f32(d_means), f32(d_stds), d_symbols, n_streams, n_per_stream, d_scratch, d_status,
           stream);
}

} // extern "C"

template <class PT>
static cst_status ans_decode_gaussian_batch_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                 const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                 const PT* d_means, const PT* d_stds, int32_t* d_symbols, size_t n_streams,
                                                 size_t n_per_stream, cst_layout layout, uint64_t* d_state, uint32_t* d_n_words_out,
                                                 int32_t* d_status, uint32_t flags, void* stream) {
    PerSymbolDecodeArgs a{};
    if (cst_status st = gaussian_decode_args(a, cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_means, d_stds,
                                             d_symbols, n_streams, n_per_stream, layout, d_state, d_status, flags)) return st;
    a.state = d_state; a.n_words_out = d_n_words_out;
    return decode_per_symbol<kAns, GaussianFamily, PT>(cfg, a, true, (hipStream_t)stream);
}

extern "C" {

cst_status cst_ans_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                         const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                         const double* d_means, const double* d_stds, int32_t* d_symbols, size_t n_streams,
                                         size_t n_per_stream, cst_layout layout, uint64_t* d_state, uint32_t* d_n_words_out,
                                         int32_t* d_status, uint32_t flags, void* stream) {
    return ans_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_means, d_stds,
           d_symbols, n_streams, n_per_stream, layout, d_state, d_n_words_out, d_status, flags, stream);
}
cst_status cst_ans_decode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                             const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                             const void* d_means, const void* d_stds, int32_t* d_symbols, size_t n_streams,
                                             size_t n_per_stream, cst_layout layout, uint64_t* d_state, uint32_t* d_n_words_out,
                                             int32_t* d_status, uint32_t flags, void* stream) {
    return ans_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, f32(d_means),
           f32(d_stds), d_symbols, n_streams, n_per_stream, layout, d_state, d_n_words_out, d_status, flags, stream);
}

} // extern "C"

template <class PT>
static cst_status range_decode_gaussian_batch_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                                   const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                                   const PT* d_means, const PT* d_stds, int32_t* d_symbols, size_t n_streams,
                                                   size_t n_per_stream, cst_layout layout, cst_range_state* d_rstate, int32_t* d_status,
                                                   uint32_t flags, void* stream) {
    PerSymbolDecodeArgs a{};
    if (cst_status st = gaussian_decode_args(a, cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_means, d_stds,
                                             d_symbols, n_streams, n_per_stream, layout, d_rstate, d_status, flags)) return st;
    a.rstate = d_rstate;
    return decode_per_symbol<kRange, GaussianFamily, PT>(cfg, a, true, (hipStream_t)stream);
}

extern "C" {

cst_status cst_range_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                           const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                           const double* d_means, const double* d_stds, int32_t* d_symbols, size_t n_streams,
                                           size_t n_per_stream, cst_layout layout, cst_range_state* d_rstate, int32_t* d_status,
                                           uint32_t flags, void* stream) {
    return range_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_means, d_stds,
           d_symbols, n_streams, n_per_stream, layout, d_rstate, d_status, flags, stream);
}
cst_status cst_range_decode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                               const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                               const void* d_means, const void* d_stds, int32_t* d_symbols, size_t n_streams,
                                               size_t n_per_stream, cst_layout layout, cst_range_state* d_rstate, int32_t* d_status,
                                               uint32_t flags, void* stream) {
    return range_decode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, f32(d_means),
           f32(d_stds), d_symbols, n_streams, n_per_stream, layout, d_rstate, d_status, flags, stream);
}

cst_status cst_ans_decode_rows_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words, size_t words_capacity,
                                     const uint32_t* d_n_words, const uint32_t* d_cdf_rows, int32_t n_symbols, int32_t min_symbol,
                                     int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t* d_state,
                                     uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    PerSymbolDecodeArgs a{};
    if (cst_status st = fill_decode_args(a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream, layout,
                                         min_symbol, n_symbols, d_status, flags)) return st;
    if (n_per_stream > 0 && !d_cdf_rows) return CST_ERR_INVALID_ARGUMENT;
    if ((flags & CST_FLAG_RAW_STATE) && !d_state) return CST_ERR_INVALID_ARGUMENT;
    a.cdf_rows = d_cdf_rows; a.state = d_state; a.n_words_out = d_n_words_out;
    return decode_per_symbol<kAns>(cfg, a, false, (hipStream_t)stream);
}

cst_status cst_range_decode_rows_batch(cst_coder_config cfg, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words, size_t words_capacity,
                                       const uint32_t* d_n_words, const uint32_t* d_cdf_rows, int32_t n_symbols, int32_t min_symbol,
                                       int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                       cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    PerSymbolDecodeArgs a{};
    if (cst_status st = fill_decode_args(a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream, layout,
                                         min_symbol, n_symbols, d_status, flags)) return st;
    if (n_per_stream > 0 && !d_cdf_rows) return CST_ERR_INVALID_ARGUMENT;
    if ((flags & CST_FLAG_RAW_STATE) && !d_rstate) return CST_ERR_INVALID_ARGUMENT;
    a.cdf_rows = d_cdf_rows; a.rstate = d_rstate;
    return decode_per_symbol<kRange>(cfg, a, false, (hipStream_t)stream);
}

// ---- chain coder ----
cst_status cst_chain_decode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_pop_words,
                                           const uint64_t* d_pop_offsets, size_t pop_stride, uint32_t* d_n_pop, const double* d_means,
                                           const double* d_stds, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, uint32_t* d_push_words, size_t push_stride, uint32_t* d_n_push,
                                           cst_chain_heads* d_heads, int32_t* d_status, void* stream) {
    PerSymbolDecodeArgs a{};
    if (max_symbol <= min_symbol) return CST_ERR_MODEL;
    if (cst_status st = chain_decode_common(a, cfg, d_pop_words, d_pop_offsets, pop_stride, d_n_pop, d_symbols, n_streams, n_per_stream, layout,
                                            min_symbol, (int64_t)max_symbol - min_symbol + 1, d_push_words, push_stride, d_n_push, d_heads,
                                            d_status)) return st;
    if (n_per_stream > 0 && (!d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    a.means = d_means; a.stds = d_stds;
    return decode_per_symbol<kChain>(cfg, a, true, (hipStream_t)stream);
}

cst_status cst_chain_decode_rows_batch(cst_coder_config cfg, const uint32_t* d_pop_words, const uint64_t* d_pop_offsets, size_t pop_stride,
                                       uint32_t* d_n_pop, const uint32_t* d_cdf_rows, size_t row_stride, int32_t n_symbols,
                                       int32_t min_symbol, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                       uint32_t* d_push_words, size_t push_stride, uint32_t* d_n_push, cst_chain_heads* d_heads,
                                       int32_t* d_status, void* stream) {
    PerSymbolDecodeArgs a{};
    if (cst_status st = chain_decode_common(a, cfg, d_pop_words, d_pop_offsets, pop_stride, d_n_pop, d_symbols, n_streams, n_per_stream, layout,
                                            min_symbol, n_symbols, d_push_words, push_stride, d_n_push, d_heads, d_status)) return st;
    if (n_per_stream > 0 && !d_cdf_rows) return CST_ERR_INVALID_ARGUMENT;
    if (row_stride != 0 && row_stride != (size_t)n_symbols + 1) return CST_ERR_INVALID_ARGUMENT;
    a.cdf_rows = d_cdf_rows; a.row_stride = row_stride;
    return decode_per_symbol<kChain>(cfg, a, false, (hipStream_t)stream);
}

cst_status cst_chain_encode_cp_batch(cst_coder_config cfg, const uint32_t* d_left, const uint32_t* d_prob, size_t n_streams,
                                     size_t n_per_stream, cst_layout layout, const uint32_t* d_pop_words, const uint64_t* d_pop_offsets,
                                     size_t pop_stride, uint32_t* d_n_pop, uint32_t* d_push_words, size_t push_stride, uint32_t* d_n_push,
                                     cst_chain_heads* d_heads, int32_t* d_status, void* stream) {
    if (n_per_stream > 0 && (!d_left || !d_prob)) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    return chain_encode_common(cfg, n_streams, n_per_stream, layout, d_pop_words, d_pop_offsets, pop_stride, d_n_pop, d_push_words, push_stride,
                               d_n_push, d_heads, d_status, hs, [&](EncEntry* out, size_t n) {
        hipLaunchKernelGGL(cp_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, d_left, d_prob, n, cfg.precision, out);
    });
}

} // extern "C"

namespace cst {

// everything that can be said about the arguments of a Laplace / Cauchy call without the device, the same for all four calls
cst_status check_family_args(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, cst_layout layout,
                             const void* d_symbols, const void* d_a, const void* d_b, const void* d_words, const void* d_n_words,
                             const void* d_status, const void* raw_state, uint32_t flags) {
    if (family != CST_FAMILY_LAPLACE && family != CST_FAMILY_CAUCHY) return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol) return CST_ERR_INVALID_ARGUMENT;
    if (!d_symbols || !d_a || !d_b || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if ((flags & CST_FLAG_RAW_STATE) && !raw_state) return CST_ERR_INVALID_ARGUMENT;
    if (cst_status st = check_common(cfg, layout)) return st;
    if (support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;      // LeakyQuantizer::new asserts this
    return CST_OK;
}

// (PT in front of FAM: CST_FAMILY_CALL names the coder and the family)
template <int KIND, class FAM, class PT>
static cst_status decode_per_symbol_of(const PT*, cst_coder_config cfg, const PerSymbolDecodeArgs& a, hipStream_t hs) {
    return decode_per_symbol<KIND, FAM, PT>(cfg, a, true, hs);
}

template <int KIND, class PT>
static cst_status decode_family(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const PT* d_a,
                                const PT* d_b, int32_t* d_symbols, size_t n_streams, size_t n_per_stream, cst_layout layout, uint64_t* d_state,
                                uint32_t* d_n_words_out, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, hipStream_t hs) {
    if (cst_status st = check_family_args(cfg, family, min_symbol, max_symbol, layout, d_symbols, d_a, d_b, d_words, d_n_words, d_status,
                                          KIND == kAns ? (const void*)d_state : (const void*)d_rstate, flags)) return st;
    PerSymbolDecodeArgs a{};
    if (cst_status st = fill_decode_args(a, cfg, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_symbols, n_streams, n_per_stream, layout,
                                         min_symbol, (int64_t)max_symbol - min_symbol + 1, d_status, flags)) return st;
    a.means = d_a; a.stds = d_b; a.state = d_state; a.n_words_out = d_n_words_out; a.rstate = d_rstate;
    return CST_FAMILY_CALL(decode_per_symbol_of, KIND, d_a, cfg, a, hs);
}

} // namespace cst

extern "C" {

cst_status cst_ans_decode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                       const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                       const double* d_a, const double* d_b, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                       cst_layout layout, uint64_t* d_state, uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_family<kAns>(cfg, family, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_a, d_b, d_symbols,
                               n_streams, n_per_stream, layout, d_state, d_n_words_out, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_decode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                         const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                         const double* d_a, const double* d_b, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                         cst_layout layout, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_family<kRange>(cfg, family, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, d_a, d_b, d_symbols,
                                 n_streams, n_per_stream, layout, nullptr, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

// ---- the float32 twins (the header's "float32 parameters"): the originals' arguments with the arrays untyped, the same host templates ----

cst_status cst_ans_decode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                           const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                           const void* d_a, const void* d_b, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, uint64_t* d_state, uint32_t* d_n_words_out, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_family<kAns>(cfg, family, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, f32(d_a), f32(d_b), d_symbols,
                               n_streams, n_per_stream, layout, d_state, d_n_words_out, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_decode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const uint32_t* d_words,
                                             const uint64_t* d_offsets, size_t stride_words, size_t words_capacity, const uint32_t* d_n_words,
                                             const void* d_a, const void* d_b, int32_t* d_symbols, size_t n_streams, size_t n_per_stream,
                                             cst_layout layout, cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return decode_family<kRange>(cfg, family, min_symbol, max_symbol, d_words, d_offsets, stride_words, words_capacity, d_n_words, f32(d_a), f32(d_b), d_symbols,
                                 n_streams, n_per_stream, layout, nullptr, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

} // extern "C"

namespace cst {

// Few streams, long rows (K >= 256: beyond decode_rows_wave_kernel's 256-entry rows): decode_wave_kernel's search over tabulated
// rows [K + 1], one WAVE per stream, for one piece [t0, t0 + count) of every stream -- the decoders are parked between the pieces.
struct CatPieceArgs {
    PerSymbolDecodeArgs a;
    const uint32_t* rows;       // [stream][count][K + 1]
    size_t t0, count;
    DecodeResume* resume;       // [stream]
    int32_t first, last;
};

template <int W, int S, int KIND>
__global__ __launch_bounds__(kBlock) void decode_rows_piece_wave_kernel(const CatPieceArgs ra) {
    const PerSymbolDecodeArgs& a = ra.a;
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (s >= a.n_streams) return;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const uint32_t n = (uint32_t)a.n_symbols;
    const size_t stride_t = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? a.n_streams : 1;
    int32_t* out = a.symbols + (a.layout == CST_LAYOUT_SYMBOL_MAJOR ? s : s * N) + ra.t0 * stride_t;

    DirectDecoder<W, S, KIND> D;
    int32_t status;
    if (ra.first) { D.init(a, s, raw); status = D.status; }
    else { const DecodeResume r = ra.resume[s]; D.resume(a, s, r); status = r.status; }
    for (size_t tl = 0; tl < ra.count && status == CST_STREAM_OK; ++tl) {
        const uint32_t* row = ra.rows + (s * ra.count + tl) * ((size_t)n + 1);
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
        // (a bad model's row starts with 0xffffffff: k == 0 or c > q)
        if (p == 0 || k == 0 || c > q || (uint64_t)c + p > ((uint64_t)1 << P)) { status = CST_STREAM_IMPOSSIBLE_SYMBOL; break; }
        if (lane == 0) out[tl * stride_t] = (int32_t)(base + k - 1);
        D.advance(q, c, p, P);
        D.look_ahead();
    }
    if (lane != 0) return;
    if (ra.last) { a.status[s] = status; D.finish(a, s, raw); }
    else { DecodeResume r{}; D.park(r); r.status = status; ra.resume[s] = r; }
}

template <int KIND>
void launch_decode_rows(cst_coder_config cfg, bool packed, const PerSymbolDecodeArgs& a, const uint32_t* rows, size_t t0, size_t count,
                        DecodeResume* resume, bool first, bool last, hipStream_t hs) {
    if (packed) {
        RowsDecodeArgs ra{a, reinterpret_cast<const uint4*>(rows), t0, count, resume, first, last};
        dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((decode_rows_wave_kernel<W, S, KIND>), dim3((unsigned)a.n_streams), dim3(kWave), 0, hs, ra); });
    } else {
        CatPieceArgs ra{a, rows, t0, count, resume, first, last};
        const dim3 grid((unsigned)((a.n_streams * kWave + kBlock - 1) / kBlock));
        dispatch_word_size(cfg, [&](auto W, auto S) { hipLaunchKernelGGL((decode_rows_piece_wave_kernel<W, S, KIND>), grid, dim3(kBlock), 0, hs, ra); });
    }
}
template void launch_decode_rows<kAns>(cst_coder_config, bool, const PerSymbolDecodeArgs&, const uint32_t*, size_t, size_t, DecodeResume*, bool, bool, hipStream_t);
template void launch_decode_rows<kRange>(cst_coder_config, bool, const PerSymbolDecodeArgs&, const uint32_t*, size_t, size_t, DecodeResume*, bool, bool, hipStream_t);

} // namespace cst
