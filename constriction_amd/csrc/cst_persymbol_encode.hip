// cst_persymbol_encode.hip -- the encoders of the per-symbol Gaussian, Laplace and Cauchy models (cst_persymbol.hpp has the map of the
// per-symbol files): gaussian_entries_kernel, pass 1 of the two-pass form (few streams); encode_gaussian_fused_kernel, entries and coder
// steps in one kernel (many streams), also behind the jump-point encoders; the Gaussian and family encode entry points.
#include "cst_persymbol.hpp"

namespace cst {

// (the kernels below are named after the family they were written for; FAM is a policy of cst_family_policy.hpp, and only the
// Gaussian stages the erf tables)
template <class FAM = GaussianFamily, class PT = double>
__global__ void gaussian_entries_kernel(int P, int32_t lo, int32_t hi, const int32_t* __restrict__ sym,
                                        const PT* __restrict__ mu, const PT* __restrict__ sd, size_t n,
                                        EncEntry* __restrict__ out) {
    const double2* erf_tab = nullptr;
    if constexpr (FAM::kErfTab) {
        __shared__ double2 erf_lds[kErfTabEntries];
        erf_tab_fill(erf_lds, threadIdx.x, blockDim.x);
        __syncthreads();
        erf_tab = erf_lds;
    }
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0, p = 0;
    const double m = load_param(mu + i), s = load_param(sd + i);
    // `assert!(std > 0.0)` and finite parameters (pybindings/stream/model.rs:654-657); out-of-support symbols
    // (quantize.rs:537-539) and degenerate distributions (quantize.rs:562-565) all end up with p = 0 = impossible
    if (FAM::valid(m, s)) {
        if (!FAM::lcp(sym[i], lo, hi, P, m, s, c, p, erf_tab)) p = 0;
        if (!FAM::kGaussian && (uint64_t)c + p > ((uint64_t)1 << P)) p = 0;      // (a left cumulative that ran backwards: degenerate)
    }
    out[i] = make_entry(c, p);
}

// ------------------------------------------------------------------------------------------------
// per-symbol Gaussians, ONE kernel (batches of many streams): a wave owns kFuStreams streams and alternates, tile by tile
// of kFuTile symbols, between
//   (A) all 64 lanes turning the tile's kFuStreams x kFuTile (symbol, mean, std) triples into coder entries
//       (two Gaussian cumulatives + floor(2^64 / p) each) in a wave-private LDS tile, and
//   (B) one lane per stream running the sequential coder recurrence over its row of that tile.
// Nothing but the inputs and the compressed words touches HBM: the two-pass form above writes a 16-byte entry per symbol
// and reads it back (4 GiB of scratch and 2.5x the algorithmic traffic at 65 536 x 4096).  The entry pass is the bulk of
// the work and runs with full lanes; the coder steps run on kFuStreams of the 64 lanes, which is why a wave takes 32
// streams, not 64: two waves per SIMD then cover each other's stalls.  Inputs are requested four items (~ 5000 cycles of
// arithmetic) before they are used.
// ------------------------------------------------------------------------------------------------
struct GaussianFusedArgs {
    const int32_t* symbols;
    const void* means;          // PT matrices, PT the kernel's parameter type (cst_persymbol.hpp)
    const void* stds;
    size_t n_streams, n_per_stream;
    int32_t layout, precision, lo, hi;
    uint32_t* words;
    size_t stride_words;
    uint32_t* n_words;
    uint64_t* state;
    cst_range_state* rstate;
    int32_t* status;
    uint32_t flags;
    // jump points (Pos: stack.rs:1130-1139, queue.rs:182-196), [n_streams][n_chunks], noted where a chunk of `interval` symbols starts; or
    // null.  ANS: (words in the bulk, state).  Range coder (round 6): (words emitted incl. held-back ones, lower, range).
    uint32_t* ckpt_pos;
    uint64_t* ckpt_state;
    uint64_t* ckpt_lower;
    uint64_t* ckpt_range;
    size_t interval, n_chunks;
};

//
// PAIR (stream-major matrices of whole tiles and whole waves: the launcher checks): a tile takes 64 bytes of each stream's
// symbols -- half a 128-byte line whose other half is the NEXT tile's, and asked for a tile apart the line came from HBM twice
// (6.60 GB counted against 5.57 GB algorithmic, profiles/r04_pmc_summary.md).  So the symbols of both tiles of a line are
// requested together, a pair of tiles ahead, and parked lane by lane in the ring columns of lanes 32..63 (a wave codes
// kFuStreams = 32 streams: no coder ever writes there), where the items pick them up one item ahead of their use.
// PT = float, stream-major: a tile's sixteen parameters of a stream are HALF a line too, and they are requested tile by tile -- the
// stash holds the symbols and has no room for 2 x 2 x 8 more values per lane, and registers that a rolled item loop indexes would go
// to scratch.  The f32 encoder fetches its parameter lines as the f64 one does, twice as many symbols to a line.
template <int W, int S, int KIND, bool PAIR = false, class FAM = GaussianFamily, class PT = double>
__global__ __launch_bounds__(kFuBlock) void encode_gaussian_fused_kernel(const GaussianFusedArgs a) {
    constexpr size_t kTabBytes = FAM::kErfTab ? kFuTabBytes : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1), wave_in_block = threadIdx.x >> 6;
    // LDS: [word rings, one per wave, aligned to their size: the hand-scheduled step forms slot addresses with and/or]
    //      [erf tables][entry tiles, one per wave]
    constexpr size_t kRingBytes = (size_t)kFuRingSlots * kWave * 4;
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem + (size_t)wave_in_block * kRingBytes);
    double2* erf_tab = reinterpret_cast<double2*>(smem + (kFuBlock / kWave) * kRingBytes);
    EncEntry* tile = reinterpret_cast<EncEntry*>(smem + (kFuBlock / kWave) * kRingBytes + kTabBytes + (size_t)wave_in_block * (kFuWaveBytes - kRingBytes));
    if ((lds_addr(ring) & (uint32_t)(kRingBytes - 1)) != 0) __builtin_trap();
    if constexpr (FAM::kErfTab) {
        erf_tab_fill(erf_tab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const size_t s0 = ((size_t)blockIdx.x * (kFuBlock / kWave) + wave_in_block) * kFuStreams;
    if (s0 >= a.n_streams) return;
    const size_t N = a.n_per_stream;
    const int P = a.precision;
    const bool symbol_major = a.layout == CST_LAYOUT_SYMBOL_MAJOR;
    const bool raw = (a.flags & CST_FLAG_RAW_STATE) != 0;
    const bool use_inv = KIND == kAns && W == 32 && S == 64 && P >= kInvMinPrecision;      // entries with 1 / p (make_entry_inv)
    const size_t s = s0 + lane;
    const bool active = lane < kFuStreams && s < a.n_streams;            // this lane codes a stream in phase B

    // phase A's work items: item w = it * 64 + lane of a tile is (stream j, symbol tl); consecutive lanes take consecutive
    // addresses of the input matrices in either layout.  Items are requested ONE item ahead of their use (the loop stays
    // rolled: eight unrolled copies of two erf would not fit the instruction cache).
    const size_t n_tiles = (N + kFuTile - 1) / kFuTile;
    auto tile_of = [&](size_t step) { return KIND == kAns ? n_tiles - 1 - step : step; };   // ANS codes last to first
    auto item_j = [&](int it) { const int w = it * kWave + lane; return symbol_major ? w % kFuStreams : w / kFuTile; };
    auto item_t = [&](int it) { const int w = it * kWave + lane; return symbol_major ? w / kFuStreams : w % kFuTile; };
    // a queue of kFuAhead requested items (HBM latency is two to three items' worth of arithmetic); the item loop below is
    // unrolled by kFuAhead so that every queue slot is a fixed set of registers
    int32_t sy_q[kFuAhead];
    PT mu_q[kFuAhead], sd_q[kFuAhead];              // (widened where an item takes them up: a float in flight is one register)
    bool ok_q[kFuAhead];
    const PT* const means = params_as<PT>(a.means);
    const PT* const stds = params_as<PT>(a.stds);
    // Full waves over rows of whole tiles walk the matrices by ADDING: item `it` of tile k lies at
    //   base(lane) + it * item_stride + k * tile_stride      (both strides wave-uniform, in either layout)
    // and the items are requested in exactly that order, so one running index per lane replaces the per-item index arithmetic
    // (two 64-bit multiply-adds, bounds tests and their exec masks: ~25 VALU and ~15 SALU per item).
    const bool walk = PAIR || (s0 + kFuStreams <= a.n_streams && N % kFuTile == 0);
    const int64_t item_stride = symbol_major ? (int64_t)(kWave / kFuStreams) * (int64_t)a.n_streams : (int64_t)(kWave / kFuTile) * (int64_t)N;
    const int64_t tile_stride = symbol_major ? (int64_t)kFuTile * (int64_t)a.n_streams : (int64_t)kFuTile;
    const int64_t wrap_delta = (KIND == kAns ? -tile_stride : tile_stride) - (int64_t)(kFuIters - 1) * item_stride;
    int64_t e_req = symbol_major ? (int64_t)item_t(0) * (int64_t)a.n_streams + (int64_t)(s0 + (size_t)item_j(0))
                                 : (int64_t)(s0 + (size_t)item_j(0)) * (int64_t)N + (int64_t)item_t(0);
    auto request = [&](int slot, size_t k, int it) {
        if (walk) {
            ok_q[slot] = true;
            if constexpr (!PAIR) sy_q[slot] = __builtin_nontemporal_load(a.symbols + e_req);
            mu_q[slot] = __builtin_nontemporal_load(means + e_req);
            sd_q[slot] = __builtin_nontemporal_load(stds + e_req);
            e_req += it == kFuIters - 1 ? wrap_delta : item_stride;
            return;
        }
        const size_t sj = s0 + (size_t)item_j(it), t = k * kFuTile + (size_t)item_t(it);
        ok_q[slot] = sj < a.n_streams && t < N;
        // (unconditional loads from an address that is always valid: a conditional load is waited for at once)
        const size_t e = ok_q[slot] ? (symbol_major ? t * a.n_streams + sj : sj * N + t) : 0;
        sy_q[slot] = __builtin_nontemporal_load(a.symbols + e);
        mu_q[slot] = __builtin_nontemporal_load(means + e);
        sd_q[slot] = __builtin_nontemporal_load(stds + e);
    };

    uint32_t* slab = a.words + (active ? s : 0) * a.stride_words;
    const uint32_t cap = active ? (uint32_t)(a.stride_words > 0xffffffffull ? 0xffffffffull : a.stride_words) : 0u;
    EncLane<W, S, kFuRingSlots> LA;
    RangeEncLane<W, S, kFuRingSlots> LR;
    if constexpr (KIND == kAns) {
        LA.init(slab, cap, ring, lane);
        if (raw && active) LA.state = (typename StateT<S>::type)a.state[s];
    } else {
        LR.init(slab, cap, ring, lane);
        if (raw && active) {
            const cst_range_state r = a.rstate[s];
            LR.lower = (typename StateT<S>::type)r.lower; LR.range = (typename StateT<S>::type)r.range;
            LR.inv_n = r.inverted_n; LR.inv_first = r.inverted_first;
        }
    }
    uint32_t bad = 0;

    // PAIR: the symbols of tiles 2 m and 2 m + 1 (one 128-byte line per stream), item `it` of the even tile in [0][it]
    int32_t sy_pair[2][kFuIters];
    int32_t sy_cur = 0;
    const int64_t sym_base = e_req;                           // item 0 of tile 0
    auto stash_slot = [&](int half, int it) {
        return ring + (((half * kFuIters + it) * 2 + (lane >> 5)) * kWave + kFuStreams + (lane & (kFuStreams - 1)));
    };
    auto pair_request = [&](size_t k_in_pair) {
        const size_t even = k_in_pair & ~(size_t)1, odd = even + 1 < n_tiles ? even + 1 : even;
        const int32_t* p0 = a.symbols + sym_base + (int64_t)even * tile_stride;
        const int32_t* p1 = a.symbols + sym_base + (int64_t)odd * tile_stride;
#pragma unroll
        for (int it = 0; it < kFuIters; ++it) {
            sy_pair[0][it] = __builtin_nontemporal_load(p0 + (int64_t)it * item_stride);
            sy_pair[1][it] = __builtin_nontemporal_load(p1 + (int64_t)it * item_stride);
        }
    };
    if (n_tiles > 0) {
        if constexpr (PAIR) pair_request(tile_of(0));
        e_req += (int64_t)tile_of(0) * tile_stride;
#pragma unroll
        for (int q = 0; q < kFuAhead; ++q) request(q, tile_of(0), q);
    }
    size_t step = 0;
    while (step < n_tiles) {
      // the tiles coded before the next symbol request: both tiles of a line (PAIR), or all of them
      size_t group_end = n_tiles;
      if constexpr (PAIR) {
          const size_t k = tile_of(step);
          const bool two = KIND == kAns ? (k & 1) != 0 : k + 1 < n_tiles;       // (ANS walks down: an odd tile, then its even partner)
          group_end = step + (two ? 2 : 1);
#pragma unroll
          for (int it = 0; it < kFuIters; ++it) {
              *stash_slot(0, it) = (uint32_t)sy_pair[0][it];
              *stash_slot(1, it) = (uint32_t)sy_pair[1][it];
          }
          pair_request(group_end < n_tiles ? tile_of(group_end) : k);          // (after the last pair: its own lines once more)
      }
      for (; step < group_end; ++step) {
        const size_t k = tile_of(step);
        wave_lds_fence();                                  // (the previous tile has been read)
        const uint32_t* stash_k = stash_slot((int)(k & 1), 0);
        if constexpr (PAIR) sy_cur = (int32_t)stash_k[0];
        // ---- phase A: entries of tile k ----
#pragma unroll 1
        for (int it0 = 0; it0 < kFuIters; it0 += kFuAhead) {
#pragma unroll
            for (int q = 0; q < kFuAhead; ++q) {
                const int it = it0 + q;
                int32_t sy;
                if constexpr (PAIR) {
                    sy = sy_cur;
                    sy_cur = (int32_t)stash_k[((it + 1) & (kFuIters - 1)) * 2 * kWave];     // (the next item's; wraps harmlessly)
                } else {
                    sy = ok_q[q] ? sy_q[q] : a.lo;                  // (items past the matrix: never coded)
                }
                const double m = ok_q[q] ? (double)mu_q[q] : 0.0, sg = ok_q[q] ? (double)sd_q[q] : 1.0;
                if (it + kFuAhead < kFuIters) request(q, k, it + kFuAhead);
                else if (step + 1 < n_tiles) request(q, tile_of(step + 1), it + kFuAhead - kFuIters);
                uint32_t c = 0, p = 0;
                // `assert!(std > 0.0)` and finite parameters (pybindings/stream/model.rs:654-657); out-of-support symbols
                // (quantize.rs:537-539) and degenerate distributions (quantize.rs:562-565) all end up with p = 0 = impossible.
                // No branches: invalid parameters are evaluated as (0, 1) and thrown away.
                const bool valid = FAM::valid(m, sg);
                const bool inside = FAM::lcp(sy, a.lo, a.hi, P, valid ? m : 0.0, valid ? sg : 1.0, c, p, erf_tab);
                if (!valid || !inside || (uint64_t)c + p > ((uint64_t)1 << P)) p = 0;
                EncEntry entry{c, p, 0u, 0u};                                   // (the range coder divides by nothing)
                if constexpr (KIND == kAns) entry = use_inv ? make_entry_inv(c, p) : make_entry_f64(c, p);
                tile[item_t(it) * kFuRowStride + item_j(it)] = entry;
            }
        }
        wave_lds_fence();
        // ---- phase B: every stream's lane over its row ----
        const size_t t0 = k * kFuTile;
        const int n_here = (int)(N - t0 < (size_t)kFuTile ? N - t0 : (size_t)kFuTile);
        if constexpr (KIND == kRange) {
            // RangeEncoder::pos() in front of a chunk (a queue: BEFORE the chunk's first symbol is encoded; chunks are whole tiles)
            if (a.ckpt_pos && active && t0 % a.interval == 0) {
                a.ckpt_pos[s * a.n_chunks + t0 / a.interval] = LR.out.wr + LR.inv_n;
                a.ckpt_lower[s * a.n_chunks + t0 / a.interval] = (uint64_t)LR.lower;
                a.ckpt_range[s * a.n_chunks + t0 / a.interval] = (uint64_t)LR.range;
            }
        }
        if (active) {
            if constexpr (KIND == kAns) {
                constexpr bool FAST = W == 32 && S == 64;            // the 32-bit-halves step (8 <= P)
                if (FAST && P >= 8 && n_here == kFuTile) {
                    // a whole tile: all sixteen entries first (one LDS wait), then sixteen hand-scheduled steps.  An
                    // impossible symbol is coded as (0, 1) -- its stream is flagged and its words are never used.
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
                    // (other presets, P < 8, the ragged tile)
                    for (int tl = n_here - 1; tl >= 0; --tl) {
                        const EncEntry e = tile[tl * kFuRowStride + lane];
                        if (e.p == 0) bad = 1;
                        else if (!bad) LA.template step<false>(use_inv ? make_entry(e.c, e.p) : e, P);
                    }
                }
            } else if (n_here == kFuTile) {
                // a whole tile: all sixteen (c, p) first (one LDS wait), then sixteen steps; an impossible symbol is coded as
                // (0, 1) -- its stream is flagged and its words are never used
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
                for (int tl = 0; tl < n_here; ++tl) {
                    const EncEntry e = tile[tl * kFuRowStride + lane];
                    if (e.p == 0) bad = 1;
                    else if (!bad) LR.step(e.c, e.p, P);
                }
            }
        }
        if constexpr (KIND == kAns) {
            // AnsCoder::pos() in front of a chunk: the symbols from t0 on are encoded (chunks are whole tiles: the launcher checks)
            if (a.ckpt_pos && active && t0 % a.interval == 0) {
                a.ckpt_pos[s * a.n_chunks + t0 / a.interval] = LA.out.wr;
                a.ckpt_state[s * a.n_chunks + t0 / a.interval] = (uint64_t)LA.state;
            }
        }
        // at most kFuTile new words per stream and tile: whole chunks leave here (<= 19 pending before, < 4 after)
        if constexpr (KIND == kAns) LA.flush_chunks(); else LR.out.flush_chunks();
      }
    }

    uint32_t n_words = 0;
    int32_t status;
    if constexpr (KIND == kAns) {
        status = LA.finish(!raw, 1u, n_words);
        if (active && raw) a.state[s] = (uint64_t)LA.state;
    } else if (raw) {
        LR.out.drain();
        n_words = LR.out.wr;
        status = LR.out.wr > LR.out.cap ? CST_STREAM_CAPACITY : CST_STREAM_OK;
        if (active) {
            cst_range_state r = a.rstate[s];
            r.lower = (uint64_t)LR.lower; r.range = (uint64_t)LR.range; r.inverted_n = LR.inv_n; r.inverted_first = LR.inv_first;
            a.rstate[s] = r;
        }
    } else {
        status = LR.finish(1u, n_words);
    }
    if (!active) return;
    if (bad) status = CST_STREAM_IMPOSSIBLE_SYMBOL;
    a.status[s] = status;
    a.n_words[s] = status == CST_STREAM_OK ? n_words : 0u;
}

// ---- host side ----
// The fused kernel pays one coder step per kFuStreams-stream wave and symbol whatever the batch; the two-pass form runs its
// entry pass on the whole chip however few streams there are.  From 16 384 streams on (512 waves of 32 streams: two
// for every SIMD pair) the fused kernel is the faster one; below, and for the one long stream of the drop-in API, two passes.
// (CST_FUSED_MIN_STREAMS in the environment moves the threshold: the parity tests run the fused kernel on small batches.)
static bool fused_encode_usable(size_t n_streams, size_t n_per_stream) {
    return n_streams >= knobs().fused_min_streams && n_per_stream >= 1;
}

template <int KIND, class FAM = GaussianFamily, class PT = double>
static cst_status encode_gaussian_fused(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                        const PT* d_means, const PT* d_stds, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                        uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, uint64_t* d_state,
                                        cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, hipStream_t hs,
                                        size_t ckpt_interval = 0, uint32_t* d_ckpt_pos = nullptr, uint64_t* d_ckpt_state = nullptr,
                                        uint64_t* d_ckpt_lower = nullptr, uint64_t* d_ckpt_range = nullptr) {
    if (cst_status st = check_common(cfg, layout)) return st;
    if (!d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (raw_state_missing<KIND>(flags, d_state, d_rstate)) return CST_ERR_INVALID_ARGUMENT;
    GaussianFusedArgs a{};
    if (ckpt_interval) {
        a.ckpt_pos = d_ckpt_pos; a.ckpt_state = d_ckpt_state; a.ckpt_lower = d_ckpt_lower; a.ckpt_range = d_ckpt_range; a.interval = ckpt_interval;
        a.n_chunks = (n_per_stream + ckpt_interval - 1) / ckpt_interval;
    }
    a.symbols = d_symbols; a.means = d_means; a.stds = d_stds; a.n_streams = n_streams; a.n_per_stream = n_per_stream;
    a.layout = layout; a.precision = cfg.precision; a.lo = min_symbol; a.hi = max_symbol;
    a.words = d_words; a.stride_words = stride_words; a.n_words = d_n_words; a.state = d_state; a.rstate = d_rstate;
    a.status = d_status; a.flags = flags;
    const size_t per_block = (size_t)(kFuBlock / kWave) * kFuStreams;
    const size_t blocks = (n_streams + per_block - 1) / per_block;
    const size_t lds = (FAM::kErfTab ? kFuTabBytes : 0) + (size_t)(kFuBlock / kWave) * kFuWaveBytes;
    // (PAIR saves a second fetch of the symbols' lines -- a fifth of the Gaussian's traffic.  The exact CDFs of the other families
    // are arithmetic, not traffic, and the pair's sixteen parked symbols do not survive their calls without scratch.)
    const bool pair = FAM::kGaussian && layout == CST_LAYOUT_STREAM_MAJOR && n_streams % kFuStreams == 0 && n_per_stream % kFuTile == 0 && n_per_stream > 0;
    if constexpr (FAM::kGaussian)
        if (cfg.word_bits == 32 && pair) return launch_with_lds(encode_gaussian_fused_kernel<32, 64, KIND, true, FAM, PT>, blocks, kFuBlock, lds, a, hs);
    return dispatch_word_size(cfg, [&](auto W, auto S) { return launch_with_lds(encode_gaussian_fused_kernel<W, S, KIND, false, FAM, PT>, blocks, kFuBlock, lds, a, hs); });
}

// the routes of a rectangular encode call of family FAM; d_a / d_b are the family's two parameters; `note`: record the route
template <int KIND, class FAM, class PT>
static cst_status encode_family(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols, const PT* d_a,
                                const PT* d_b, size_t n_streams, size_t n_per_stream, cst_layout layout, uint32_t* d_words,
                                size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, cst_range_state* d_rstate, int32_t* d_status,
                                uint32_t flags, hipStream_t hs, bool note = true) {
    const bool fused = fused_encode_usable(n_streams, n_per_stream);
    // (`note` is false for one f64 call that has never recorded its route; the float calls all do)
    if (note || kParamF32<PT>) note_kernel(fused ? FamilyNames<FAM, PT>::fused[KIND == kRange] : FamilyNames<FAM, PT>::two_pass[KIND == kRange], CST_OK);
    if (fused)
        return encode_gaussian_fused<KIND, FAM, PT>(cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, n_streams, n_per_stream, layout, d_words,
                                                stride_words, d_n_words, d_state, d_rstate, d_status, flags, hs);
    return encode_two_pass<KIND>(cfg, n_streams, n_per_stream, layout, d_words, stride_words, d_n_words, d_state, d_rstate, d_status, flags, hs,
                                 [&](EncEntry* out, size_t n) {
        hipLaunchKernelGGL((gaussian_entries_kernel<FAM, PT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, cfg.precision, min_symbol, max_symbol,
                           d_symbols, d_a, d_b, n, out);
    });
}

} // namespace cst

using namespace cst;

template <class PT>
static cst_status ans_encode_gaussian_batch_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                 const PT* d_means, const PT* d_stds, size_t n_streams, size_t n_per_stream,
                                                 cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                 uint64_t* d_state, int32_t* d_status, uint32_t flags, void* stream) {
    if (n_per_stream > 0 && (!d_symbols || !d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol || support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;
    return encode_family<kAns, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
                                               stride_words, d_n_words, d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

extern "C" {

cst_status cst_ans_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                         const double* d_means, const double* d_stds, size_t n_streams, size_t n_per_stream,
                                         cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                         uint64_t* d_state, int32_t* d_status, uint32_t flags, void* stream) {
    return ans_encode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
           stride_words, d_n_words, d_state, d_status, flags, stream);
}
cst_status cst_ans_encode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                             const void* d_means, const void* d_stds, size_t n_streams, size_t n_per_stream,
                                             cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                             uint64_t* d_state, int32_t* d_status, uint32_t flags, void* stream) {
    return ans_encode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), n_streams, n_per_stream, layout, d_words,
           stride_words, d_n_words, d_state, d_status, flags, stream);
}

} // extern "C"

template <class PT>
static cst_status range_encode_gaussian_batch_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                   const PT* d_means, const PT* d_stds, size_t n_streams, size_t n_per_stream,
                                                   cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                   cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    if (n_per_stream > 0 && (!d_symbols || !d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol || support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;
    // (this call has never recorded its route with note_kernel())
    return encode_family<kRange, GaussianFamily>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
                                                 stride_words, d_n_words, nullptr, d_rstate, d_status, flags, (hipStream_t)stream, false);
}

extern "C" {

cst_status cst_range_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                           const double* d_means, const double* d_stds, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                           cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return range_encode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
           stride_words, d_n_words, d_rstate, d_status, flags, stream);
}
cst_status cst_range_encode_gaussian_batch_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                               const void* d_means, const void* d_stds, size_t n_streams, size_t n_per_stream,
                                               cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                               cst_range_state* d_rstate, int32_t* d_status, uint32_t flags, void* stream) {
    return range_encode_gaussian_batch_impl(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), n_streams, n_per_stream, layout,
           d_words, stride_words, d_n_words, d_rstate, d_status, flags, stream);
}

// Jump points for the reference's flagship call (every symbol its own (mean, std)): the fused encoder notes AnsCoder::pos() in
// front of every chunk of `ckpt_interval` symbols (a multiple of the kernel's 16-symbol tile), and the decoder runs every
// (stream, chunk) pair as a coder of its own -- the per-symbol parameters are a matrix of the symbols' shape, so chunk j of stream
// s is row s * n_chunks + j of all three matrices viewed as [n_streams * n_chunks][interval].  What that buys: the lane decoder of
// 65 536 streams is ONE wave per SIMD and spends a third of its cycles waiting; with two jump points per stream the small-geometry
// kernel (LaneGeo<true>) runs two.
} // extern "C"

template <class PT>
static cst_status ans_encode_gaussian_batch_ckpt_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                      const PT* d_means, const PT* d_stds, size_t n_streams, size_t n_per_stream,
                                                      cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                      size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_state, int32_t* d_status, void* stream) {
    if (n_per_stream > 0 && (!d_symbols || !d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if (!d_ckpt_pos || !d_ckpt_state || ckpt_interval == 0 || ckpt_interval % kFuTile != 0 || n_per_stream % ckpt_interval != 0) return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol || support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;
    if (n_streams == 0) return CST_OK;
    return note_kernel(FamilyNames<GaussianFamily, PT>::fused_ckpt[0], encode_gaussian_fused<kAns, GaussianFamily, PT>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words, stride_words,
                                       d_n_words, nullptr, nullptr, d_status, CST_FLAG_NONE, (hipStream_t)stream, ckpt_interval, d_ckpt_pos, d_ckpt_state));
}

extern "C" {

cst_status cst_ans_encode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                              const double* d_means, const double* d_stds, size_t n_streams, size_t n_per_stream,
                                              cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                              size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_state, int32_t* d_status, void* stream) {
    return ans_encode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
           stride_words, d_n_words, ckpt_interval, d_ckpt_pos, d_ckpt_state, d_status, stream);
}
cst_status cst_ans_encode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                  const void* d_means, const void* d_stds, size_t n_streams, size_t n_per_stream,
                                                  cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                  size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_state, int32_t* d_status, void* stream) {
    return ans_encode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), n_streams, n_per_stream, layout,
           d_words, stride_words, d_n_words, ckpt_interval, d_ckpt_pos, d_ckpt_state, d_status, stream);
}

// ... and for the range coder (round 6): the fused encoder notes RangeEncoder::pos() in front of every chunk, the decoder builds the
// RangeDecoder::seek states of the (stream, chunk) pairs (point re-read at the jump point: range_ckpt_virtual_state) and runs them as
// streams of their own -- the small-geometry lane decoder, two waves per SIMD, where the plain decoder of 65 536 streams has one
} // extern "C"

template <class PT>
static cst_status range_encode_gaussian_batch_ckpt_impl(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                        const PT* d_means, const PT* d_stds, size_t n_streams, size_t n_per_stream,
                                                        cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                        size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_lower, uint64_t* d_ckpt_range,
                                                        int32_t* d_status, void* stream) {
    if (n_per_stream > 0 && (!d_symbols || !d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if (!d_ckpt_pos || !d_ckpt_lower || !d_ckpt_range || ckpt_interval == 0 || ckpt_interval % kFuTile != 0 || n_per_stream % ckpt_interval != 0)
        return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol || support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;
    if (n_streams == 0) return CST_OK;
    return note_kernel(FamilyNames<GaussianFamily, PT>::fused_ckpt[1],
                       encode_gaussian_fused<kRange, GaussianFamily, PT>(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
                                                     stride_words, d_n_words, nullptr, nullptr, d_status, CST_FLAG_NONE, (hipStream_t)stream, ckpt_interval,
                                                     d_ckpt_pos, nullptr, d_ckpt_lower, d_ckpt_range));
}

extern "C" {

cst_status cst_range_encode_gaussian_batch_ckpt(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                const double* d_means, const double* d_stds, size_t n_streams, size_t n_per_stream,
                                                cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_lower, uint64_t* d_ckpt_range,
                                                int32_t* d_status, void* stream) {
    return range_encode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_symbols, d_means, d_stds, n_streams, n_per_stream, layout, d_words,
           stride_words, d_n_words, ckpt_interval, d_ckpt_pos, d_ckpt_lower, d_ckpt_range, d_status, stream);
}
cst_status cst_range_encode_gaussian_batch_ckpt_f32(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                                    const void* d_means, const void* d_stds, size_t n_streams, size_t n_per_stream,
                                                    cst_layout layout, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                                    size_t ckpt_interval, uint32_t* d_ckpt_pos, uint64_t* d_ckpt_lower, uint64_t* d_ckpt_range,
                                                    int32_t* d_status, void* stream) {
    return range_encode_gaussian_batch_ckpt_impl(cfg, min_symbol, max_symbol, d_symbols, f32(d_means), f32(d_stds), n_streams, n_per_stream, layout,
           d_words, stride_words, d_n_words, ckpt_interval, d_ckpt_pos, d_ckpt_lower, d_ckpt_range, d_status, stream);
}

cst_status cst_chain_encode_gaussian_batch(cst_coder_config cfg, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                           const double* d_means, const double* d_stds, size_t n_streams, size_t n_per_stream,
                                           cst_layout layout, const uint32_t* d_pop_words, const uint64_t* d_pop_offsets, size_t pop_stride,
                                           uint32_t* d_n_pop, uint32_t* d_push_words, size_t push_stride, uint32_t* d_n_push,
                                           cst_chain_heads* d_heads, int32_t* d_status, void* stream) {
    if (n_per_stream > 0 && (!d_symbols || !d_means || !d_stds)) return CST_ERR_INVALID_ARGUMENT;
    if (max_symbol <= min_symbol || support_too_large(cfg, min_symbol, max_symbol)) return CST_ERR_MODEL;
    hipStream_t hs = (hipStream_t)stream;
    return chain_encode_common(cfg, n_streams, n_per_stream, layout, d_pop_words, d_pop_offsets, pop_stride, d_n_pop, d_push_words, push_stride,
                               d_n_push, d_heads, d_status, hs, [&](EncEntry* out, size_t n) {
        hipLaunchKernelGGL(gaussian_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, cfg.precision, min_symbol,
                           max_symbol, d_symbols, d_means, d_stds, n, out);
    });
}

cst_status cst_ans_encode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                       const double* d_a, const double* d_b, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                       uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status,
                                       uint32_t flags, void* stream) {
    if (cst_status st = check_family_args(cfg, family, min_symbol, max_symbol, layout, d_symbols, d_a, d_b, d_words, d_n_words, d_status, d_state, flags))
        return st;
    return CST_FAMILY_CALL(encode_family, kAns, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, n_streams, n_per_stream, layout, d_words, stride_words,
                           d_n_words, d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_encode_family_batch(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                         const double* d_a, const double* d_b, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                         uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status,
                                         uint32_t flags, void* stream) {
    if (cst_status st = check_family_args(cfg, family, min_symbol, max_symbol, layout, d_symbols, d_a, d_b, d_words, d_n_words, d_status, d_rstate, flags))
        return st;
    return CST_FAMILY_CALL(encode_family, kRange, cfg, min_symbol, max_symbol, d_symbols, d_a, d_b, n_streams, n_per_stream, layout, d_words, stride_words,
                           d_n_words, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

// ---- the float32 twins (the header's "float32 parameters"): the originals' arguments with the arrays untyped, the same host templates ----

cst_status cst_ans_encode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                           const void* d_a, const void* d_b, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                           uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, uint64_t* d_state, int32_t* d_status,
                                           uint32_t flags, void* stream) {
    if (cst_status st = check_family_args(cfg, family, min_symbol, max_symbol, layout, d_symbols, f32(d_a), f32(d_b), d_words, d_n_words, d_status, d_state, flags))
        return st;
    return CST_FAMILY_CALL(encode_family, kAns, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), n_streams, n_per_stream, layout, d_words, stride_words,
                           d_n_words, d_state, nullptr, d_status, flags, (hipStream_t)stream);
}

cst_status cst_range_encode_family_batch_f32(cst_coder_config cfg, int32_t family, int32_t min_symbol, int32_t max_symbol, const int32_t* d_symbols,
                                             const void* d_a, const void* d_b, size_t n_streams, size_t n_per_stream, cst_layout layout,
                                             uint32_t* d_words, size_t stride_words, uint32_t* d_n_words, cst_range_state* d_rstate, int32_t* d_status,
                                             uint32_t flags, void* stream) {
    if (cst_status st = check_family_args(cfg, family, min_symbol, max_symbol, layout, d_symbols, f32(d_a), f32(d_b), d_words, d_n_words, d_status, d_rstate, flags))
        return st;
    return CST_FAMILY_CALL(encode_family, kRange, cfg, min_symbol, max_symbol, d_symbols, f32(d_a), f32(d_b), n_streams, n_per_stream, layout, d_words, stride_words,
                           d_n_words, nullptr, d_rstate, d_status, flags, (hipStream_t)stream);
}

} // extern "C"
