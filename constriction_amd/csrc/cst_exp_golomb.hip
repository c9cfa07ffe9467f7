// cst_exp_golomb.hip -- Exponential-Golomb symbol codes (the reference's constriction.symbol: src/symbol/exp_golomb.rs with the bit
// containers of src/symbol/mod.rs): batched and ragged stack / queue coders and the exact bit count that sizes their slabs.
//
// The codeword of a symbol x of an unsigned type of B bits: m = x + 1, len = floor(log2 m); in prefix order len zeros, then the
// len + 1 bits of m from the most significant down (2 len + 1 bits).  x = N::MAX wraps in the reference (m == 0) and codes as B zeros,
// a one, B zeros; here m is kept one bit wider than N, so that m = 2^B, len = B is the same rule and not a special case.
// A queue writes prefix order, symbols front to back, no seal; a stack writes every codeword reversed (suffix order), a stream's
// symbols back to front, and one seal bit.  Bits fill u32 words from bit 0 upwards, as in cst_huffman.hip, whose kernels these
// follow: one lane per stream, a 64-bit accumulator (encoder) or window (decoder), symbols through wave-private LDS tiles, words in
// 16-byte groups.  There is no table: the length is a count-leading-zeros of m, the zero run a find-first-set of the window.
#include <algorithm>
#include <type_traits>

#include "cst_symbol_select.hpp"

namespace cst {

namespace {

struct EgEncArgs {
    const void* symbols;
    size_t n_streams, n_per;
    uint32_t* words;
    size_t stride;
    uint32_t* n_words;
    uint64_t* n_bits;
    uint64_t* cont;
    int32_t* status;
    bool vec;          // slabs 16-byte aligned: words leave in 16-byte groups
};

struct EgDecArgs {
    const uint32_t* words;
    const uint64_t* offsets;
    size_t stride, capacity;
    const uint32_t* n_words;
    void* symbols;
    size_t n_streams, n_per;
    uint64_t* cont;
    uint32_t* n_words_out;
    int32_t* status;
};

struct EgRaggedEncArgs {
    const void* symbols;
    const uint64_t* sym_offsets;
    size_t n_streams;
    uint32_t* words;
    const uint64_t* word_offsets;
    size_t stride;
    uint32_t* n_words;
    uint64_t* n_bits;
    int32_t* status;
    bool vec;          // d_words 16-byte aligned: a slab that starts at a multiple of four words stores 16-byte groups
};

struct EgRaggedDecArgs {
    const uint32_t* words;
    const uint64_t* word_offsets;
    size_t stride, capacity;
    const uint32_t* n_words;
    void* symbols;
    const uint64_t* sym_offsets;
    size_t n_streams;
    int32_t* status;
};

template <int SB>
__device__ inline uint32_t eg_load(const void* base, size_t i) {
    if constexpr (SB == 1) return static_cast<const uint8_t*>(base)[i];
    else if constexpr (SB == 2) return static_cast<const uint16_t*>(base)[i];
    else return static_cast<const uint32_t*>(base)[i];
}

template <int SB>
__device__ inline void eg_store(void* base, size_t i, uint32_t v) {
    if constexpr (SB == 1) static_cast<uint8_t*>(base)[i] = (uint8_t)v;
    else if constexpr (SB == 2) static_cast<uint16_t*>(base)[i] = (uint16_t)v;
    else static_cast<uint32_t*>(base)[i] = v;
}

// wave-private LDS tiles: 64 stream rows x kEgTile symbols, row stride kEgTileStride words (conflict-free for the row-wise fill and
// for the lane-per-row reads): the layout of the Huffman kernels' tiles
constexpr int kEgTile = 32;
constexpr int kEgTileStride = kEgTile + 1;
constexpr int kEgTileWords = (kBlock / kWave) * kWave * kEgTileStride;

__device__ __forceinline__ void eg_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// symbols [t0, t0 + tlen) of the wave's 64 rows -> tile.  Lane l reads column (l & 31) of rows (l >> 5) + 2k: every load instruction
// reads two contiguous row segments
template <int SB>
__device__ __forceinline__ void eg_tile_fill(const void* sym, size_t n_streams, size_t n, size_t s0, size_t t0, uint32_t tlen, int lane,
                                             uint32_t* tile) {
    const uint32_t col = (uint32_t)lane & 31u;
    uint32_t r[kEgTile / 2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int k = 0; k < kEgTile / 2; ++k) {
            const int row = (lane >> 5) + 2 * (k + half * (kEgTile / 2));
            const size_t s = s0 + (size_t)row;
            r[k] = (s < n_streams && col < tlen) ? eg_load<SB>(sym, s * n + t0 + col) : 0u;
        }
#pragma unroll
        for (int k = 0; k < kEgTile / 2; ++k) tile[((lane >> 5) + 2 * (k + half * (kEgTile / 2))) * kEgTileStride + col] = r[k];
    }
}

// tile -> symbols [t0, t0 + tlen) of the wave's 64 rows (the mirror image of eg_tile_fill)
template <int SB>
__device__ __forceinline__ void eg_tile_drain(void* sym, size_t n_streams, size_t n, size_t s0, size_t t0, uint32_t tlen, int lane,
                                              const uint32_t* tile) {
    const uint32_t col = (uint32_t)lane & 31u;
#pragma unroll 8
    for (int k = 0; k < kWave / 2; ++k) {
        const int row = (lane >> 5) + 2 * k;
        const size_t s = s0 + (size_t)row;
        if (s < n_streams && col < tlen) eg_store<SB>(sym, s * n + t0 + col, tile[row * kEgTileStride + col]);
    }
}

// A lane's compressed words on their way to its slab: four at a time as one 16-byte store where the slab is 16-byte aligned, else
// one by one.  `cap` bounds every store.
struct EgWordSink {
    uint32_t* out;
    size_t cap;
    uint32_t nw;      // words emitted (stored or held)
    uint4 grp;
    bool vec;

    __device__ __forceinline__ bool put(uint32_t w) {
        if (nw >= cap) return false;
        if (!vec) { out[nw++] = w; return true; }
        const uint32_t c = nw & 3u;
        grp.x = c == 0 ? w : grp.x;
        grp.y = c == 1 ? w : grp.y;
        grp.z = c == 2 ? w : grp.z;
        grp.w = c == 3 ? w : grp.w;
        ++nw;
        if (c == 3) *reinterpret_cast<uint4*>(out + (nw - 4)) = grp;
        return true;
    }
    __device__ __forceinline__ void finish() {    // the words of an incomplete last group
        if (!vec) return;
        const uint32_t c = nw & 3u, b = nw - c;
        if (c > 0) out[b] = grp.x;
        if (c > 1) out[b + 1] = grp.y;
        if (c > 2) out[b + 2] = grp.z;
    }
};

// m = x + 1 without the wrap and len = floor(log2 m) <= B
template <int SB>
__device__ __forceinline__ uint32_t eg_len(uint32_t x, uint64_t& m) {
    m = (uint64_t)x + 1u;
    if constexpr (SB == 4) return 63u - (uint32_t)__clzll((long long)m);
    else return 31u - (uint32_t)__clz((int)(uint32_t)m);
}

// appends `len` (<= 33) bits to the (<= 31) pending ones; emits the words that fill up.  false: the slab is full
__device__ __forceinline__ bool eg_put_bits(uint64_t code, uint32_t len, uint64_t& acc, uint32_t& nb, EgWordSink& sink) {
    acc |= code << nb;          // nb + len <= 64
    nb += len;
    if (nb >= 32) {
        if (!sink.put((uint32_t)acc)) return false;
        acc >>= 32;
        nb -= 32;
        if (nb >= 32) {         // (31 pending + 33 new bits)
            if (!sink.put((uint32_t)acc)) return false;
            acc >>= 32;
            nb -= 32;
        }
    }
    return true;
}

// One codeword.  In write order (bit 0 first) the stack's codeword is m itself under len zeros, the queue's is len zeros under m
// bit-reversed.  Up to len = 16 the 2 len + 1 bits go in one piece; a longer codeword (u32 symbols from 2^17 - 1 on, up to 65 bits) does
// not fit beside 31 pending bits and goes as two pieces, the value (len + 1 <= 33 bits) and the zero run (len <= 32).
template <bool STACK, int SB>
__device__ __forceinline__ bool eg_put_symbol(uint32_t x, uint64_t& acc, uint32_t& nb, EgWordSink& sink) {
    uint64_t m;
    const uint32_t len = eg_len<SB>(x, m);
    if constexpr (STACK) {
        if (SB < 4 || len <= 16) return eg_put_bits(m, 2 * len + 1, acc, nb, sink);
        return eg_put_bits(m, len + 1, acc, nb, sink) && eg_put_bits(0ull, len, acc, nb, sink);
    } else {
        uint64_t rev;           // the len + 1 bits of m, most significant first
        if constexpr (SB == 4) rev = __builtin_bitreverse64(m) >> (63 - len);
        else rev = __builtin_bitreverse32((uint32_t)m) >> (31 - len);
        if (SB < 4 || len <= 16) return eg_put_bits(rev << len, 2 * len + 1, acc, nb, sink);
        return eg_put_bits(0ull, len, acc, nb, sink) && eg_put_bits(rev, len + 1, acc, nb, sink);
    }
}

// seal (stack) and the partial word, then the counts.  `bits`: the written bits before the seal (the reference's len())
template <bool STACK>
__device__ __forceinline__ int32_t eg_finish(int32_t st, bool open, uint64_t& acc, uint32_t& nb, EgWordSink& sink) {
    if (st == CST_STREAM_OK && !open) {
        if (STACK && !eg_put_bits(1ull, 1u, acc, nb, sink)) st = CST_STREAM_CAPACITY;
        if (st == CST_STREAM_OK && nb > 0 && !sink.put((uint32_t)acc)) st = CST_STREAM_CAPACITY;
    }
    if (st == CST_STREAM_OK) sink.finish();
    return st;
}

template <bool STACK, int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_encode_kernel(EgEncArgs a) {
    __shared__ uint32_t s_tiles[kEgTileWords];
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s0 = (size_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1));
    if (s0 >= a.n_streams) return;                  // (wave-uniform: the whole wave lies past the batch)
    uint32_t* tile = s_tiles + (size_t)(threadIdx.x / kWave) * kWave * kEgTileStride;
    const size_t s = s0 + (size_t)lane;
    const bool valid = s < a.n_streams;
    EgWordSink sink{valid ? a.words + s * a.stride : nullptr, valid ? a.stride : 0, 0u, make_uint4(0, 0, 0, 0), a.vec};
    uint64_t acc = 0;
    uint32_t nb = 0;
    int32_t st = valid ? CST_STREAM_OK : CST_STREAM_INVALID_DATA;
    if (valid && a.cont) {
        const uint64_t c = a.cont[s];
        nb = (uint32_t)(c >> 32);
        acc = c & 0xffffffffull;
        if (nb >= 32) { st = CST_STREAM_INVALID_DATA; nb = 0; acc = 0; }
        else acc &= (1ull << nb) - 1;
    }
    const size_t n = a.n_per;
    const uint32_t* my = tile + lane * kEgTileStride;
    for (size_t done = 0; done < n; done += kEgTile) {
        // queue: tiles front to back; stack: back to front, each read from its end
        const size_t t0 = STACK ? (n - done > (size_t)kEgTile ? n - done - kEgTile : 0) : done;
        const uint32_t tlen = (uint32_t)((n - done) < (size_t)kEgTile ? (n - done) : (size_t)kEgTile);
        eg_lds_fence();
        eg_tile_fill<SB>(a.symbols, a.n_streams, n, s0, t0, tlen, lane, tile);
        eg_lds_fence();
        if (st != CST_STREAM_OK) continue;
        for (uint32_t j = 0; j < tlen; ++j) {
            if (!eg_put_symbol<STACK, SB>(my[STACK ? tlen - 1 - j : j], acc, nb, sink)) { st = CST_STREAM_CAPACITY; break; }
        }
    }
    if (!valid) return;
    const uint64_t bits = 32ull * sink.nw + nb;
    st = eg_finish<STACK>(st, a.cont != nullptr, acc, nb, sink);
    if (st != CST_STREAM_OK) {
        a.n_words[s] = 0;
        if (a.n_bits) a.n_bits[s] = 0;
    } else {
        a.n_words[s] = sink.nw;
        if (a.n_bits) a.n_bits[s] = bits;
        if (a.cont) a.cont[s] = (acc & 0xffffffffull) | ((uint64_t)nb << 32);
    }
    a.status[s] = st;
}

// A lane's read side: a 64-bit window of the next bits (queue: from bit 0 up; stack: from bit 63 down; the bits beyond `have` are
// zero), refilled a word at a time, the next word loaded one refill ahead.
template <bool STACK>
struct EgReader {
    const uint32_t* w;
    size_t nw;        // words of the stream
    size_t wi;        // queue: next word to load; stack: words below the window still to load
    uint64_t buf;
    uint32_t have;    // valid bits in buf
    uint32_t pf;      // the next word to enter the window

    // from the words alone (cont == nullptr) or from a continued container.  false: not a container
    __device__ __forceinline__ bool open(const uint32_t* words, size_t n_words, const uint64_t* cont) {
        w = words; nw = n_words; wi = 0; buf = 0; have = 0; pf = 0;
        if (STACK) {
            if (cont) {
                const uint64_t c = *cont;
                have = (uint32_t)(c >> 32);
                if (have >= 32) { have = 0; return false; }
                buf = have ? (uint64_t)(uint32_t)c << (64 - have) : 0ull;
                wi = nw;
            } else {
                if (nw == 0 || w[nw - 1] == 0u) return false;       // no words, or a zero last word: no seal
                const uint32_t last = w[nw - 1];                    // the seal is the HIGHEST set bit of the last word
                have = 31u - (uint32_t)__clz((int)last);
                buf = have ? (uint64_t)last << (64 - have) : 0ull;
                wi = nw - 1;
            }
            pf = wi > 0 ? w[wi - 1] : 0u;
        } else {
            const uint64_t p = cont ? *cont : 0ull;
            if (p > 32ull * nw) return false;
            wi = (size_t)(p >> 5);
            if ((p & 31u) != 0) {
                buf = w[wi++] >> (p & 31u);
                have = 32u - (uint32_t)(p & 31u);
            }
            pf = wi < nw ? w[wi] : 0u;
        }
        return true;
    }
    __device__ __forceinline__ void close() { nw = 0; wi = 0; buf = 0; have = 0; pf = 0; }

    // the highest bit index a reader may start at: 32 n_words of a queue, the position of a stack's seal.  false: a stack without
    // words or with a zero last word
    __device__ __forceinline__ static bool limit(const uint32_t* words, size_t n_words, uint64_t& bits) {
        return symbol_bit_limit<STACK>(words, n_words, bits);
    }

    // at bit index p <= limit(): a queue reads p, p + 1, ...; a stack p - 1, p - 2, ...
    __device__ __forceinline__ void seek(const uint32_t* words, size_t n_words, uint64_t p) {
        w = words; nw = n_words; buf = 0;
        wi = (size_t)(p >> 5);
        const uint32_t r = (uint32_t)(p & 31u);
        if (STACK) {
            have = r;
            if (r) buf = (uint64_t)w[wi] << (64 - r);       // (the bits from p upwards leave the window at its top)
            pf = wi > 0 ? w[wi - 1] : 0u;
        } else {
            have = 0;
            if (r) { buf = w[wi++] >> r; have = 32u - r; }
            pf = wi < nw ? w[wi] : 0u;
        }
    }

    // at least 33 valid bits, or all that is left of the stream
    __device__ __forceinline__ void refill() {
        if (STACK) {
            while (have <= 32 && wi > 0) {
                buf |= (uint64_t)pf << (32 - have); have += 32; --wi;
                pf = wi > 0 ? w[wi - 1] : 0u;
            }
        } else {
            while (have <= 32 && wi < nw) {
                buf |= (uint64_t)pf << have; have += 32; ++wi;
                pf = wi < nw ? w[wi] : 0u;
            }
        }
    }

    // exp_golomb.rs:135-171.  false: an invalid codeword (the zero run or the value runs out of bits, len > B, or len == B with a
    // value that is not zero)
    template <int SB>
    __device__ __forceinline__ bool decode(uint32_t& sym) {
        constexpr uint32_t B = 8u * SB;
        refill();
        const uint32_t len = buf == 0 ? 64u : (uint32_t)(STACK ? __clzll((long long)buf) : __builtin_ctzll(buf));
        if (len >= have || len > B) return false;       // (no one among the valid bits: they ran out, or the run is longer than 33 > B)
        buf = STACK ? buf << (len + 1) : buf >> (len + 1);
        have -= len + 1;
        if constexpr (SB == 4) {
            if (have < len) refill();                   // (a codeword of more than 33 bits)
        }
        if (have < len) return false;
        uint32_t v = 0;                                 // the len bits below m's leading one
        if (len) v = STACK ? (uint32_t)(buf >> (64 - len)) : __builtin_bitreverse32((uint32_t)buf) >> (32 - len);
        buf = STACK ? buf << len : buf >> len;
        have -= len;
        if (len == B && v != 0u) return false;
        sym = ((uint32_t)(1ull << len) | v) - 1u;       // (len == 32: 0 - 1 = u32::MAX)
        return true;
    }

    // what the container holds after the symbols read: d_cont / d_n_words_out of the batch decoders
    __device__ __forceinline__ void position(uint64_t& cont, uint32_t& n_words_out) const {
        if (STACK) {
            const uint64_t remaining = 32ull * wi + have;
            const uint32_t r = (uint32_t)(remaining & 31u);
            n_words_out = (uint32_t)(remaining >> 5);
            cont = r ? ((buf >> (64 - r)) | ((uint64_t)r << 32)) : 0ull;
        } else {
            const uint64_t pos = 32ull * wi - have;
            n_words_out = (uint32_t)((pos + 31) >> 5);
            cont = pos;
        }
    }
};

template <bool STACK, int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_decode_kernel(EgDecArgs a) {
    __shared__ uint32_t s_tiles[kEgTileWords];
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s0 = (size_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1));
    if (s0 >= a.n_streams) return;                  // (wave-uniform)
    uint32_t* tile = s_tiles + (size_t)(threadIdx.x / kWave) * kWave * kEgTileStride;
    const size_t s = s0 + (size_t)lane;
    const bool valid = s < a.n_streams;
    int32_t st = CST_STREAM_INVALID_DATA;
    EgReader<STACK> rd;
    rd.close();
    rd.w = a.words;
    if (valid) {
        const size_t base = a.offsets ? (size_t)a.offsets[s] : s * a.stride;
        const size_t nw = a.n_words[s];
        const bool inside = !((!a.offsets && nw > a.stride) || (a.capacity && (base > a.capacity || nw > a.capacity - base)));
        if (inside && rd.open(a.words + base, nw, a.cont ? a.cont + s : nullptr)) st = CST_STREAM_OK;
        else rd.close();
    }
    const size_t n = a.n_per;
    for (size_t t0 = 0; t0 < n; t0 += kEgTile) {
        const uint32_t tlen = (uint32_t)((n - t0) < (size_t)kEgTile ? (n - t0) : (size_t)kEgTile);
        for (uint32_t j = 0; j < tlen; ++j) {
            uint32_t sym = 0;          // (from the failing symbol on: 0)
            if (st == CST_STREAM_OK && !rd.template decode<SB>(sym)) { st = CST_STREAM_INVALID_DATA; sym = 0; }
            tile[lane * kEgTileStride + j] = sym;
        }
        eg_lds_fence();
        eg_tile_drain<SB>(a.symbols, a.n_streams, n, s0, t0, tlen, lane, tile);
        eg_lds_fence();
    }
    if (!valid) return;
    a.status[s] = st;
    if (st != CST_STREAM_OK) return;                // d_cont / d_n_words_out stay as they came in
    uint64_t cont;
    uint32_t left;
    rd.position(cont, left);
    if (a.n_words_out) a.n_words_out[s] = left;
    if (a.cont) a.cont[s] = cont;
}

// ---- streams of different lengths: one lane per stream over its own symbol range and its own word slab ----

template <bool STACK, int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_encode_ragged_kernel(EgRaggedEncArgs a) {
    const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
    size_t base = s * a.stride, cap = a.stride;
    if (a.word_offsets) {
        const uint64_t w0 = a.word_offsets[s], w1 = a.word_offsets[s + 1];
        base = (size_t)w0;
        cap = w1 >= w0 ? (size_t)(w1 - w0) : 0;     // (offsets that run backwards: a slab of no words)
    }
    int32_t st = CST_STREAM_OK;
    if (hi < lo || hi - lo > 0xffffffffull) st = CST_STREAM_CAPACITY;
    EgWordSink sink{a.words + base, cap, 0u, make_uint4(0, 0, 0, 0), a.vec && (base & 3u) == 0};
    uint64_t acc = 0;
    uint32_t nb = 0;
    if (st == CST_STREAM_OK) {
        const uint64_t n = hi - lo;
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t x = eg_load<SB>(a.symbols, (size_t)(STACK ? hi - 1 - i : lo + i));
            if (!eg_put_symbol<STACK, SB>(x, acc, nb, sink)) { st = CST_STREAM_CAPACITY; break; }
        }
    }
    const uint64_t bits = 32ull * sink.nw + nb;
    st = eg_finish<STACK>(st, false, acc, nb, sink);
    a.n_words[s] = st == CST_STREAM_OK ? sink.nw : 0u;
    if (a.n_bits) a.n_bits[s] = st == CST_STREAM_OK ? bits : 0ull;
    a.status[s] = st;
}

template <bool STACK, int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_decode_ragged_kernel(EgRaggedDecArgs a) {
    const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
    if (hi < lo) { a.status[s] = CST_STREAM_INVALID_DATA; return; }      // (no output range: nothing is written)
    const size_t base = a.word_offsets ? (size_t)a.word_offsets[s] : s * a.stride;
    const size_t nw = a.n_words[s];
    const bool inside = !((!a.word_offsets && nw > a.stride) || (a.capacity && (base > a.capacity || nw > a.capacity - base)));
    int32_t st = CST_STREAM_INVALID_DATA;
    EgReader<STACK> rd;
    if (inside && rd.open(a.words + base, nw, nullptr)) st = CST_STREAM_OK;
    else rd.close();
    for (uint64_t i = lo; i < hi; ++i) {
        uint32_t sym = 0;
        if (st == CST_STREAM_OK && !rd.template decode<SB>(sym)) { st = CST_STREAM_INVALID_DATA; sym = 0; }
        eg_store<SB>(a.symbols, (size_t)i, sym);
    }
    a.status[s] = st;
}

// ---- jump points: entry d_chunk_offsets[s] + j of d_jump_bits is the bit index in stream s's container at which a
// reader starts symbols [j I, min((j + 1) I, length)) -- the BitJump of the Huffman coders with Exp-Golomb codeword lengths ----

struct EgJumpEncArgs {
    EgRaggedEncArgs r;
    uint64_t interval;                  // symbols per chunk,
    const uint64_t* chunk_offsets;      // [n_streams + 1], and
    uint64_t* jump_bits;                // the table
};

struct EgJumpDecArgs {
    EgRaggedDecArgs r;
    uint64_t interval;                  // symbols per chunk,
    const uint64_t* chunk_offsets;      // [n_streams + 1],
    size_t n_chunks_total;              // the entries of
    const uint64_t* jump_bits;          // the table
    SymbolSelectLanes sel;              // SELECT: one lane per piece in place of one per chunk
};

// One lane per stream, chunk by chunk in coding order, so that the symbol loop is the plain encoder's.  A queue notes the
// container's length in front of chunk j (the bits of symbols[: j I]), a stack behind it (the bits of symbols[j I :]): one 8-byte
// store per chunk, always between two whole codewords, and none outside the stream's own entries.
template <bool STACK, int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_encode_ragged_jump_kernel(EgJumpEncArgs j) {
    const EgRaggedEncArgs& a = j.r;
    const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
    size_t base = s * a.stride, cap = a.stride;
    if (a.word_offsets) {
        const uint64_t w0 = a.word_offsets[s], w1 = a.word_offsets[s + 1];
        base = (size_t)w0;
        cap = w1 >= w0 ? (size_t)(w1 - w0) : 0;     // (offsets that run backwards: a slab of no words)
    }
    int32_t st = CST_STREAM_OK;
    if (hi < lo || hi - lo > 0xffffffffull) st = CST_STREAM_CAPACITY;
    EgWordSink sink{a.words + base, cap, 0u, make_uint4(0, 0, 0, 0), a.vec && (base & 3u) == 0};
    uint64_t acc = 0;
    uint32_t nb = 0;
    if (st == CST_STREAM_OK) {
        const uint32_t n = (uint32_t)(hi - lo);
        const uint32_t I = (uint32_t)j.interval;
        const uint32_t chunks = n / I + (n % I != 0);
        const uint64_t c0 = j.chunk_offsets[s], c1 = j.chunk_offsets[s + 1];
        const uint64_t slots = c1 > c0 ? c1 - c0 : 0;      // (a table that does not describe the stream is not written beyond them)
        for (uint32_t k = 0; k < chunks && st == CST_STREAM_OK; ++k) {
            const uint32_t c = STACK ? chunks - 1 - k : k;
            const uint32_t first = c * I, len = n - first < I ? n - first : I;      // (c I < n <= 2^32 - 1)
            if constexpr (!STACK) {
                if (c < slots) j.jump_bits[c0 + c] = 32ull * sink.nw + nb;
            }
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t x = eg_load<SB>(a.symbols, (size_t)(lo + first + (STACK ? len - 1 - i : i)));
                if (!eg_put_symbol<STACK, SB>(x, acc, nb, sink)) { st = CST_STREAM_CAPACITY; break; }
            }
            if constexpr (STACK) {
                if (st == CST_STREAM_OK && c < slots) j.jump_bits[c0 + c] = 32ull * sink.nw + nb;
            }
        }
    }
    const uint64_t bits = 32ull * sink.nw + nb;
    st = eg_finish<STACK>(st, false, acc, nb, sink);
    a.n_words[s] = st == CST_STREAM_OK ? sink.nw : 0u;
    if (a.n_bits) a.n_bits[s] = st == CST_STREAM_OK ? bits : 0ull;
    a.status[s] = st;
}

// the chunk-lane decoder's wave-private tiles: 64 chunk rows x kEgTile symbols.  There is no code table, so the tiles are all the
// LDS of a block.  u8 and u16 symbols lie in 16-bit elements, row stride 17 words; u32 symbols in 32-bit elements, row stride 33
// words: both odd, so the lane-per-row writes of a wave meet no bank twice.  17 KiB or 33 KiB a block: four blocks share a CU.
template <int SB>
struct EgJumpTile {
    using T = std::conditional_t<SB == 4, uint32_t, uint16_t>;
    static constexpr int kStride = SB == 4 ? kEgTile + 1 : kEgTile + 2;     // in elements
    static constexpr int kElems = (kBlock / kWave) * kWave * kStride;
};

// One lane per CHUNK: lane c finds its stream by a search of chunk_offsets, judges jump_bits[c] against the stream's bit limit,
// opens the window there and decodes at most `interval` symbols, 32 at a time into its tile row; the wave then stores every row as
// one contiguous run of the flat output.  d_status has been zeroed (CST_STREAM_OK): a chunk that fails raises its stream's status
// with an atomic max, and thread t also judges stream t's table (INVALID_DATA if it does not describe the stream).
// SELECT: one lane per PIECE of a select call (cst_symbol_select.hpp); (out_lo, skip, len) come from the piece's record, the
// lane decodes and drops `skip` symbols first, and its status goes to the record.
template <bool STACK, int SB, bool SELECT>
__global__ void __launch_bounds__(kBlock) exp_golomb_decode_ragged_jump_kernel(EgJumpDecArgs j) {
    using Tile = EgJumpTile<SB>;
    __shared__ typename Tile::T s_tiles[Tile::kElems];
    const EgRaggedDecArgs& a = j.r;
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (!SELECT) {
        if (t < a.n_streams) {
            const uint64_t lo = a.sym_offsets[t], hi = a.sym_offsets[t + 1];
            const uint64_t c0 = j.chunk_offsets[t], c1 = j.chunk_offsets[t + 1];
            if (hi < lo || c1 < c0 || c1 > j.n_chunks_total || c1 - c0 != (hi - lo + j.interval - 1) / j.interval)
                atomicMax(a.status + t, (int32_t)CST_STREAM_INVALID_DATA);
        }
    }
    const size_t n_lanes = SELECT ? j.sel.n_pieces : j.n_chunks_total;
    const int lane = threadIdx.x & (kWave - 1);
    if (t - (size_t)lane >= n_lanes) return;      // (wave-uniform: the whole wave lies past the chunks)
    typename Tile::T* tile = s_tiles + (size_t)(threadIdx.x / kWave) * kWave * Tile::kStride;

    uint64_t obase = 0;       // where the lane's symbols go
    uint32_t clen = 0;        // how many it stores (0: no chunk of a well-described stream / no piece of a query, nothing is written)
    uint32_t skip = 0;        // SELECT: symbols decoded and dropped first
    size_t s = 0;
    int32_t st = CST_STREAM_OK;
    EgReader<STACK> rd;
    rd.close();
    if constexpr (SELECT) {
        if (t < n_lanes) {
            clen = j.sel.len[t];
            if (clen) {
                obase = j.sel.out_lo[t];
                skip = j.sel.skip[t];
                const uint32_t* w = a.words + j.sel.word_off[t];      // (a slice the pieces kernel has checked)
                const size_t nw = j.sel.n_words[t];
                const uint32_t e = j.sel.entry[t];
                uint64_t bits;
                if (EgReader<STACK>::limit(w, nw, bits)) {
                    const uint64_t p = e == kSelectNoEntry ? (STACK ? bits : 0ull) : j.sel.jump_bits[e];
                    if (p <= bits) rd.seek(w, nw, p);
                    else st = CST_STREAM_INVALID_DATA;
                } else st = CST_STREAM_INVALID_DATA;
            }
        }
    } else {
        // chunk t belongs to the stream s with chunk_offsets[s] <= t < chunk_offsets[s + 1]
        for (size_t hi_s = a.n_streams; hi_s - s > 1;) {
            const size_t mid = s + (hi_s - s) / 2;
            if (j.chunk_offsets[mid] <= t) s = mid;
            else hi_s = mid;
        }
        if (t < n_lanes) {
            const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
            const uint64_t c0 = j.chunk_offsets[s], c1 = j.chunk_offsets[s + 1];
            if (hi >= lo && c0 <= t && t < c1 && c1 <= j.n_chunks_total && c1 - c0 == (hi - lo + j.interval - 1) / j.interval) {
                obase = lo + (t - c0) * j.interval;
                clen = (uint32_t)(hi - obase < j.interval ? hi - obase : j.interval);
                const size_t base = a.word_offsets ? (size_t)a.word_offsets[s] : s * a.stride;
                const size_t nw = a.n_words[s];
                const bool inside = !((!a.word_offsets && nw > a.stride) || (a.capacity && (base > a.capacity || nw > a.capacity - base)));
                uint64_t bits;
                const uint64_t p = j.jump_bits[t];
                // before any word at the jump point is read: the point lies inside the stream's bits
                if (inside && EgReader<STACK>::limit(a.words + base, nw, bits) && p <= bits) rd.seek(a.words + base, nw, p);
                else st = CST_STREAM_INVALID_DATA;
            }
        }
    }
    int32_t worst = st;
    if constexpr (SELECT) {
        for (uint32_t i = 0; i < skip && st == CST_STREAM_OK; ++i) {
            uint32_t sym;
            if (!rd.template decode<SB>(sym)) worst = st = CST_STREAM_INVALID_DATA;
        }
    }
    uint32_t wmax = clen;     // the wave's longest chunk
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, d, kWave));
    const uint32_t col = (uint32_t)lane & 31u;
    const uint32_t obase_lo = (uint32_t)obase, obase_hi = (uint32_t)(obase >> 32);
    for (uint32_t t0 = 0; t0 < wmax; t0 += kEgTile) {
        const uint32_t tlen = clen > t0 ? (clen - t0 < (uint32_t)kEgTile ? clen - t0 : (uint32_t)kEgTile) : 0u;
        for (uint32_t i = 0; i < tlen; ++i) {
            uint32_t sym = 0;          // (from the failure to the chunk's end: 0)
            if (st == CST_STREAM_OK && !rd.template decode<SB>(sym)) { worst = st = CST_STREAM_INVALID_DATA; sym = 0; }
            tile[lane * Tile::kStride + i] = (typename Tile::T)sym;
        }
        eg_lds_fence();
        // lane l stores column (l & 31) of rows (l >> 5) + 2k, each row at its own place in the flat output
#pragma unroll 8
        for (int k = 0; k < kWave / 2; ++k) {
            const int row = (lane >> 5) + 2 * k;
            const uint64_t rbase = (uint64_t)(uint32_t)__shfl((int)obase_lo, row, kWave) | ((uint64_t)(uint32_t)__shfl((int)obase_hi, row, kWave) << 32);
            const uint32_t rlen = (uint32_t)__shfl((int)clen, row, kWave);
            if (t0 + col < rlen) eg_store<SB>(a.symbols, (size_t)(rbase + t0 + col), tile[row * Tile::kStride + col]);
        }
        eg_lds_fence();
    }
    if constexpr (SELECT) {
        if (t < n_lanes) j.sel.status[t] = worst;
    } else {
        if (worst != CST_STREAM_OK) atomicMax(a.status + s, worst);
    }
}

// ---- the exact bit count of every stream: one wave per stream, 16 bytes of symbols per lane and step ----

template <int SB>
__device__ __forceinline__ uint32_t eg_bits(uint32_t x) {
    uint64_t m;
    return 2u * eg_len<SB>(x, m) + 1u;
}

template <int SB>
__global__ void __launch_bounds__(kBlock) exp_golomb_count_bits_kernel(const void* symbols, const uint64_t* sym_offsets, size_t n_streams,
                                                                       size_t n_per, uint64_t* n_bits) {
    const int lane = threadIdx.x & (kWave - 1);
    const size_t n_waves = (size_t)gridDim.x * (kBlock / kWave);
    for (size_t s = (size_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; s < n_streams; s += n_waves) {
        uint64_t lo = (uint64_t)s * n_per, hi = lo + n_per;
        if (sym_offsets) { lo = sym_offsets[s]; hi = sym_offsets[s + 1]; }
        uint64_t sum = 0;
        if (hi > lo) {
            const uint8_t* p = static_cast<const uint8_t*>(symbols) + lo * SB;
            const uint64_t bytes = (hi - lo) * SB;
            const uint64_t to_line = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u;    // (a multiple of SB)
            const uint64_t head = to_line < bytes ? to_line : bytes;
            const uint64_t groups = (bytes - head) / 16;
            const uint64_t tail = head + 16 * groups;
            for (uint64_t i = (uint64_t)lane * SB; i < head; i += (uint64_t)kWave * SB) sum += eg_bits<SB>(eg_load<SB>(p + i, 0));
            for (uint64_t g = lane; g < groups; g += kWave) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + head + 16 * g);
                const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr (SB == 4) {
                        sum += eg_bits<4>(q[k]);
                    } else if constexpr (SB == 2) {
                        sum += eg_bits<2>(q[k] & 0xffffu) + eg_bits<2>(q[k] >> 16);
                    } else {
                        sum += eg_bits<1>(q[k] & 0xffu) + eg_bits<1>((q[k] >> 8) & 0xffu) + eg_bits<1>((q[k] >> 16) & 0xffu) + eg_bits<1>(q[k] >> 24);
                    }
                }
            }
            for (uint64_t i = tail + (uint64_t)lane * SB; i < bytes; i += (uint64_t)kWave * SB) sum += eg_bits<SB>(eg_load<SB>(p + i, 0));
        }
        uint32_t slo = (uint32_t)sum, shi = (uint32_t)(sum >> 32);
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const uint64_t other = (uint64_t)(uint32_t)__shfl_down((int)slo, d, kWave) | ((uint64_t)(uint32_t)__shfl_down((int)shi, d, kWave) << 32);
            const uint64_t t = (((uint64_t)shi << 32) | slo) + other;
            slo = (uint32_t)t;
            shi = (uint32_t)(t >> 32);
        }
        if (lane == 0) n_bits[s] = ((uint64_t)shi << 32) | slo;
    }
}

template <typename K, typename... A>
cst_status launch_eg(K kernel, size_t blocks, hipStream_t hs, A... args) {
    if (blocks == 0) return CST_OK;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, hs, args...);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

// kernel<STACK, SB> for the run-time semantics and symbol width
#define CST_EG_DISPATCH(KERNEL, stack, sb, blocks, hs, args)                                        \
    ((stack) ? ((sb) == 1 ? launch_eg(KERNEL<true, 1>, blocks, hs, args)                            \
                : (sb) == 2 ? launch_eg(KERNEL<true, 2>, blocks, hs, args)                          \
                            : launch_eg(KERNEL<true, 4>, blocks, hs, args))                         \
             : ((sb) == 1 ? launch_eg(KERNEL<false, 1>, blocks, hs, args)                           \
                : (sb) == 2 ? launch_eg(KERNEL<false, 2>, blocks, hs, args)                         \
                            : launch_eg(KERNEL<false, 4>, blocks, hs, args)))

inline bool eg_semantics_ok(int32_t semantics) { return semantics == CST_HUFFMAN_STACK || semantics == CST_HUFFMAN_QUEUE; }
inline bool eg_width_ok(int32_t symbol_bytes) { return symbol_bytes == 1 || symbol_bytes == 2 || symbol_bytes == 4; }
inline size_t eg_blocks(size_t n_streams) { return (n_streams + kBlock - 1) / kBlock; }
// chunks of 32 .. 2^31 - 32 symbols, a multiple of the symbol tile's width
inline bool eg_interval_ok(size_t interval) { return interval > 0 && interval % kEgTile == 0 && interval <= 0x7fffffffull; }

// exp_golomb_decode_ragged_jump_kernel<STACK, SB, SELECT> over `lanes` chunks or pieces
template <bool SELECT>
cst_status eg_jump_decode(bool stack, int32_t sb, size_t lanes, hipStream_t hs, const EgJumpDecArgs& a) {
    const size_t blocks = eg_blocks(lanes);
    if (stack) return sb == 1 ? launch_eg(exp_golomb_decode_ragged_jump_kernel<true, 1, SELECT>, blocks, hs, a)
                    : sb == 2 ? launch_eg(exp_golomb_decode_ragged_jump_kernel<true, 2, SELECT>, blocks, hs, a)
                              : launch_eg(exp_golomb_decode_ragged_jump_kernel<true, 4, SELECT>, blocks, hs, a);
    return sb == 1 ? launch_eg(exp_golomb_decode_ragged_jump_kernel<false, 1, SELECT>, blocks, hs, a)
         : sb == 2 ? launch_eg(exp_golomb_decode_ragged_jump_kernel<false, 2, SELECT>, blocks, hs, a)
                   : launch_eg(exp_golomb_decode_ragged_jump_kernel<false, 4, SELECT>, blocks, hs, a);
}

} // namespace

} // namespace cst

using namespace cst;

extern "C" {

size_t cst_exp_golomb_max_words(size_t n_per_stream, int32_t symbol_bytes, int32_t semantics) {
    if (!eg_width_ok(symbol_bytes) || !eg_semantics_ok(semantics)) return 0;
    const size_t len = 16 * (size_t)symbol_bytes + 1;      // 2 B + 1
    if (n_per_stream > (SIZE_MAX - 1024) / len) return 0;
    // every codeword at its longest + up to 31 bits a continued call starts with + the seal of a stack, in whole 64-byte units
    const size_t words = (n_per_stream * len + 32 + 31) / 32;
    return (words + 15) / 16 * 16;
}

cst_status cst_exp_golomb_count_bits(const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets, size_t n_streams,
                                     size_t n_per_stream, uint64_t* d_n_bits, void* stream) {
    if (!eg_width_ok(symbol_bytes) || !d_n_bits) return CST_ERR_INVALID_ARGUMENT;
    if (!d_symbols && (d_sym_offsets || n_per_stream > 0)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    hipStream_t hs = (hipStream_t)stream;
    const size_t per_block = kBlock / kWave;
    const size_t blocks = std::min<size_t>((n_streams + per_block - 1) / per_block, 16384);
    cst_status rc;
    if (symbol_bytes == 1) rc = launch_eg(exp_golomb_count_bits_kernel<1>, blocks, hs, d_symbols, d_sym_offsets, n_streams, n_per_stream, d_n_bits);
    else if (symbol_bytes == 2) rc = launch_eg(exp_golomb_count_bits_kernel<2>, blocks, hs, d_symbols, d_sym_offsets, n_streams, n_per_stream, d_n_bits);
    else rc = launch_eg(exp_golomb_count_bits_kernel<4>, blocks, hs, d_symbols, d_sym_offsets, n_streams, n_per_stream, d_n_bits);
    return note_kernel("exp_golomb_count_bits_kernel", rc);
}

cst_status cst_exp_golomb_encode_batch(int32_t semantics, const void* d_symbols, int32_t symbol_bytes, size_t n_streams,
                                       size_t n_per_stream, uint32_t* d_words, size_t stride_words, uint32_t* d_n_words,
                                       uint64_t* d_n_bits, uint64_t* d_cont, int32_t* d_status, void* stream) {
    if (!d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!d_words && stride_words) return CST_ERR_INVALID_ARGUMENT;      // (no slab at all: every stream needs none or reports CAPACITY)
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (n_per_stream > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgEncArgs a{};
    a.symbols = d_symbols; a.n_streams = n_streams; a.n_per = n_per_stream;
    a.words = d_words; a.stride = stride_words; a.n_words = d_n_words; a.n_bits = d_n_bits; a.cont = d_cont; a.status = d_status;
    a.vec = stride_words % 4 == 0 && (reinterpret_cast<uintptr_t>(d_words) & 15u) == 0;
    hipStream_t hs = (hipStream_t)stream;
    return note_kernel("exp_golomb_encode_kernel",
                       CST_EG_DISPATCH(exp_golomb_encode_kernel, semantics == CST_HUFFMAN_STACK, symbol_bytes, eg_blocks(n_streams), hs, a));
}

cst_status cst_exp_golomb_decode_batch(int32_t semantics, const uint32_t* d_words, const uint64_t* d_offsets, size_t stride_words,
                                       size_t words_capacity, const uint32_t* d_n_words, void* d_symbols, int32_t symbol_bytes,
                                       size_t n_streams, size_t n_per_stream, uint64_t* d_cont, uint32_t* d_n_words_out,
                                       int32_t* d_status, void* stream) {
    if (!d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (n_per_stream > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    if (!d_words && (d_offsets || stride_words)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgDecArgs a{};
    a.words = d_words;     // (NULL: every stream must be empty, nothing is read)
    a.offsets = d_offsets; a.stride = stride_words; a.capacity = words_capacity; a.n_words = d_n_words;
    a.symbols = d_symbols; a.n_streams = n_streams; a.n_per = n_per_stream;
    a.cont = d_cont; a.n_words_out = d_n_words_out; a.status = d_status;
    hipStream_t hs = (hipStream_t)stream;
    return note_kernel("exp_golomb_decode_kernel",
                       CST_EG_DISPATCH(exp_golomb_decode_kernel, semantics == CST_HUFFMAN_STACK, symbol_bytes, eg_blocks(n_streams), hs, a));
}

cst_status cst_exp_golomb_encode_ragged(int32_t semantics, const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets,
                                        size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                        uint32_t* d_n_words, uint64_t* d_n_bits, int32_t* d_status, void* stream) {
    if (!d_symbols || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgRaggedEncArgs a{};
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words;
    a.n_words = d_n_words; a.n_bits = d_n_bits; a.status = d_status;
    a.vec = (reinterpret_cast<uintptr_t>(d_words) & 15u) == 0 && (d_word_offsets || stride_words % 4 == 0);
    hipStream_t hs = (hipStream_t)stream;
    return note_kernel("exp_golomb_encode_ragged_kernel",
                       CST_EG_DISPATCH(exp_golomb_encode_ragged_kernel, semantics == CST_HUFFMAN_STACK, symbol_bytes, eg_blocks(n_streams), hs, a));
}

cst_status cst_exp_golomb_decode_ragged(int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                        size_t words_capacity, const uint32_t* d_n_words, void* d_symbols, int32_t symbol_bytes,
                                        const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, void* stream) {
    if (!d_words || !d_n_words || !d_symbols || !d_sym_offsets || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgRaggedDecArgs a{};
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words; a.capacity = words_capacity; a.n_words = d_n_words;
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.status = d_status;
    hipStream_t hs = (hipStream_t)stream;
    return note_kernel("exp_golomb_decode_ragged_kernel",
                       CST_EG_DISPATCH(exp_golomb_decode_ragged_kernel, semantics == CST_HUFFMAN_STACK, symbol_bytes, eg_blocks(n_streams), hs, a));
}

cst_status cst_exp_golomb_encode_ragged_jump(int32_t semantics, const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets,
                                             size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                             uint32_t* d_n_words, uint64_t* d_n_bits, size_t jump_interval, const uint64_t* d_chunk_offsets,
                                             uint64_t* d_jump_bits, int32_t* d_status, void* stream) {
    if (!d_symbols || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_interval_ok(jump_interval) || !d_chunk_offsets || !d_jump_bits) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgJumpEncArgs j{};
    EgRaggedEncArgs& a = j.r;
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words;
    a.n_words = d_n_words; a.n_bits = d_n_bits; a.status = d_status;
    a.vec = (reinterpret_cast<uintptr_t>(d_words) & 15u) == 0 && (d_word_offsets || stride_words % 4 == 0);
    j.interval = jump_interval; j.chunk_offsets = d_chunk_offsets; j.jump_bits = d_jump_bits;
    hipStream_t hs = (hipStream_t)stream;
    return note_kernel("exp_golomb_encode_ragged_jump_kernel",
                       CST_EG_DISPATCH(exp_golomb_encode_ragged_jump_kernel, semantics == CST_HUFFMAN_STACK, symbol_bytes, eg_blocks(n_streams), hs, j));
}

cst_status cst_exp_golomb_decode_ragged_jump(int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                             size_t words_capacity, const uint32_t* d_n_words, void* d_symbols, int32_t symbol_bytes,
                                             const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                             const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint64_t* d_jump_bits,
                                             int32_t* d_status, void* stream) {
    if (!d_words || !d_n_words || !d_symbols || !d_sym_offsets || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_interval_ok(jump_interval) || !d_chunk_offsets || !d_jump_bits) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    EgJumpDecArgs j{};
    EgRaggedDecArgs& a = j.r;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words; a.capacity = words_capacity; a.n_words = d_n_words;
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.status = d_status;
    j.interval = jump_interval; j.chunk_offsets = d_chunk_offsets; j.n_chunks_total = n_chunks_total; j.jump_bits = d_jump_bits;
    hipStream_t hs = (hipStream_t)stream;
    CST_HIP_TRY(hipMemsetAsync(d_status, 0, n_streams * sizeof(int32_t), hs));      // CST_STREAM_OK: the kernel only raises it
    const size_t lanes = std::max(n_streams, n_chunks_total);      // a lane per chunk, and one per stream for the table's check
    return note_kernel("exp_golomb_decode_ragged_jump_kernel", eg_jump_decode<false>(semantics == CST_HUFFMAN_STACK, symbol_bytes, lanes, hs, j));
}

cst_status cst_exp_golomb_decode_ragged_select(int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                               size_t words_capacity, const uint32_t* d_n_words, const uint64_t* d_sym_offsets, size_t n_streams,
                                               size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                               const uint64_t* d_jump_bits, const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                               const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets,
                                               size_t n_pieces_total, void* d_symbols_out, int32_t symbol_bytes, const uint64_t* d_out_offsets,
                                               void* d_scratch, int32_t* d_status, void* stream) {
    if (!d_words || !d_n_words || !d_sym_offsets) return CST_ERR_INVALID_ARGUMENT;
    if (!eg_semantics_ok(semantics) || !eg_width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    const int table = (d_chunk_offsets != nullptr) + (d_jump_bits != nullptr);
    if (!symbol_select_args_ok(jump_interval, table, n_chunks_total, d_query_first, d_query_count, n_pieces_total)) return CST_ERR_INVALID_ARGUMENT;
    if (n_queries > 0 && (!d_query_stream || !d_piece_offsets || !d_symbols_out || !d_out_offsets || !d_scratch || !d_status))
        return CST_ERR_INVALID_ARGUMENT;
    if (n_queries == 0) return CST_OK;
    if (n_queries > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    const RaggedSelect b = symbol_select_batch(d_word_offsets, stride_words, words_capacity, d_n_words, d_sym_offsets, n_streams, jump_interval,
                                               d_chunk_offsets, n_chunks_total, d_query_stream, d_query_first, d_query_count, n_queries,
                                               d_piece_offsets, n_pieces_total, d_out_offsets);
    const RaggedSelectPieces v(d_scratch, n_pieces_total);
    EgJumpDecArgs j{};
    j.r.words = d_words; j.r.symbols = d_symbols_out;
    j.sel = symbol_select_lanes(v, d_jump_bits, n_pieces_total);
    hipStream_t hs = (hipStream_t)stream;
    const bool stack = semantics == CST_HUFFMAN_STACK;
    return note_kernel("exp_golomb_decode_ragged_jump_kernel<select>", symbol_select_run(stack, b, d_words, d_jump_bits, v, d_status, hs, [&] {
                           return eg_jump_decode<true>(stack, symbol_bytes, n_pieces_total, hs, j);
                       }));
}

}  // extern "C"
