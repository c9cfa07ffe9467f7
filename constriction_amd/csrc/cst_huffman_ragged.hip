// cst_huffman_ragged.hip -- Huffman symbol codes for streams of different lengths: one bit container per document, all of them in
// one launch (the layout of cst_exp_golomb_*_ragged), the exact bit count that sizes their slabs, and jump points.
//
// The containers and the codebook are those of cst_huffman.hip; every stream's words are what cst_huffman_encode_batch writes for
// it as a one-row batch.  A jump point of a prefix code is one bit position and no coder state: entry d_chunk_offsets[s] + j of
// d_jump_bits is the bit index in stream s's container at which a reader starts symbols [j I, min((j + 1) I, length)) -- for a
// queue the first bit of that chunk's first codeword (read upwards), for a stack one past the highest bit of it (read downwards;
// entry 0 is n_bits, where the seal sits).  Either way it is the container's length when the encoder crosses that boundary, so
// the encoder notes it on its way, and the jump decoder runs one lane per CHUNK: the longest chain of a launch is I symbols.
#include <algorithm>
#include <type_traits>

#include "cst_huffman.hpp"
#include "cst_symbol_select.hpp"

namespace cst {

namespace {

struct HrEncArgs {
    const uint2* enc;
    const uint32_t* pool;
    uint32_t n_sym;
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
    uint64_t interval;                  // jump points (JUMP): symbols per chunk,
    const uint64_t* chunk_offsets;      // [n_streams + 1], and
    uint64_t* jump_bits;                // the table
};

struct HrDecArgs {
    const uint32_t* lut;
    const uint32_t* child;
    uint32_t n_sym;
    int32_t lut_bits;
    const uint32_t* words;
    const uint64_t* word_offsets;
    size_t stride, capacity;
    const uint32_t* n_words;
    void* symbols;
    const uint64_t* sym_offsets;
    size_t n_streams;
    int32_t* status;
    uint64_t interval;                  // the jump decoder: symbols per chunk,
    const uint64_t* chunk_offsets;      // [n_streams + 1],
    size_t n_chunks_total;              // the entries of
    const uint64_t* jump_bits;          // the table
};

// the SELECT form of the jump decoder: one lane per piece of a select call (cst_symbol_select.hpp)
struct HrSelArgs : HrDecArgs {
    SymbolSelectLanes sel;
};

// dynamic LDS: [codeword table (LDS_TAB)].  One lane per stream, its symbols read where they lie.
template <bool STACK, bool LONG, bool LDS_TAB, int SB, bool JUMP>
__global__ void __launch_bounds__(kBlock) huffman_encode_ragged_kernel(HrEncArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_enc_lds[];
    const uint2* enc = a.enc;
    if constexpr (LDS_TAB) {
        uint2* t = reinterpret_cast<uint2*>(s_enc_lds);
        for (uint32_t i = threadIdx.x; i < a.n_sym; i += kBlock) t[i] = a.enc[i];
        __syncthreads();
        enc = t;
    }
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
    WordSink sink{a.words + base, cap, 0u, make_uint4(0, 0, 0, 0), a.vec && (base & 3u) == 0};
    uint64_t acc = 0;
    uint32_t nb = 0;
    if (st == CST_STREAM_OK) {
        // chunk by chunk in coding order (without jump points: the stream is one chunk), so that the symbol loop itself is the
        // plain encoder's.  A queue notes the container's length in front of chunk j (the bits of symbols[: j I]), a stack behind
        // it (the bits of symbols[j I :]); `slots` entries are this stream's (a table that does not describe the stream is not
        // written beyond them).
        const uint32_t n = (uint32_t)(hi - lo);
        const uint32_t I = JUMP ? (uint32_t)a.interval : (n ? n : 1u);
        const uint32_t chunks = n / I + (n % I != 0);
        uint64_t c0 = 0, slots = 0;
        if constexpr (JUMP) {
            c0 = a.chunk_offsets[s];
            const uint64_t c1 = a.chunk_offsets[s + 1];
            slots = c1 > c0 ? c1 - c0 : 0;
        }
        for (uint32_t k = 0; k < chunks && st == CST_STREAM_OK; ++k) {
            const uint32_t j = STACK ? chunks - 1 - k : k;
            const uint32_t first = j * I, len = n - first < I ? n - first : I;      // (j I < n <= 2^32 - 1)
            if constexpr (JUMP && !STACK) {
                if (j < slots) a.jump_bits[c0 + j] = 32ull * sink.nw + nb;
            }
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t x = load_sym<SB>(a.symbols, (size_t)(lo + first + (STACK ? len - 1 - i : i)));
                if (x >= a.n_sym) { st = CST_STREAM_IMPOSSIBLE_SYMBOL; break; }
                if (!put_symbol<LONG>(enc[x], a.pool, acc, nb, sink)) { st = CST_STREAM_CAPACITY; break; }
            }
            if constexpr (JUMP && STACK) {
                if (st == CST_STREAM_OK && j < slots) a.jump_bits[c0 + j] = 32ull * sink.nw + nb;
            }
        }
    }
    const uint64_t bits = 32ull * sink.nw + nb;   // the reference's len(): written bits, without the seal
    if (st == CST_STREAM_OK) {
        if (STACK && !put_bits(1u, 1u, acc, nb, sink)) st = CST_STREAM_CAPACITY;   // the seal
        if (st == CST_STREAM_OK && nb > 0 && !sink.put((uint32_t)acc)) st = CST_STREAM_CAPACITY;
    }
    if (st == CST_STREAM_OK) sink.finish();
    a.n_words[s] = st == CST_STREAM_OK ? sink.nw : 0u;
    if (a.n_bits) a.n_bits[s] = st == CST_STREAM_OK ? bits : 0ull;
    a.status[s] = st;
}

// A lane's read side: a 64-bit window of the next bits (queue: from bit 0 up; stack: from bit 63 down; the bits beyond `have`
// are zero), refilled a word at a time, the next word loaded one refill ahead -- the window of huffman_decode_kernel, opened at
// any bit index of the container.
template <bool STACK>
struct HuffReader {
    const uint32_t* w;
    size_t nw;        // words of the stream
    size_t wi;        // queue: next word to load; stack: words below the window still to load
    uint64_t buf;
    uint32_t have;    // valid bits in buf
    uint32_t pf;      // the next word to enter the window

    __device__ __forceinline__ void close() { nw = 0; wi = 0; buf = 0; have = 0; pf = 0; }

    // the highest bit index a reader may start at: the container's bit length.  A stack's is the position of its seal, the
    // HIGHEST set bit of its last word.  false: a stack without words or with a zero last word
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

    // one symbol.  CST_STREAM_OUT_OF_DATA: the bits ran out inside a codeword
    template <bool LONG>
    __device__ __forceinline__ int32_t decode(const uint32_t* s_lut, const uint32_t* child, uint32_t n_sym, uint32_t L, uint32_t lmask,
                                              uint32_t& sym) {
        if (STACK) {
            if (have <= 32 && wi > 0) {
                buf |= (uint64_t)pf << (32 - have); have += 32; --wi;
                pf = wi > 0 ? w[wi - 1] : 0u;
            }
        } else {
            if (have <= 32 && wi < nw) {
                buf |= (uint64_t)pf << have; have += 32; ++wi;
                pf = wi < nw ? w[wi] : 0u;
            }
        }
        const uint32_t idx = STACK ? (uint32_t)__builtin_bitreverse64(buf) & lmask : (uint32_t)buf & lmask;
        const uint32_t e = s_lut[idx];
        if (!LONG || !(e & kLutCont)) {
            const uint32_t len = (e >> kLutLenShift) & 63u;
            if (len > have) return CST_STREAM_OUT_OF_DATA;      // (have < 32 only once the words are exhausted)
            buf = STACK ? buf << len : buf >> len;
            have -= len;
            sym = e & ((1u << kLutLenShift) - 1u);
            return CST_STREAM_OK;
        }
        if (L > have) return CST_STREAM_OUT_OF_DATA;
        buf = STACK ? buf << L : buf >> L;
        have -= L;
        uint32_t node = e & ((1u << kLutLenShift) - 1u);
        while (node >= n_sym) {
            if (have == 0) {
                if (STACK ? wi == 0 : wi >= nw) return CST_STREAM_OUT_OF_DATA;
                if (STACK) { buf = (uint64_t)pf << 32; --wi; pf = wi > 0 ? w[wi - 1] : 0u; }
                else { buf = pf; ++wi; pf = wi < nw ? w[wi] : 0u; }
                have = 32;
            }
            const uint32_t bit = STACK ? (uint32_t)(buf >> 63) : (uint32_t)buf & 1u;
            buf = STACK ? buf << 1 : buf >> 1;
            --have;
            node = child[2u * (node - n_sym) + bit];
        }
        sym = node;
        return CST_STREAM_OK;
    }
};

__device__ __forceinline__ uint32_t* stage_lut(uint32_t* lds, const uint32_t* lut, uint32_t lut_n) {
    for (uint32_t i = threadIdx.x; i < lut_n; i += kBlock) lds[i] = lut[i];
    __syncthreads();
    return lds;
}

// the words of stream s, checked against the buffer as cst_huffman_decode_batch checks them.  false: counts or offsets that
// exceed it
__device__ __forceinline__ bool stream_words(const HrDecArgs& a, size_t s, size_t& base, size_t& nw) {
    base = a.word_offsets ? (size_t)a.word_offsets[s] : s * a.stride;
    nw = a.n_words[s];
    return !((!a.word_offsets && nw > a.stride) || (a.capacity && (base > a.capacity || nw > a.capacity - base)));
}

// dynamic LDS: [decode table, 2^lut_bits words].  One lane per stream, its symbols stored where they belong.
template <bool STACK, bool LONG, int SB>
__global__ void __launch_bounds__(kBlock) huffman_decode_ragged_kernel(HrDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dec_lds[];
    const uint32_t lut_n = 1u << a.lut_bits;
    const uint32_t* s_lut = stage_lut(s_dec_lds, a.lut, lut_n);
    const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
    if (hi < lo) { a.status[s] = CST_STREAM_INVALID_DATA; return; }      // (no output range: nothing is written)
    size_t base, nw;
    int32_t st = CST_STREAM_INVALID_DATA;
    HuffReader<STACK> rd;
    rd.close();
    uint64_t bits;
    if (stream_words(a, s, base, nw) && HuffReader<STACK>::limit(a.words + base, nw, bits)) {
        rd.seek(a.words + base, nw, STACK ? bits : 0ull);
        st = CST_STREAM_OK;
    }
    const uint32_t L = (uint32_t)a.lut_bits, lmask = lut_n - 1u;
    for (uint64_t i = lo; i < hi; ++i) {
        uint32_t sym = 0;          // (after an error: 0)
        if (st == CST_STREAM_OK) {
            st = rd.template decode<LONG>(s_lut, a.child, a.n_sym, L, lmask, sym);
            if (st != CST_STREAM_OK) sym = 0;
        }
        store_sym<SB>(a.symbols, (size_t)i, sym);
    }
    a.status[s] = st;
}

// the jump decoder's wave-private tiles: 64 chunk rows x kTile symbols of 16 bits (an alphabet has at most 2^16 symbols), row
// stride 17 words: conflict-free for the lane-per-row writes, and half the LDS of the rectangular decoder's tiles, so that four
// blocks (16 KiB of table + 17 KiB of tiles each) share a CU
constexpr int kJumpTileStride = kTile + 2;      // in 16-bit units
constexpr size_t kJumpTileBytesPerBlock = (size_t)(kBlock / kWave) * kWave * kJumpTileStride * sizeof(uint16_t);

// dynamic LDS: [decode table, 2^lut_bits words] [one output tile per wave].  One lane per CHUNK: lane c finds its stream by a
// search of chunk_offsets, opens the window at jump_bits[c] and decodes at most `interval` symbols, 32 at a time into its tile
// row; the wave then stores every row as one contiguous run of the flat output (128 B of int32, 32 B of uint8).
// d_status has been zeroed (CST_STREAM_OK): a chunk that fails raises its stream's status with an atomic max, and thread t also
// judges stream t's table (INVALID_DATA if it does not describe the stream).
// SELECT: one lane per PIECE of a select call; (out_lo, skip, len) come from the piece's record in place of (obase, clen), the
// lane decodes and drops `skip` symbols first, and its status goes to the record.
template <bool STACK, bool LONG, int SB, bool SELECT = false>
__global__ void __launch_bounds__(kBlock) huffman_decode_ragged_jump_kernel(std::conditional_t<SELECT, HrSelArgs, HrDecArgs> a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dec_lds[];
    const uint32_t lut_n = 1u << a.lut_bits;
    const uint32_t* s_lut = stage_lut(s_dec_lds, a.lut, lut_n);
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (!SELECT) {
        if (t < a.n_streams) {
            const uint64_t lo = a.sym_offsets[t], hi = a.sym_offsets[t + 1];
            const uint64_t c0 = a.chunk_offsets[t], c1 = a.chunk_offsets[t + 1];
            if (hi < lo || c1 < c0 || c1 > a.n_chunks_total || c1 - c0 != (hi - lo + a.interval - 1) / a.interval)
                atomicMax(a.status + t, (int32_t)CST_STREAM_INVALID_DATA);
        }
    }
    size_t n_lanes = a.n_chunks_total;
    if constexpr (SELECT) n_lanes = a.sel.n_pieces;
    const int lane = threadIdx.x & (kWave - 1);
    if (t - (size_t)lane >= n_lanes) return;      // (wave-uniform: the whole wave lies past the chunks)
    uint16_t* tile = reinterpret_cast<uint16_t*>(s_dec_lds + ((lut_n + 3) & ~3u)) + (size_t)(threadIdx.x / kWave) * kWave * kJumpTileStride;

    // chunk t belongs to the stream s with chunk_offsets[s] <= t < chunk_offsets[s + 1]
    size_t s = 0;
    if constexpr (!SELECT) {
        for (size_t hi_s = a.n_streams; hi_s - s > 1;) {
            const size_t mid = s + (hi_s - s) / 2;
            if (a.chunk_offsets[mid] <= t) s = mid;
            else hi_s = mid;
        }
    }
    uint64_t obase = 0;       // where the chunk's symbols go
    uint32_t clen = 0;        // how many it has (0: no chunk of a well-described stream, nothing is written)
    int32_t st = CST_STREAM_OK;
    HuffReader<STACK> rd;
    rd.close();
    uint32_t skip = 0;        // SELECT: symbols decoded and dropped first
    if constexpr (SELECT) {
        if (t < n_lanes && (clen = a.sel.len[t]) != 0) {
            obase = a.sel.out_lo[t];
            skip = a.sel.skip[t];
            const uint32_t* w = a.words + a.sel.word_off[t];      // (a slice the pieces kernel has checked)
            const size_t nw = a.sel.n_words[t];
            const uint32_t e = a.sel.entry[t];
            uint64_t bits;
            if (HuffReader<STACK>::limit(w, nw, bits)) {
                const uint64_t p = e == kSelectNoEntry ? (STACK ? bits : 0ull) : a.sel.jump_bits[e];
                if (p <= bits) rd.seek(w, nw, p);
                else st = CST_STREAM_INVALID_DATA;
            } else st = CST_STREAM_INVALID_DATA;
        }
    } else if (t < a.n_chunks_total) {
        const uint64_t lo = a.sym_offsets[s], hi = a.sym_offsets[s + 1];
        const uint64_t c0 = a.chunk_offsets[s], c1 = a.chunk_offsets[s + 1];
        if (hi >= lo && c0 <= t && t < c1 && c1 <= a.n_chunks_total && c1 - c0 == (hi - lo + a.interval - 1) / a.interval) {
            obase = lo + (t - c0) * a.interval;
            clen = (uint32_t)(hi - obase < a.interval ? hi - obase : a.interval);
            size_t base, nw;
            uint64_t bits;
            const uint64_t p = a.jump_bits[t];
            // before any word at the jump point is read: the point lies inside the stream's bits
            if (stream_words(a, s, base, nw) && HuffReader<STACK>::limit(a.words + base, nw, bits) && p <= bits) rd.seek(a.words + base, nw, p);
            else st = CST_STREAM_INVALID_DATA;
        }
    }
    uint32_t wmax = clen;     // the wave's longest chunk
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, d, kWave));
    const uint32_t L = (uint32_t)a.lut_bits, lmask = lut_n - 1u;
    const uint32_t col = (uint32_t)lane & 31u;
    const uint32_t obase_lo = (uint32_t)obase, obase_hi = (uint32_t)(obase >> 32);
    int32_t worst = st;
    if constexpr (SELECT) {
        for (; skip > 0 && st == CST_STREAM_OK; --skip) {
            uint32_t sym;
            worst = st = rd.template decode<LONG>(s_lut, a.child, a.n_sym, L, lmask, sym);
        }
    }
    for (uint32_t t0 = 0; t0 < wmax; t0 += kTile) {
        const uint32_t tlen = clen > t0 ? (clen - t0 < (uint32_t)kTile ? clen - t0 : (uint32_t)kTile) : 0u;
        for (uint32_t j = 0; j < tlen; ++j) {
            uint32_t sym = 0;          // (from the failure to the chunk's end: 0)
            if (st == CST_STREAM_OK) {
                st = rd.template decode<LONG>(s_lut, a.child, a.n_sym, L, lmask, sym);
                if (st != CST_STREAM_OK) { sym = 0; worst = st; }
            }
            tile[lane * kJumpTileStride + j] = (uint16_t)sym;
        }
        wave_lds_fence();
        // lane l stores column (l & 31) of rows (l >> 5) + 2k, each row at its own place in the flat output
#pragma unroll 8
        for (int k = 0; k < kWave / 2; ++k) {
            const int row = (lane >> 5) + 2 * k;
            const uint64_t rbase = (uint64_t)(uint32_t)__shfl((int)obase_lo, row, kWave) | ((uint64_t)(uint32_t)__shfl((int)obase_hi, row, kWave) << 32);
            const uint32_t rlen = (uint32_t)__shfl((int)clen, row, kWave);
            if (t0 + col < rlen) store_sym<SB>(a.symbols, (size_t)(rbase + t0 + col), tile[row * kJumpTileStride + col]);
        }
        wave_lds_fence();
    }
    if constexpr (SELECT) {
        if (t < n_lanes) a.sel.status[t] = worst;
    } else {
        if (worst != CST_STREAM_OK) atomicMax(a.status + s, worst);
    }
}

// ---- the exact bit count of every stream: one wave per stream, 16 bytes of symbols per lane and step ----

template <int SB>
__global__ void __launch_bounds__(kBlock) huffman_count_bits_kernel(const uint2* __restrict__ enc, uint32_t n_sym, const void* symbols,
                                                                    const uint64_t* sym_offsets, size_t n_streams, size_t n_per,
                                                                    uint64_t* n_bits) {
    const int lane = threadIdx.x & (kWave - 1);
    const size_t n_waves = (size_t)gridDim.x * (kBlock / kWave);
    auto len_of = [&](uint32_t x) -> uint32_t { return x < n_sym ? enc[x].y : 0u; };    // (not in the alphabet: the encoder reports it)
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
            for (uint64_t i = (uint64_t)lane * SB; i < head; i += (uint64_t)kWave * SB) sum += len_of(load_sym<SB>(p + i, 0));
            for (uint64_t g = lane; g < groups; g += kWave) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + head + 16 * g);
                const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr (SB == 4) sum += len_of(q[k]);
                    else sum += len_of(q[k] & 0xffu) + len_of((q[k] >> 8) & 0xffu) + len_of((q[k] >> 16) & 0xffu) + len_of(q[k] >> 24);
                }
            }
            for (uint64_t i = tail + (uint64_t)lane * SB; i < bytes; i += (uint64_t)kWave * SB) sum += len_of(load_sym<SB>(p + i, 0));
        }
        uint32_t slo = (uint32_t)sum, shi = (uint32_t)(sum >> 32);
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const uint64_t other = (uint64_t)(uint32_t)__shfl_down((int)slo, d, kWave) | ((uint64_t)(uint32_t)__shfl_down((int)shi, d, kWave) << 32);
            const uint64_t sm = (((uint64_t)shi << 32) | slo) + other;
            slo = (uint32_t)sm;
            shi = (uint32_t)(sm >> 32);
        }
        if (lane == 0) n_bits[s] = ((uint64_t)shi << 32) | slo;
    }
}

// kernel<STACK, LONG, ..., SB, ...> for the run-time semantics, codeword lengths and symbol width
template <bool STACK, bool LONG, bool JUMP>
cst_status encode_ragged_sb(const HrEncArgs& a, int32_t symbol_bytes, hipStream_t hs) {
    const size_t tab = ((size_t)a.n_sym * sizeof(uint2) + 15) & ~(size_t)15;
    if (tab <= kEncLdsBytes) {
        if (symbol_bytes == 1) return launch_huff(huffman_encode_ragged_kernel<STACK, LONG, true, 1, JUMP>, a.n_streams, tab, hs, a);
        return launch_huff(huffman_encode_ragged_kernel<STACK, LONG, true, 4, JUMP>, a.n_streams, tab, hs, a);
    }
    if (symbol_bytes == 1) return launch_huff(huffman_encode_ragged_kernel<STACK, LONG, false, 1, JUMP>, a.n_streams, 0, hs, a);
    return launch_huff(huffman_encode_ragged_kernel<STACK, LONG, false, 4, JUMP>, a.n_streams, 0, hs, a);
}

template <bool JUMP>
cst_status encode_ragged(const HuffCodebook* c, int32_t semantics, const HrEncArgs& a, int32_t symbol_bytes, hipStream_t hs) {
    const bool lng = c->max_len > 32;
    const char* name = lng ? "huffman_encode_ragged_long_kernel" : "huffman_encode_ragged_kernel";
    if (semantics == CST_HUFFMAN_STACK)
        return note_kernel(name, lng ? encode_ragged_sb<true, true, JUMP>(a, symbol_bytes, hs) : encode_ragged_sb<true, false, JUMP>(a, symbol_bytes, hs));
    return note_kernel(name, lng ? encode_ragged_sb<false, true, JUMP>(a, symbol_bytes, hs) : encode_ragged_sb<false, false, JUMP>(a, symbol_bytes, hs));
}

#define CST_HR_DECODE(KERNEL, lanes, lds)                                                                                   \
    (semantics == CST_HUFFMAN_STACK                                                                                         \
         ? (lng ? (symbol_bytes == 1 ? launch_huff(KERNEL<true, true, 1>, lanes, lds, hs, a) : launch_huff(KERNEL<true, true, 4>, lanes, lds, hs, a))        \
                : (symbol_bytes == 1 ? launch_huff(KERNEL<true, false, 1>, lanes, lds, hs, a) : launch_huff(KERNEL<true, false, 4>, lanes, lds, hs, a)))     \
         : (lng ? (symbol_bytes == 1 ? launch_huff(KERNEL<false, true, 1>, lanes, lds, hs, a) : launch_huff(KERNEL<false, true, 4>, lanes, lds, hs, a))      \
                : (symbol_bytes == 1 ? launch_huff(KERNEL<false, false, 1>, lanes, lds, hs, a) : launch_huff(KERNEL<false, false, 4>, lanes, lds, hs, a))))

// huffman_decode_ragged_jump_kernel<STACK, LONG, SB, true> over the pieces of a select call
template <bool STACK, bool LONG>
cst_status decode_select_sb(const HrSelArgs& a, int32_t symbol_bytes, size_t lds, hipStream_t hs) {
    if (symbol_bytes == 1) return launch_huff(huffman_decode_ragged_jump_kernel<STACK, LONG, 1, true>, a.sel.n_pieces, lds, hs, a);
    return launch_huff(huffman_decode_ragged_jump_kernel<STACK, LONG, 4, true>, a.sel.n_pieces, lds, hs, a);
}

cst_status decode_select(bool stack, bool lng, const HrSelArgs& a, int32_t symbol_bytes, size_t lds, hipStream_t hs) {
    if (stack) return lng ? decode_select_sb<true, true>(a, symbol_bytes, lds, hs) : decode_select_sb<true, false>(a, symbol_bytes, lds, hs);
    return lng ? decode_select_sb<false, true>(a, symbol_bytes, lds, hs) : decode_select_sb<false, false>(a, symbol_bytes, lds, hs);
}

inline bool semantics_ok(int32_t semantics) { return semantics == CST_HUFFMAN_STACK || semantics == CST_HUFFMAN_QUEUE; }
inline bool width_ok(int32_t symbol_bytes) { return symbol_bytes == 1 || symbol_bytes == 4; }
// chunks of 32 .. 2^31 - 32 symbols, a multiple of the symbol tile's width
inline bool interval_ok(size_t interval) { return interval > 0 && interval % kTile == 0 && interval <= 0x7fffffffull; }

cst_status encode_ragged_args(const void* cb, int32_t semantics, const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets,
                              uint32_t* d_words, uint32_t* d_n_words, int32_t* d_status) {
    if (!valid_cb(cb) || !d_symbols || !d_sym_offsets || !d_words || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!semantics_ok(semantics) || !width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    return CST_OK;
}

cst_status decode_ragged_args(const void* cb, int32_t semantics, const uint32_t* d_words, const uint32_t* d_n_words, void* d_symbols,
                              int32_t symbol_bytes, const uint64_t* d_sym_offsets, int32_t* d_status) {
    if (!valid_cb(cb) || !d_words || !d_n_words || !d_symbols || !d_sym_offsets || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!semantics_ok(semantics) || !width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (symbol_bytes == 1 && static_cast<const HuffCodebook*>(cb)->n > 256) return CST_ERR_INVALID_ARGUMENT;    // the alphabet does not fit the type
    return CST_OK;
}

HrEncArgs enc_args(const HuffCodebook* c, int32_t semantics, const void* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams,
                   uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, uint32_t* d_n_words, uint64_t* d_n_bits,
                   int32_t* d_status) {
    HrEncArgs a{};
    a.pool = c->d_pool[semantics == CST_HUFFMAN_QUEUE];
    a.enc = c->d_enc[semantics == CST_HUFFMAN_QUEUE];
    a.n_sym = (uint32_t)c->n;
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words;
    a.n_words = d_n_words; a.n_bits = d_n_bits; a.status = d_status;
    a.vec = (reinterpret_cast<uintptr_t>(d_words) & 15u) == 0 && (d_word_offsets || stride_words % 4 == 0);
    return a;
}

HrDecArgs dec_args(const HuffCodebook* c, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words, size_t words_capacity,
                   const uint32_t* d_n_words, void* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status) {
    HrDecArgs a{};
    a.lut = c->d_lut; a.child = c->d_child; a.n_sym = (uint32_t)c->n; a.lut_bits = c->lut_bits;
    a.words = d_words; a.word_offsets = d_word_offsets; a.stride = stride_words; a.capacity = words_capacity; a.n_words = d_n_words;
    a.symbols = d_symbols; a.sym_offsets = d_sym_offsets; a.n_streams = n_streams; a.status = d_status;
    return a;
}

inline size_t lut_bytes(const HuffCodebook* c) { return ((sizeof(uint32_t) << c->lut_bits) + 15) & ~(size_t)15; }

} // namespace

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_huffman_count_bits(const void* cb, const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets, size_t n_streams,
                                  size_t n_per_stream, uint64_t* d_n_bits, void* stream) {
    if (!valid_cb(cb) || !width_ok(symbol_bytes) || !d_n_bits) return CST_ERR_INVALID_ARGUMENT;
    if (!d_symbols && (d_sym_offsets || n_per_stream > 0)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    const size_t per_block = kBlock / kWave;
    const size_t blocks = std::min<size_t>((n_streams + per_block - 1) / per_block, 16384);
    const uint2* enc = c->d_enc[0];          // (a codeword is as long in either bit order)
    const uint32_t n_sym = (uint32_t)c->n;
    if (symbol_bytes == 1) hipLaunchKernelGGL(huffman_count_bits_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, hs, enc, n_sym, d_symbols, d_sym_offsets, n_streams, n_per_stream, d_n_bits);
    else hipLaunchKernelGGL(huffman_count_bits_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, hs, enc, n_sym, d_symbols, d_sym_offsets, n_streams, n_per_stream, d_n_bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) set_hip_error(e, "huffman_count_bits_kernel");
    return note_kernel("huffman_count_bits_kernel", e == hipSuccess ? CST_OK : CST_ERR_HIP);
}

cst_status cst_huffman_encode_ragged(const void* cb, int32_t semantics, const void* d_symbols, int32_t symbol_bytes, const uint64_t* d_sym_offsets,
                                     size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                     uint32_t* d_n_words, uint64_t* d_n_bits, int32_t* d_status, void* stream) {
    const cst_status rc = encode_ragged_args(cb, semantics, d_symbols, symbol_bytes, d_sym_offsets, d_words, d_n_words, d_status);
    if (rc != CST_OK) return rc;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    const HrEncArgs a = enc_args(c, semantics, d_symbols, d_sym_offsets, n_streams, d_words, d_word_offsets, stride_words, d_n_words, d_n_bits, d_status);
    return encode_ragged<false>(c, semantics, a, symbol_bytes, (hipStream_t)stream);
}

cst_status cst_huffman_decode_ragged(const void* cb, int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets, size_t stride_words,
                                     size_t words_capacity, const uint32_t* d_n_words, void* d_symbols, int32_t symbol_bytes,
                                     const uint64_t* d_sym_offsets, size_t n_streams, int32_t* d_status, void* stream) {
    const cst_status rc = decode_ragged_args(cb, semantics, d_words, d_n_words, d_symbols, symbol_bytes, d_sym_offsets, d_status);
    if (rc != CST_OK) return rc;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    const HrDecArgs a = dec_args(c, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams, d_status);
    hipStream_t hs = (hipStream_t)stream;
    const bool lng = c->max_len > c->lut_bits;
    return note_kernel(lng ? "huffman_decode_ragged_long_kernel" : "huffman_decode_ragged_kernel",
                       CST_HR_DECODE(huffman_decode_ragged_kernel, n_streams, lut_bytes(c)));
}

cst_status cst_huffman_encode_ragged_jump(const void* cb, int32_t semantics, const void* d_symbols, int32_t symbol_bytes,
                                          const uint64_t* d_sym_offsets, size_t n_streams, uint32_t* d_words, const uint64_t* d_word_offsets,
                                          size_t stride_words, uint32_t* d_n_words, uint64_t* d_n_bits, size_t jump_interval,
                                          const uint64_t* d_chunk_offsets, uint64_t* d_jump_bits, int32_t* d_status, void* stream) {
    const cst_status rc = encode_ragged_args(cb, semantics, d_symbols, symbol_bytes, d_sym_offsets, d_words, d_n_words, d_status);
    if (rc != CST_OK) return rc;
    if (!interval_ok(jump_interval) || !d_chunk_offsets || !d_jump_bits) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    HrEncArgs a = enc_args(c, semantics, d_symbols, d_sym_offsets, n_streams, d_words, d_word_offsets, stride_words, d_n_words, d_n_bits, d_status);
    a.interval = jump_interval; a.chunk_offsets = d_chunk_offsets; a.jump_bits = d_jump_bits;
    return encode_ragged<true>(c, semantics, a, symbol_bytes, (hipStream_t)stream);
}

cst_status cst_huffman_decode_ragged_jump(const void* cb, int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                          size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, void* d_symbols,
                                          int32_t symbol_bytes, const uint64_t* d_sym_offsets, size_t n_streams, size_t jump_interval,
                                          const uint64_t* d_chunk_offsets, size_t n_chunks_total, const uint64_t* d_jump_bits,
                                          int32_t* d_status, void* stream) {
    const cst_status rc = decode_ragged_args(cb, semantics, d_words, d_n_words, d_symbols, symbol_bytes, d_sym_offsets, d_status);
    if (rc != CST_OK) return rc;
    if (!interval_ok(jump_interval) || !d_chunk_offsets || !d_jump_bits) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    HrDecArgs a = dec_args(c, d_words, d_word_offsets, stride_words, words_capacity, d_n_words, d_symbols, d_sym_offsets, n_streams, d_status);
    a.interval = jump_interval; a.chunk_offsets = d_chunk_offsets; a.n_chunks_total = n_chunks_total; a.jump_bits = d_jump_bits;
    hipStream_t hs = (hipStream_t)stream;
    CST_HIP_TRY(hipMemsetAsync(d_status, 0, n_streams * sizeof(int32_t), hs));      // CST_STREAM_OK: the kernel only raises it
    const bool lng = c->max_len > c->lut_bits;
    const size_t lanes = std::max(n_streams, n_chunks_total);      // a lane per chunk, and one per stream for the table's check
    return note_kernel(lng ? "huffman_decode_ragged_jump_long_kernel" : "huffman_decode_ragged_jump_kernel",
                       CST_HR_DECODE(huffman_decode_ragged_jump_kernel, lanes, lut_bytes(c) + kJumpTileBytesPerBlock));
}

cst_status cst_huffman_decode_ragged_select(const void* cb, int32_t semantics, const uint32_t* d_words, const uint64_t* d_word_offsets,
                                            size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, const uint64_t* d_sym_offsets,
                                            size_t n_streams, size_t jump_interval, const uint64_t* d_chunk_offsets, size_t n_chunks_total,
                                            const uint64_t* d_jump_bits, const uint32_t* d_query_stream, const uint64_t* d_query_first,
                                            const uint64_t* d_query_count, size_t n_queries, const uint64_t* d_piece_offsets,
                                            size_t n_pieces_total, void* d_symbols_out, int32_t symbol_bytes, const uint64_t* d_out_offsets,
                                            void* d_scratch, int32_t* d_status, void* stream) {
    if (!valid_cb(cb) || !d_words || !d_n_words || !d_sym_offsets) return CST_ERR_INVALID_ARGUMENT;
    if (!semantics_ok(semantics) || !width_ok(symbol_bytes)) return CST_ERR_INVALID_ARGUMENT;
    if (symbol_bytes == 1 && static_cast<const HuffCodebook*>(cb)->n > 256) return CST_ERR_INVALID_ARGUMENT;    // the alphabet does not fit the type
    const int table = (d_chunk_offsets != nullptr) + (d_jump_bits != nullptr);
    if (!symbol_select_args_ok(jump_interval, table, n_chunks_total, d_query_first, d_query_count, n_pieces_total)) return CST_ERR_INVALID_ARGUMENT;
    if (n_queries > 0 && (!d_query_stream || !d_piece_offsets || !d_symbols_out || !d_out_offsets || !d_scratch || !d_status))
        return CST_ERR_INVALID_ARGUMENT;
    if (n_queries == 0) return CST_OK;
    if (n_queries > ((size_t)0x7fffffff) * 256) return CST_ERR_INVALID_ARGUMENT;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    const RaggedSelect b = symbol_select_batch(d_word_offsets, stride_words, words_capacity, d_n_words, d_sym_offsets, n_streams, jump_interval,
                                               d_chunk_offsets, n_chunks_total, d_query_stream, d_query_first, d_query_count, n_queries,
                                               d_piece_offsets, n_pieces_total, d_out_offsets);
    const RaggedSelectPieces v(d_scratch, n_pieces_total);
    HrSelArgs a{};
    a.lut = c->d_lut; a.child = c->d_child; a.n_sym = (uint32_t)c->n; a.lut_bits = c->lut_bits;
    a.words = d_words; a.symbols = d_symbols_out;
    a.sel = symbol_select_lanes(v, d_jump_bits, n_pieces_total);
    hipStream_t hs = (hipStream_t)stream;
    const bool stack = semantics == CST_HUFFMAN_STACK, lng = c->max_len > c->lut_bits;
    return note_kernel(lng ? "huffman_decode_ragged_jump_long_kernel<select>" : "huffman_decode_ragged_jump_kernel<select>",
                       symbol_select_run(stack, b, d_words, d_jump_bits, v, d_status, hs, [&] {
                           return decode_select(stack, lng, a, symbol_bytes, lut_bytes(c) + kJumpTileBytesPerBlock, hs);
                       }));
}

}  // extern "C"
