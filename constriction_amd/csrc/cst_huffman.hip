// cst_huffman.hip -- Huffman symbol codes (the reference's constriction.symbol: src/symbol/huffman.rs, src/symbol/mod.rs):
// the host tree construction, the device codebook and the batched stack / queue coders (streams of different lengths:
// cst_huffman_ragged.hip; what the two files share: cst_huffman.hpp).
//
// One lane codes one stream against a codebook shared by the whole batch.  The bit containers are the reference's
// (symbol/mod.rs:376-393, 438-455, 600-617, 642-655): bits are written from bit 0 of a u32 word upwards; a queue is read
// front to back from bit 0 upwards, a stack from the last written bit downwards.  The encoder keeps a 64-bit accumulator
// per lane and emits a word whenever 32 or more bits are pending; the decoder keeps a 64-bit window of the next bits
// (low end first for a queue, high end first for a stack), looks the first kLutBits of it up in a table held in LDS and,
// for a longer codeword, walks the inner nodes from where the table left off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <queue>
#include <vector>

#include "cst_huffman.hpp"

namespace cst {

namespace {

void free_cb(HuffCodebook* c) {
    for (int k = 0; k < 2; ++k) {
        if (c->d_enc[k]) (void)hipFree(c->d_enc[k]);
        if (c->d_pool[k]) (void)hipFree(c->d_pool[k]);
    }
    if (c->d_lut) (void)hipFree(c->d_lut);
    if (c->d_child) (void)hipFree(c->d_child);
    c->magic = 0;
    delete c;
}

struct EncArgs {
    const uint2* enc;
    const uint32_t* pool;
    uint32_t n_sym;
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

struct DecArgs {
    const uint32_t* lut;
    const uint32_t* child;
    uint32_t n_sym;
    int32_t lut_bits;
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

// wave-private LDS tiles: 64 stream rows x kTile symbols (row stride kTileStride words, conflict-free for both the row-wise
// fill and the lane-per-row reads).  The encoder stages its symbols through one, the decoder its decoded symbols.
constexpr int kTileStride = kTile + 1;
constexpr size_t kTileBytesPerBlock = (size_t)(kBlock / kWave) * kWave * kTileStride * sizeof(uint32_t);

// symbols [t0, t0 + tlen) of the wave's 64 rows -> tile.  Lane l reads column (l & 31) of rows (l >> 5) + 2k: every load
// instruction reads two contiguous row segments (128 B of int32, 32 B of uint8) instead of 64 scattered elements.
template <int SB>
__device__ __forceinline__ void tile_fill(const void* sym, size_t n_streams, size_t n, size_t s0, size_t t0, uint32_t tlen, int lane,
                                          uint32_t* tile) {
    const uint32_t col = (uint32_t)lane & 31u;
    uint32_t r[kTile / 2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int k = 0; k < kTile / 2; ++k) {
            const int row = (lane >> 5) + 2 * (k + half * (kTile / 2));
            const size_t s = s0 + (size_t)row;
            r[k] = (s < n_streams && col < tlen) ? load_sym<SB>(sym, s * n + t0 + col) : 0u;
        }
#pragma unroll
        for (int k = 0; k < kTile / 2; ++k) tile[((lane >> 5) + 2 * (k + half * (kTile / 2))) * kTileStride + col] = r[k];
    }
}

// tile -> symbols [t0, t0 + tlen) of the wave's 64 rows (the mirror image of tile_fill)
template <int SB>
__device__ __forceinline__ void tile_drain(void* sym, size_t n_streams, size_t n, size_t s0, size_t t0, uint32_t tlen, int lane,
                                           const uint32_t* tile) {
    const uint32_t col = (uint32_t)lane & 31u;
#pragma unroll 8
    for (int k = 0; k < kWave / 2; ++k) {
        const int row = (lane >> 5) + 2 * k;
        const size_t s = s0 + (size_t)row;
        if (s < n_streams && col < tlen) store_sym<SB>(sym, s * n + t0 + col, tile[row * kTileStride + col]);
    }
}

// dynamic LDS: [codeword table (LDS_TAB), 16-B aligned] [one symbol tile per wave]
template <bool STACK, bool LONG, bool LDS_TAB, int SB>
__global__ void __launch_bounds__(kBlock) huffman_encode_kernel(EncArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_enc_lds[];
    const uint2* enc = a.enc;
    uint32_t* tiles = s_enc_lds;
    if constexpr (LDS_TAB) {
        uint2* t = reinterpret_cast<uint2*>(s_enc_lds);
        for (uint32_t i = threadIdx.x; i < a.n_sym; i += kBlock) t[i] = a.enc[i];
        __syncthreads();
        enc = t;
        tiles = s_enc_lds + ((2 * (size_t)a.n_sym + 3) & ~(size_t)3);
    }
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s0 = (size_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1));
    if (s0 >= a.n_streams) return;                  // (wave-uniform: the whole wave lies past the batch)
    uint32_t* tile = tiles + (size_t)(threadIdx.x / kWave) * kWave * kTileStride;
    const size_t s = s0 + (size_t)lane;
    const bool valid = s < a.n_streams;
    WordSink sink{a.words + s * a.stride, a.stride, 0u, make_uint4(0, 0, 0, 0), a.vec};
    uint64_t acc = 0;
    uint32_t nb = 0;
    int32_t st = valid ? CST_STREAM_OK : CST_STREAM_INVALID_DATA;
    if (valid && a.cont) {
        const uint64_t c = a.cont[s];
        nb = (uint32_t)(c >> 32);
        acc = c & 0xffffffffull;
        if (nb >= 32) st = CST_STREAM_INVALID_DATA;
        else acc &= (1ull << nb) - 1;
    }
    const size_t n = a.n_per;
    const uint32_t* my = tile + lane * kTileStride;
    for (size_t done = 0; done < n; done += kTile) {
        // queue: tiles front to back; stack: back to front, each read from its end
        const size_t t0 = STACK ? (n - done > (size_t)kTile ? n - done - kTile : 0) : done;
        const uint32_t tlen = (uint32_t)((n - done) < (size_t)kTile ? (n - done) : (size_t)kTile);
        wave_lds_fence();
        tile_fill<SB>(a.symbols, a.n_streams, n, s0, t0, tlen, lane, tile);
        wave_lds_fence();
        if (st != CST_STREAM_OK) continue;
        for (uint32_t j = 0; j < tlen; ++j) {
            const uint32_t x = my[STACK ? tlen - 1 - j : j];
            if (x >= a.n_sym) { st = CST_STREAM_IMPOSSIBLE_SYMBOL; break; }
            if (!put_symbol<LONG>(enc[x], a.pool, acc, nb, sink)) { st = CST_STREAM_CAPACITY; break; }
        }
    }
    if (!valid) return;
    const uint64_t bits = 32ull * sink.nw + nb;   // the reference's len(): written bits, without the seal
    if (st == CST_STREAM_OK && !a.cont) {
        if (STACK && !put_bits(1u, 1u, acc, nb, sink)) st = CST_STREAM_CAPACITY;   // the seal (mod.rs:264-283)
        if (st == CST_STREAM_OK && nb > 0 && !sink.put((uint32_t)acc)) st = CST_STREAM_CAPACITY;
    }
    if (st != CST_STREAM_OK) {
        a.n_words[s] = 0;
        if (a.n_bits) a.n_bits[s] = 0;
    } else {
        sink.finish();
        a.n_words[s] = sink.nw;
        if (a.n_bits) a.n_bits[s] = bits;
        if (a.cont) a.cont[s] = (acc & 0xffffffffull) | ((uint64_t)nb << 32);
    }
    a.status[s] = st;
}

// dynamic LDS: [decode table, 2^lut_bits words] [one output tile per wave]
template <bool STACK, bool LONG, int SB>
__global__ void __launch_bounds__(kBlock) huffman_decode_kernel(DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dec_lds[];
    uint32_t* s_lut = s_dec_lds;
    const uint32_t lut_n = 1u << a.lut_bits;
    for (uint32_t i = threadIdx.x; i < lut_n; i += kBlock) s_lut[i] = a.lut[i];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const size_t s0 = (size_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1));
    if (s0 >= a.n_streams) return;                  // (wave-uniform)
    uint32_t* tile = s_dec_lds + ((lut_n + 3) & ~3u) + (size_t)(threadIdx.x / kWave) * kWave * kTileStride;
    const size_t s = s0 + (size_t)lane;
    const bool valid = s < a.n_streams;
    const uint32_t lmask = lut_n - 1u;
    const uint32_t L = (uint32_t)a.lut_bits;
    size_t base = 0, nw = 0;
    int32_t st = CST_STREAM_OK;
    if (valid) {
        base = a.offsets ? (size_t)a.offsets[s] : s * a.stride;
        nw = a.n_words[s];
        if ((!a.offsets && nw > a.stride) || (a.capacity && (base > a.capacity || nw > a.capacity - base))) {
            st = CST_STREAM_INVALID_DATA;
            nw = 0;
        }
    } else {
        st = CST_STREAM_INVALID_DATA;
    }
    const uint32_t* w = a.words + base;
    uint64_t buf = 0;     // queue: the next bits from bit 0 up; stack: the next bits from bit 63 down
    uint32_t have = 0;    // valid bits in buf
    size_t wi = 0;        // queue: next word to load; stack: words below the window still to load
    if (st == CST_STREAM_OK) {
        if (STACK) {
            if (a.cont) {
                const uint64_t c = a.cont[s];
                have = (uint32_t)(c >> 32);
                if (have >= 32) st = CST_STREAM_INVALID_DATA;
                else buf = have ? (uint64_t)(uint32_t)c << (64 - have) : 0ull;
                wi = nw;
            } else if (nw == 0 || w[nw - 1] == 0u) {
                st = CST_STREAM_INVALID_DATA;   // no words, or a trailing zero word: no seal (mod.rs:478-497)
            } else {
                // the seal is the HIGHEST set bit of the last word (where the writer put it)
                const uint32_t last = w[nw - 1];
                have = 31u - (uint32_t)__clz(last);
                buf = have ? (uint64_t)last << (64 - have) : 0ull;
                wi = nw - 1;
            }
        } else {
            const uint64_t p = a.cont ? a.cont[s] : 0ull;
            if (p > 32ull * nw) {
                st = CST_STREAM_INVALID_DATA;
            } else {
                wi = (size_t)(p >> 5);
                if ((p & 31u) != 0) {
                    buf = w[wi++] >> (p & 31u);
                    have = 32u - (uint32_t)(p & 31u);
                }
            }
        }
    }
    if (st != CST_STREAM_OK) { wi = 0; have = 0; nw = 0; }
    // the next word to enter the window, loaded one refill ahead so that its latency overlaps the symbols before it
    uint32_t pf = STACK ? (wi > 0 ? w[wi - 1] : 0u) : (wi < nw ? w[wi] : 0u);
    const size_t n = a.n_per;
    for (size_t t0 = 0; t0 < n; t0 += kTile) {
        const uint32_t tlen = (uint32_t)((n - t0) < (size_t)kTile ? (n - t0) : (size_t)kTile);
        for (uint32_t j = 0; j < tlen; ++j) {
            uint32_t sym = 0;          // (after an error: 0)
            if (st == CST_STREAM_OK) {
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
                    if (len > have) {
                        st = CST_STREAM_OUT_OF_DATA;   // (have < 32 only once the words are exhausted)
                    } else {
                        buf = STACK ? buf << len : buf >> len;
                        have -= len;
                        sym = e & ((1u << kLutLenShift) - 1u);
                    }
                } else if (L > have) {
                    st = CST_STREAM_OUT_OF_DATA;
                } else {
                    buf = STACK ? buf << L : buf >> L;
                    have -= L;
                    uint32_t node = e & ((1u << kLutLenShift) - 1u);
                    while (node >= a.n_sym) {
                        if (have == 0) {
                            if (STACK ? wi == 0 : wi >= nw) break;
                            if (STACK) { buf = (uint64_t)pf << 32; --wi; pf = wi > 0 ? w[wi - 1] : 0u; }
                            else { buf = pf; ++wi; pf = wi < nw ? w[wi] : 0u; }
                            have = 32;
                        }
                        const uint32_t bit = STACK ? (uint32_t)(buf >> 63) : (uint32_t)buf & 1u;
                        buf = STACK ? buf << 1 : buf >> 1;
                        --have;
                        node = a.child[2u * (node - a.n_sym) + bit];
                    }
                    if (node >= a.n_sym) st = CST_STREAM_OUT_OF_DATA;
                    else sym = node;
                }
            }
            tile[lane * kTileStride + j] = sym;
        }
        wave_lds_fence();
        tile_drain<SB>(a.symbols, a.n_streams, n, s0, t0, tlen, lane, tile);
        wave_lds_fence();
    }
    if (!valid) return;
    if (st == CST_STREAM_OUT_OF_DATA) {      // the reference has read every bit when it reports the end of the data
        if (STACK) { wi = 0; have = 0; }
        else { wi = nw; have = 0; }
    }
    a.status[s] = st;
    if (STACK) {
        const uint64_t remaining = 32ull * wi + have;
        const uint32_t r = (uint32_t)(remaining & 31u);
        if (a.n_words_out) a.n_words_out[s] = (uint32_t)(remaining >> 5);
        if (a.cont) a.cont[s] = r ? ((buf >> (64 - r)) | ((uint64_t)r << 32)) : 0ull;
    } else {
        const uint64_t pos = 32ull * wi - have;
        if (a.n_words_out) a.n_words_out[s] = (uint32_t)((pos + 31) >> 5);
        if (a.cont) a.cont[s] = pos;
    }
}

template <bool STACK, bool LONG>
cst_status encode_sb(const EncArgs& a, int32_t symbol_bytes, hipStream_t hs) {
    const size_t tab = ((size_t)a.n_sym * sizeof(uint2) + 15) & ~(size_t)15;
    if (tab <= kEncLdsBytes) {
        if (symbol_bytes == 1) return launch_huff(huffman_encode_kernel<STACK, LONG, true, 1>, a.n_streams, tab + kTileBytesPerBlock, hs, a);
        return launch_huff(huffman_encode_kernel<STACK, LONG, true, 4>, a.n_streams, tab + kTileBytesPerBlock, hs, a);
    }
    if (symbol_bytes == 1) return launch_huff(huffman_encode_kernel<STACK, LONG, false, 1>, a.n_streams, kTileBytesPerBlock, hs, a);
    return launch_huff(huffman_encode_kernel<STACK, LONG, false, 4>, a.n_streams, kTileBytesPerBlock, hs, a);
}

template <bool STACK, bool LONG>
cst_status decode_sb(const DecArgs& a, int32_t symbol_bytes, hipStream_t hs) {
    const size_t lds = (((sizeof(uint32_t) << a.lut_bits) + 15) & ~(size_t)15) + kTileBytesPerBlock;
    if (symbol_bytes == 1) return launch_huff(huffman_decode_kernel<STACK, LONG, 1>, a.n_streams, lds, hs, a);
    return launch_huff(huffman_decode_kernel<STACK, LONG, 4>, a.n_streams, lds, hs, a);
}

} // namespace

} // namespace cst

using namespace cst;

extern "C" {

// src/symbol/huffman.rs:62-116 (EncoderHuffmanTree::try_from_probabilities): pop the two smallest (probability, index)
// pairs -- the first becomes bit 0, the second bit 1 -- and push their sum as node n, n+1, ...; the sum in the input's
// float type (f32_sums: every value rounded to f32, every sum an f32 addition).
cst_status cst_huffman_tree(const double* h_probs, size_t n, int32_t f32_sums, uint64_t* h_nodes) {
    if (!h_probs || !h_nodes) return CST_ERR_INVALID_ARGUMENT;
    if (n == 0 || n > ((size_t)1 << 60)) return CST_ERR_MODEL;
    using Item = std::pair<double, uint64_t>;
    std::vector<Item> items(n);
    for (size_t i = 0; i < n; ++i) {
        double p = h_probs[i];
        if (!(p >= 0.0) || std::isinf(p)) return CST_ERR_MODEL;     // NaN, negative, infinite
        if (f32_sums) {
            p = (double)(float)p;
            if (std::isinf(p)) return CST_ERR_MODEL;
        }
        items[i] = Item(p, (uint64_t)i);
    }
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap(std::greater<Item>(), std::move(items));
    std::fill(h_nodes, h_nodes + (2 * n - 1), 0ull);
    uint64_t next = n;
    while (heap.size() >= 2) {
        const Item a = heap.top(); heap.pop();
        const Item b = heap.top(); heap.pop();
        const double sum = f32_sums ? (double)((float)a.first + (float)b.first) : a.first + b.first;
        heap.push(Item(sum, next));
        h_nodes[a.second] = next << 1;
        h_nodes[b.second] = (next << 1) | 1u;
        ++next;
    }
    return CST_OK;
}

cst_status cst_huffman_codebook_create(const uint64_t* h_nodes, size_t n, void* stream, void** out) {
    if (!out) return CST_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!h_nodes || n == 0 || n > CST_HUFFMAN_MAX_SYMBOLS) return CST_ERR_INVALID_ARGUMENT;
    const size_t n_nodes = 2 * n - 1, root = n_nodes - 1;
    // the tree: every node but the root names a parent that comes after it (the construction numbers parents after their
    // children, which also rules out cycles) and every child slot is taken exactly once
    std::vector<uint32_t> child(2 * (n - 1) + 2, 0xffffffffu);
    std::vector<int32_t> depth(n_nodes, 0);
    if (h_nodes[root] != 0) return CST_ERR_MODEL;
    for (size_t i = 0; i < root; ++i) {
        const uint64_t parent = h_nodes[i] >> 1, bit = h_nodes[i] & 1u;
        if (parent < n || parent > root || parent <= i) return CST_ERR_MODEL;
        uint32_t& slot = child[2 * (parent - n) + bit];
        if (slot != 0xffffffffu) return CST_ERR_MODEL;
        slot = (uint32_t)i;
    }
    int32_t max_len = 0;
    for (size_t i = root; i-- > 0;) {
        depth[i] = depth[h_nodes[i] >> 1] + 1;
        if (i < n) max_len = std::max(max_len, depth[i]);
    }
    // codewords: suffix order (leaf to root, what the stack writes) and prefix order (root to leaf, the queue)
    std::vector<uint2> enc[2] = {std::vector<uint2>(n), std::vector<uint2>(n)};
    std::vector<uint32_t> pool[2];
    std::vector<uint8_t> bits;
    for (size_t s = 0; s < n; ++s) {
        const uint32_t len = (uint32_t)depth[s];
        bits.clear();
        for (size_t v = s; v != root; v = h_nodes[v] >> 1) bits.push_back((uint8_t)(h_nodes[v] & 1u));   // suffix order
        for (int k = 0; k < 2; ++k) {
            auto bit_at = [&](uint32_t j) { return k == 0 ? bits[j] : bits[len - 1 - j]; };
            if (len <= 32) {
                uint32_t code = 0;
                for (uint32_t j = 0; j < len; ++j) code |= (uint32_t)bit_at(j) << j;
                enc[k][s] = make_uint2(code, len);
            } else {
                if (pool[k].size() + (len + 31) / 32 > 0xffffffffull) return CST_ERR_INVALID_ARGUMENT;
                const size_t off = pool[k].size();
                pool[k].resize(off + (len + 31) / 32, 0u);
                for (uint32_t j = 0; j < len; ++j) pool[k][off + j / 32] |= (uint32_t)bit_at(j) << (j % 32);
                enc[k][s] = make_uint2((uint32_t)off, len);
            }
        }
    }
    // decode table of the first lut_bits bits (bit j of the index = the j-th bit read)
    const int32_t lut_bits = std::min(kLutBits, max_len);
    std::vector<uint32_t> lut((size_t)1 << lut_bits, 0u);
    struct Visit { uint32_t node, depth, prefix; };
    std::vector<Visit> todo{{(uint32_t)root, 0u, 0u}};
    while (!todo.empty()) {
        const Visit v = todo.back();
        todo.pop_back();
        if (v.node < n) {
            for (uint32_t ext = 0; ext < (1u << (lut_bits - v.depth)); ++ext)
                lut[v.prefix | (ext << v.depth)] = v.node | (v.depth << kLutLenShift);
        } else if ((int32_t)v.depth == lut_bits) {
            lut[v.prefix] = v.node | kLutCont;
        } else {
            for (uint32_t b = 0; b < 2; ++b)
                todo.push_back({child[2 * (v.node - n) + b], v.depth + 1, v.prefix | (b << v.depth)});
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return CST_ERR_NO_DEVICE;
    HuffCodebook* c = new (std::nothrow) HuffCodebook();
    if (!c) return CST_ERR_OUT_OF_MEMORY;
    c->n = (int32_t)n; c->max_len = max_len; c->lut_bits = lut_bits;
    hipGetDevice(&c->device);
    hipStream_t hs = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    auto upload = [&](auto** dst, const auto* src, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, hs);
    };
    for (int k = 0; k < 2; ++k) {
        upload(&c->d_enc[k], enc[k].data(), enc[k].size() * sizeof(uint2));
        upload(&c->d_pool[k], pool[k].data(), pool[k].size() * sizeof(uint32_t));
    }
    upload(&c->d_lut, lut.data(), lut.size() * sizeof(uint32_t));
    upload(&c->d_child, child.data(), 2 * (n - 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipStreamSynchronize(hs);     // the host vectors must outlive the copies
    if (e != hipSuccess) {
        set_hip_error(e, "huffman codebook upload");
        free_cb(c);
        return e == hipErrorOutOfMemory ? CST_ERR_OUT_OF_MEMORY : CST_ERR_HIP;
    }
    *out = c;
    return CST_OK;
}

cst_status cst_huffman_codebook_destroy(void* cb) {
    if (!cb) return CST_OK;
    if (!valid_cb(cb)) return CST_ERR_INVALID_ARGUMENT;
    free_cb(static_cast<HuffCodebook*>(cb));
    return CST_OK;
}

size_t cst_huffman_max_words(const void* cb, size_t n_per_stream, int32_t semantics) {
    if (!valid_cb(cb) || (semantics != CST_HUFFMAN_STACK && semantics != CST_HUFFMAN_QUEUE)) return 0;
    const size_t len = (size_t)static_cast<const HuffCodebook*>(cb)->max_len;
    if (len && n_per_stream > (SIZE_MAX - 1024) / len) return 0;
    // every codeword at its longest + up to 31 bits a continued call starts with + the seal of a stack, in whole 64-byte units
    const size_t words = (n_per_stream * len + 32 + 31) / 32;
    return (words + 15) / 16 * 16;
}

cst_status cst_huffman_encode_batch(const void* cb, int32_t semantics, const void* d_symbols, int32_t symbol_bytes,
                                    size_t n_streams, size_t n_per_stream, uint32_t* d_words, size_t stride_words,
                                    uint32_t* d_n_words, uint64_t* d_n_bits, uint64_t* d_cont, int32_t* d_status, void* stream) {
    if (!valid_cb(cb) || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (!d_words && stride_words) return CST_ERR_INVALID_ARGUMENT;      // (no slab at all: every stream needs none or reports CAPACITY)
    if (semantics != CST_HUFFMAN_STACK && semantics != CST_HUFFMAN_QUEUE) return CST_ERR_INVALID_ARGUMENT;
    if (symbol_bytes != 1 && symbol_bytes != 4) return CST_ERR_INVALID_ARGUMENT;
    if (n_per_stream > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    EncArgs a{};
    a.pool = c->d_pool[semantics == CST_HUFFMAN_QUEUE];
    a.enc = c->d_enc[semantics == CST_HUFFMAN_QUEUE];
    a.n_sym = (uint32_t)c->n;
    a.symbols = d_symbols; a.n_streams = n_streams; a.n_per = n_per_stream;
    a.words = d_words; a.stride = stride_words; a.n_words = d_n_words; a.n_bits = d_n_bits; a.cont = d_cont; a.status = d_status;
    a.vec = stride_words % 4 == 0 && (reinterpret_cast<uintptr_t>(d_words) & 15u) == 0;
    hipStream_t hs = (hipStream_t)stream;
    const bool lng = c->max_len > 32;
    if (semantics == CST_HUFFMAN_STACK)
        return lng ? note_kernel("huffman_encode_long_kernel", encode_sb<true, true>(a, symbol_bytes, hs))
                   : note_kernel("huffman_encode_kernel", encode_sb<true, false>(a, symbol_bytes, hs));
    return lng ? note_kernel("huffman_encode_long_kernel", encode_sb<false, true>(a, symbol_bytes, hs))
               : note_kernel("huffman_encode_kernel", encode_sb<false, false>(a, symbol_bytes, hs));
}

cst_status cst_huffman_decode_batch(const void* cb, int32_t semantics, const uint32_t* d_words, const uint64_t* d_offsets,
                                    size_t stride_words, size_t words_capacity, const uint32_t* d_n_words, void* d_symbols,
                                    int32_t symbol_bytes, size_t n_streams, size_t n_per_stream, uint64_t* d_cont,
                                    uint32_t* d_n_words_out, int32_t* d_status, void* stream) {
    if (!valid_cb(cb) || !d_n_words || !d_status) return CST_ERR_INVALID_ARGUMENT;
    if (semantics != CST_HUFFMAN_STACK && semantics != CST_HUFFMAN_QUEUE) return CST_ERR_INVALID_ARGUMENT;
    if (symbol_bytes != 1 && symbol_bytes != 4) return CST_ERR_INVALID_ARGUMENT;
    if (n_per_stream > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    const HuffCodebook* c = static_cast<const HuffCodebook*>(cb);
    if (symbol_bytes == 1 && c->n > 256) return CST_ERR_INVALID_ARGUMENT;    // the alphabet does not fit the type
    if (!d_words && (d_offsets || stride_words)) return CST_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return CST_OK;
    if (!on_device(c)) return CST_ERR_INVALID_ARGUMENT;
    DecArgs a{};
    a.lut = c->d_lut; a.child = c->d_child; a.n_sym = (uint32_t)c->n; a.lut_bits = c->lut_bits;
    a.words = d_words;     // (NULL: every stream must be empty, nothing is read)
    a.offsets = d_offsets; a.stride = stride_words; a.capacity = words_capacity; a.n_words = d_n_words;
    a.symbols = d_symbols; a.n_streams = n_streams; a.n_per = n_per_stream;
    a.cont = d_cont; a.n_words_out = d_n_words_out; a.status = d_status;
    hipStream_t hs = (hipStream_t)stream;
    const bool lng = c->max_len > c->lut_bits;
    if (semantics == CST_HUFFMAN_STACK)
        return lng ? note_kernel("huffman_decode_long_kernel", decode_sb<true, true>(a, symbol_bytes, hs))
                   : note_kernel("huffman_decode_kernel", decode_sb<true, false>(a, symbol_bytes, hs));
    return lng ? note_kernel("huffman_decode_long_kernel", decode_sb<false, true>(a, symbol_bytes, hs))
               : note_kernel("huffman_decode_kernel", decode_sb<false, false>(a, symbol_bytes, hs));
}

}  // extern "C"
