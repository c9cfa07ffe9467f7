// cst_huffman.hpp -- what the Huffman translation units share (cst_huffman.hip: codebooks and the rectangular coders;
// cst_huffman_ragged.hip: streams of different lengths and their jump points): the device codebook, the decode table's
// constants and the write side of a bit container.
#pragma once

#include "cst_common.hpp"

namespace cst {

namespace {

constexpr int kLutBits = 12;                  // decode table: 2^12 entries x 4 B = 16 KiB of LDS
constexpr uint32_t kLutCont = 0x80000000u;    // entry is an inner node: the codeword is longer than the table's bits
constexpr int kLutLenShift = 18;              // entry = leaf-or-node index (< 2^18) | length << 18 | kLutCont
constexpr size_t kEncLdsBytes = 64 * 1024;    // encoder codeword table in LDS up to 8192 symbols, read from global beyond

struct HuffCodebook {
    uint32_t magic = 0x48554646u;
    int32_t n = 0;
    int32_t max_len = 0;
    int32_t lut_bits = 0;
    int device = 0;
    uint2* d_enc[2] = {nullptr, nullptr};    // per symbol {codeword, length}, [0] suffix order (stack), [1] prefix order (queue);
                                             // a codeword of more than 32 bits holds the offset of its bits in d_pool[...]
    uint32_t* d_pool[2] = {nullptr, nullptr};
    uint32_t* d_lut = nullptr;               // [2^lut_bits]
    uint32_t* d_child = nullptr;             // [2 * (n - 1)] children of the inner nodes n .. 2n-2, bit 0 then bit 1
};

inline bool valid_cb(const void* cb) { return cb && static_cast<const HuffCodebook*>(cb)->magic == 0x48554646u; }

template <int SB>
__device__ inline uint32_t load_sym(const void* base, size_t i) {
    if constexpr (SB == 1) return static_cast<const uint8_t*>(base)[i];
    else return (uint32_t)static_cast<const int32_t*>(base)[i];    // negative -> >= n: impossible
}

template <int SB>
__device__ inline void store_sym(void* base, size_t i, uint32_t v) {
    if constexpr (SB == 1) static_cast<uint8_t*>(base)[i] = (uint8_t)v;
    else static_cast<int32_t*>(base)[i] = (int32_t)v;
}

// wave-private LDS tiles: 64 stream rows x kTile symbols.  The encoder stages its symbols through one, the decoders their
// decoded symbols.
constexpr int kTile = 32;

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A lane's compressed words on their way to its slab: collected four at a time and written as one 16-byte store when the slab
// is 16-byte aligned (VEC: stride_words % 4 == 0 and an aligned base -- what cst_huffman_max_words gives), else one by one.
struct WordSink {
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

// appends `len` (<= 32) bits; emits a word once 32 are pending.  false: the slab is full
__device__ __forceinline__ bool put_bits(uint32_t code, uint32_t len, uint64_t& acc, uint32_t& nb, WordSink& sink) {
    acc |= (uint64_t)code << nb;
    nb += len;
    if (nb >= 32) {
        if (!sink.put((uint32_t)acc)) return false;
        acc >>= 32;
        nb -= 32;
    }
    return true;
}

template <bool LONG>
__device__ __forceinline__ bool put_symbol(uint2 e, const uint32_t* pool, uint64_t& acc, uint32_t& nb, WordSink& sink) {
    if (!LONG || e.y <= 32) return put_bits(e.x, e.y, acc, nb, sink);
    // out of line: a codeword of more than 32 bits, in emission order in the pool, 32 bits at a time
    const uint32_t* p = pool + e.x;
    for (uint32_t left = e.y; left > 0;) {
        const uint32_t k = left < 32 ? left : 32;
        if (!put_bits(*p++, k, acc, nb, sink)) return false;
        left -= k;
    }
    return true;
}

template <typename K, typename A>
cst_status launch_huff(K kernel, size_t n_lanes, size_t lds_bytes, hipStream_t hs, const A& args) {
    const size_t blocks = (n_lanes + kBlock - 1) / kBlock;
    if (blocks == 0) return CST_OK;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (lds_bytes > 64 * 1024) {
        CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds_bytes));
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), lds_bytes, hs, args);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

inline bool on_device(const HuffCodebook* c) {
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev == c->device;
}

} // namespace

} // namespace cst
