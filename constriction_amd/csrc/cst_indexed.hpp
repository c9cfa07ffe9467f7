// cst_indexed.hpp -- what the two translation units of indexed table coding share: the table-set handle, the
// LDS image's readers and the handle checks.
//   cst_indexed.hip          the table set itself and the rectangular coders (one length for every stream)
//   cst_indexed_ragged.hip   streams of different lengths, plain and with jump points
// Every kernel instantiation lives in ONE of the two files; nothing here is a kernel.
#pragma once
#include <type_traits>

#include "cst_persymbol.hpp"

// What the opaque table-set handle of the C ABI (a void *) points to.
struct cst_table_set {
    uint32_t magic = 0;          // kIxMagic while the handle lives
    int32_t precision = 0, min_symbol = 0, n_symbols = 0, n_tables = 0;
    int device = 0;
    int32_t pitch = 0;           // entries per row: n_symbols + 1
    int32_t wide = 0;            // 32-bit row entries (P > 16)
    int32_t bucket_bits = 0;     // b: 2^b + 1 bucket entries per table
    int32_t bucket_wide = 0;     // 16-bit bucket entries (n_symbols > 256), else 8-bit
    uint32_t rows_bytes = 0;     // multiples of 16; the buckets follow the rows
    uint32_t image_bytes = 0;
    unsigned char* d_image = nullptr;
};

namespace cst {

constexpr uint32_t kIxMagic = 0x58495443u;
constexpr int kIxRingSlots = 32;                              // words per lane: at most 13 emitted + 6 pending between two points
constexpr int kIxAhead = 24;                                  // decode: words kept requested beyond the read position
constexpr size_t kIxRingBytes = (size_t)(kBlock / kWave) * kIxRingSlots * kWave * 4;
constexpr size_t kIxTileBytes = (size_t)(kBlock / kWave) * kWave * kTileStride * 4;
constexpr size_t kIxFixedLds = kIxRingBytes + kIxTileBytes;   // 32 KiB + 36 KiB
constexpr size_t kIxMaxImage = 90 * 1024;                     // what fits beside them in a CU's 160 KiB (include/constriction_amd.h)
constexpr int kIxMaxBucketBits = 8;

template <bool WIDE>
__device__ __forceinline__ uint32_t row_at(const unsigned char* rows, uint32_t e) {
    if constexpr (WIDE) return reinterpret_cast<const uint32_t*>(rows)[e];
    else return reinterpret_cast<const uint16_t*>(rows)[e];
}

// the workgroup's copy of the first `bytes` (a multiple of 16) of the image
__device__ __forceinline__ void stage_image(unsigned char* lds, const unsigned char* image, uint32_t bytes) {
    const uint4* src = reinterpret_cast<const uint4*>(image);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (uint32_t i = threadIdx.x; i < bytes / 16; i += blockDim.x) dst[i] = src[i];
}

// (symbol, index) of one position as the encoder's tile holds it: the table in the high half, the symbol's place in the support in
// the low one, both clamped to ONE past their last legal value -- which marks the impossible symbol, and no more
__device__ __forceinline__ uint32_t pack_position(int32_t sym, int32_t idx, int32_t min_symbol, uint32_t nsym, uint32_t K) {
    return (min((uint32_t)idx, K) << 16) | min((uint32_t)sym - (uint32_t)min_symbol, nsym);
}

// quantile -> (index, left cumulative, probability) inside row k: bucket[q >> shift] holds the bucket's first quantile and its
// successor the first quantile of the next bucket, so the symbol lies between the two; most buckets begin and end in one symbol
template <bool WIDE>
__device__ __forceinline__ void indexed_lookup(const unsigned char* rows, const unsigned char* buckets, bool bucket_wide, uint32_t bstride,
                                               uint32_t pitch, uint32_t k, uint32_t q, int shift, uint32_t pmask, uint32_t& idx, uint32_t& c,
                                               uint32_t& p) {
    const uint32_t b = k * bstride + (q >> shift);
    uint32_t lo, hi;
    if (bucket_wide) { lo = reinterpret_cast<const uint16_t*>(buckets)[b]; hi = reinterpret_cast<const uint16_t*>(buckets)[b + 1u]; }
    else { lo = buckets[b]; hi = buckets[b + 1u]; }
    const uint32_t base = k * pitch;
    for (int guard = 0; guard < 17 && __any(lo < hi); ++guard) {          // (c[lo] <= q < c[hi + 1] throughout; 2^16 symbols at most)
        const uint32_t mid = (lo + hi + 1u) >> 1;
        const bool up = row_at<WIDE>(rows, base + mid) <= q;
        if (lo < hi) { lo = up ? mid : lo; hi = up ? hi : mid - 1u; }
    }
    c = row_at<WIDE>(rows, base + lo);
    p = (row_at<WIDE>(rows, base + lo + 1u) - c) & pmask;
    idx = lo;
}

// ---- host side ----
static inline const cst_table_set* as_table_set(const void* p) { return reinterpret_cast<const cst_table_set*>(p); }
static inline bool table_set_alive(const cst_table_set* t) { return t && t->magic == kIxMagic; }

} // namespace cst
