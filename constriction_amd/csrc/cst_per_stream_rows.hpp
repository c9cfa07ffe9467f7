// cst_per_stream_rows.hpp -- one cdf row per stream, held in LDS for a whole kernel: what the per-stream ANS coder
// (cst_ans_ps.hip), the per-stream range coder (cst_range_ps.hip) and their ragged forms (cst_ragged_ps.hip) share.
//
// Each lane's cumulative table (n+1 entries of 16 bits, row length L = 2^k) is TRANSPOSED per wave: entry e of lane l
// lives at [e][l] (like the word rings).  The bank of an access then depends on the lane only, whatever index the lane
// probes: two lanes per bank instead of the ~6-way conflicts random per-lane indices cause in a row-per-lane layout
// (PMC: 200 of 1100 cycles per decoded symbol were bank conflicts).  A coder needs (c, p) = (row[i], row[i+1] - row[i]);
// a decoder finds the largest i with row[i] <= q by a 4-ary search (3 probes per round, ceil(log4 n) rounds, branch free),
// started from a 64-bucket index of the row where 6 <= P <= 15.
#pragma once
#include "cst_ans_kernels.hpp"

namespace cst {

// this lane's column of its wave's transposed table: entry i at base[i * kWave]
struct LaneRow {
    const uint16_t* base;  // &table_of_wave[0][lane]
    __device__ __forceinline__ uint32_t at(uint32_t i) const { return base[i * kWave]; }
};

// `a`: the kernel's argument struct (cdf16 [n_tables][L], L, n_symbols, n_streams = lanes with a stream).
// `pad`: entries behind cdf[n] become 0xFFFF, a sentinel above every quantile when P <= 15 (the decoder's search
// then needs no bounds checks).  `lanes_per_table`: lane j of the block stages row (block_s0 + j) / lanes_per_table
// (a stream decoded by several lanes, one per chunk: every such lane holds its own copy of the stream's row).
template <class Args>
__device__ __forceinline__ void stage_rows(uint16_t* lds_rows, const Args& a, size_t block_s0, bool pad = false, size_t lanes_per_table = 1) {
    const uint32_t L = (uint32_t)a.L, mask = L - 1;
    const uint32_t total = blockDim.x * L;
    const int shift = __builtin_ctz(L);
    for (uint32_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const uint32_t j = idx >> shift, e = idx & mask;
        const size_t s = block_s0 + j;
        const size_t row = lanes_per_table == 1 ? s : s / lanes_per_table;
        uint16_t v = s < a.n_streams ? a.cdf16[row * L + e] : (uint16_t)0;
        if (pad && e > (uint32_t)a.n_symbols) v = 0xFFFFu;
        lds_rows[((size_t)(j >> 6) * L + e) * kWave + (j & 63u)] = v;      // [wave][entry][lane]
    }
}

// The same staging where a lane's row is not a function of its number (ragged batches, cst_ragged_ps.hip: the stream a
// schedule gives the lane, or the stream that owns the lane's chunk): `lane_row` [blockDim.x] in LDS, written by the lanes
// themselves (a barrier between that and this call); kPsNoRow = a lane without a stream, whose row is staged as zeros.
constexpr uint32_t kPsNoRow = 0xffffffffu;
template <class Args>
__device__ __forceinline__ void stage_rows_by_index(uint16_t* lds_rows, const Args& a, const uint32_t* lane_row, bool pad = false) {
    const uint32_t L = (uint32_t)a.L, mask = L - 1;
    const uint32_t total = blockDim.x * L;
    const int shift = __builtin_ctz(L);
    for (uint32_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const uint32_t j = idx >> shift, e = idx & mask;
        const uint32_t row = lane_row[j];
        uint16_t v = row != kPsNoRow ? a.cdf16[(size_t)row * L + e] : (uint16_t)0;
        if (pad && e > (uint32_t)a.n_symbols) v = 0xFFFFu;
        lds_rows[((size_t)(j >> 6) * L + e) * kWave + (j & 63u)] = v;      // [wave][entry][lane]
    }
}

// Bucket index of the per-stream decoders: kPsBuckets + 1 entries per stream, start[b] = the symbol index whose bin
// holds quantile b * 2^(P - log2 kPsBuckets); kPsIdxStride entries per lane, stored [bucket][lane] like the tables.
constexpr int kPsBucketBits = 6, kPsBuckets = 1 << kPsBucketBits, kPsIdxStride = 66;

// P in [6, 15]: bucket index + sentinel-padded rows (see stage_rows); otherwise the plain bounded 4-ary search
__host__ __device__ inline bool ps_indexed(int P) { return P >= kPsBucketBits && P <= 15; }

// this lane's own row -> its bucket index (one pass over the row); `bidx` = &index_of_wave[0][lane]
__device__ __forceinline__ void ps_build_bucket_index(const LaneRow& R, uint16_t* bidx, int P, uint32_t n) {
    uint32_t i = 0;
    const uint32_t w = 1u << (P - kPsBucketBits);
    for (uint32_t b = 0; b < (uint32_t)kPsBuckets; ++b) {
        const uint32_t q0 = b * w;
        while (i + 1 < n && R.at(i + 1) <= q0) ++i;
        bidx[b * kWave] = (uint16_t)i;
    }
    bidx[kPsBuckets * kWave] = (uint16_t)(n - 1);
    wave_lds_fence();
}

// the largest i in [0, n) with row[i] <= q.  Every lane of the wave must call it (wave-uniform trip counts).
__device__ __forceinline__ uint32_t ps_search(const LaneRow& R, const uint16_t* bidx, bool indexed, uint32_t q, int P, uint32_t n) {
    uint32_t lo;
    if (indexed) {
        // the answer lies in [start[b], start[b+1]]; everything behind start[b+1] (including the padding) is > q,
        // so the 4-ary refinement needs no bounds checks and a lane that is done is not disturbed by extra rounds
        const uint32_t b = q >> (P - kPsBucketBits);
        lo = bidx[b * kWave];
        uint32_t size = (uint32_t)bidx[(b + 1) * kWave] - lo + 1u;
        while (__any(size > 1)) {
            const uint32_t step = (size + 3) >> 2;
            // (probes clamped to index n, whose entry 2^P is itself above every quantile: the row may be exactly
            // n + 1 entries long, and an index behind it would wrap around to the row's small first entries)
            const uint32_t v1 = R.at(min(lo + step, n)), v2 = R.at(min(lo + 2 * step, n)), v3 = R.at(min(lo + 3 * step, n));
            lo += ((v1 <= q ? 1u : 0u) + (v2 <= q ? 1u : 0u) + (v3 <= q ? 1u : 0u)) * step;
            size = step;
        }
    } else {
        // 4-ary search over [0, n), wave-uniform trip count
        lo = 0;
        uint32_t size = n;
        while (size > 1) {
            const uint32_t step = (size + 3) >> 2;
            const uint32_t p1 = lo + step, p2 = p1 + step, p3 = p2 + step;
            const uint32_t v1 = p1 < n ? R.at(p1) : 0x10000u, v2 = p2 < n ? R.at(p2) : 0x10000u, v3 = p3 < n ? R.at(p3) : 0x10000u;
            lo += ((v1 <= q ? 1u : 0u) + (v2 <= q ? 1u : 0u) + (v3 <= q ? 1u : 0u)) * step;
            size = step;
        }
    }
    return lo;
}

// threads per block such that rows + rings + (symbol tiles | bucket index) fit in the 160 KiB of LDS of one CU
static int pick_block(int L, bool with_tiles, size_t& lds) {
    for (int threads = 256; threads >= 64; threads -= 64) {
        lds = (size_t)threads * L * 2 + (size_t)(threads / kWave) * (kRingWords + (with_tiles ? kWave * kTileStride : 0)) * sizeof(uint32_t) +
              (with_tiles ? 0 : (size_t)threads * kPsIdxStride * 2);   // encoder: symbol tiles; decoder: bucket index
        if (lds <= 160 * 1024) return threads;
    }
    return 0;
}

template <typename K, typename A>
static cst_status launch_ps(K kernel, const A& a, bool with_tiles, hipStream_t hs) {
    size_t lds = 0;
    const int threads = pick_block(a.L, with_tiles, lds);
    if (threads == 0) return CST_ERR_INVALID_ARGUMENT;   // support too large for LDS-resident per-stream tables
    const size_t blocks = (a.n_streams + threads - 1) / threads;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (lds > 64 * 1024)
        CST_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, hs, a);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

} // namespace cst
