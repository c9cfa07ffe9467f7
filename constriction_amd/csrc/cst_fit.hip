// cst_fit.hip -- fitting table models on the device: histograms of int32 symbols (one for the whole array, one
// per index class, one per stream) and the way from counts to cdf rows through the Categorical quantisers that exist already
// (cst_categorical_fast_cdf_rows / cst_categorical_perfect_cdf_rows and their host forms).
#include <vector>

#include "cst_common.hpp"

namespace cst {

typedef int32_t v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t kFitLdsBins = 16384;      // 64 KiB of uint32 bins (replicas included) per workgroup: two workgroups per CU
constexpr uint32_t kFitMaxReplicas = 8;
constexpr uint32_t kFitUnit = 4096;          // per-stream counts: symbols of one unit of work (one wave, 16 loads of 16 bytes per lane)
constexpr int kFitPsMaxSymbols = 1024;       // a wave-private LDS row of 4 KiB

// orders a wave's LDS accesses: what its lanes added to the row is what they read afterwards
__device__ __forceinline__ void fit_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what the lanes of a (whole, converged) wave counted outside the support: summed across the wave, one atomic per wave
__device__ __forceinline__ void fit_add_outside(uint32_t* outside, uint32_t n) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(outside, n);
}

struct FitCountArgs {
    const int32_t* symbols;
    const void* indices;          // nullptr: one table
    uint32_t n_total;
    int32_t min_symbol;
    uint32_t n_symbols, n_tables;
    uint32_t rep_shift;           // LDS path: log2(replicas of every bin)
    uint32_t wave_uniform;        // LDS path: a wave whose 64 symbols fall into one bin adds them with one atomic
    uint32_t* counts;
    uint32_t* outside;
};

// bin of (symbol, index), or 0xffffffff for a symbol outside the support or an index outside [0, n_tables)
template <int IB>
__device__ __forceinline__ uint32_t fit_bin(const FitCountArgs& a, int32_t sym, uint32_t i) {
    const uint32_t b = (uint32_t)sym - (uint32_t)a.min_symbol;
    uint32_t k = 0;
    if (IB == 1) k = reinterpret_cast<const uint8_t*>(a.indices)[i];
    if (IB == 4) k = (uint32_t)reinterpret_cast<const int32_t*>(a.indices)[i];
    return (b < a.n_symbols && k < a.n_tables) ? k * a.n_symbols + b : 0xffffffffu;
}

// One histogram of the flat array, or one per index class.  LDS = true: every workgroup counts into its own copy of the bins
// (2^rep_shift replicas of each, side by side and picked by lane id, so that the lanes of a wave that meet in one bin spread over
// several addresses) and adds the bins it touched to the zeroed result.  LDS = false: global atomics, for supports beyond LDS.
// IB = bytes of an index (0: none).
template <bool LDS, int IB>
__global__ __launch_bounds__(kBlock) void fit_count_kernel(const FitCountArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fit_bins[];
    const uint32_t n_bins = a.n_symbols * a.n_tables;
    const uint32_t lane_rep = threadIdx.x & ((1u << a.rep_shift) - 1u);
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < (n_bins << a.rep_shift); i += kBlock) fit_bins[i] = 0u;
        __syncthreads();
    }
    uint32_t n_outside = 0;
    auto count = [&](uint32_t bin) {
        if (bin == 0xffffffffu) { ++n_outside; return; }
        if (LDS) atomicAdd(&fit_bins[(bin << a.rep_shift) + lane_rep], 1u);
        else atomicAdd(&a.counts[bin], 1u);
    };
    // four bins of one 16-byte load; a wave that is whole and of one mind (constant data: 64 lanes on one LDS address) adds once
    auto count4 = [&](uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
        if (LDS && a.wave_uniform) {
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
            const bool same = b0 == first && b1 == first && b2 == first && b3 == first;
            if (first != 0xffffffffu && __all(same) && __popcll(__ballot(1)) == kWave) {
                if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&fit_bins[first << a.rep_shift], 4u * kWave);
                return;
            }
        }
        count(b0); count(b1); count(b2); count(b3);
    };

    // [0, head): up to the first 16-byte boundary of the symbol array; [head, head + 4 * n_vec): whole 16-byte loads; the rest
    const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(a.symbols) >> 2) & 3u);
    uint32_t head = (4u - mis) & 3u;
    if (head > a.n_total) head = a.n_total;
    const uint32_t n_vec = (a.n_total - head) / 4u;
    const uint32_t tail0 = head + 4u * n_vec;
    const uint32_t gid = blockIdx.x * kBlock + threadIdx.x, n_threads = gridDim.x * kBlock;
    if (gid < head) count(fit_bin<IB>(a, a.symbols[gid], gid));
    if (gid < a.n_total - tail0) count(fit_bin<IB>(a, a.symbols[tail0 + gid], tail0 + gid));
    const v4i* vec = reinterpret_cast<const v4i*>(a.symbols + head);
    for (uint32_t j = gid; j < n_vec; j += n_threads) {
        const v4i v = __builtin_nontemporal_load(vec + j);
        const uint32_t i = head + 4u * j;
        count4(fit_bin<IB>(a, v.x, i), fit_bin<IB>(a, v.y, i + 1u), fit_bin<IB>(a, v.z, i + 2u), fit_bin<IB>(a, v.w, i + 3u));
    }
    fit_add_outside(a.outside, n_outside);
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock) {
            uint32_t v = 0;
            for (uint32_t r = 0; r < (1u << a.rep_shift); ++r) v += fit_bins[(i << a.rep_shift) + r];
            if (v) atomicAdd(&a.counts[i], v);
        }
    }
}

struct FitPsArgs {
    const int32_t* symbols;
    const uint64_t* offsets;      // nullptr: stream s is [s * n_per, (s + 1) * n_per)
    uint64_t base;                // flat position of the first symbol (offsets[0]; 0 without offsets)
    uint32_t n_total;             // symbols from `base` on
    uint32_t n_streams, n_per;
    int32_t min_symbol;
    uint32_t n_symbols;
    uint32_t* counts;
    uint32_t* outside;
};

__device__ __forceinline__ uint64_t fit_ps_begin(const FitPsArgs& a, uint32_t s) {
    return a.offsets ? a.offsets[s] : (uint64_t)s * a.n_per;
}

// One histogram per stream.  The flat array is cut into units of kFitUnit symbols and a wave owns a unit and a private LDS row:
// it walks the streams that meet its unit, counts each one's part into the row and hands the row over -- by plain stores where the
// part is the whole stream (the row is final), by atomic adds of the bins it touched where a long stream spreads over several
// units.  Nothing but the unit bounds what a wave reads: offsets that do not ascend give wrong counts, never a read outside
// [base, base + n_total).
__global__ __launch_bounds__(kBlock) void fit_count_ps_kernel(const FitPsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fit_rows[];
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint32_t* row = fit_rows + (threadIdx.x >> 6) * a.n_symbols;
    const uint32_t unit = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const uint64_t u0 = a.base + (uint64_t)unit * kFitUnit;
    const uint64_t end = a.base + a.n_total;
    if (u0 >= end) return;
    const uint64_t u1 = u0 + kFitUnit < end ? u0 + kFitUnit : end;
    // the stream that holds position u0: the last one that begins at or before it
    uint32_t s;
    if (a.offsets) {
        uint32_t lo = 0, hi = a.n_streams;          // first stream that begins behind u0
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.offsets[mid] <= u0) lo = mid + 1; else hi = mid;
        }
        s = lo > 0 ? lo - 1 : 0;
    } else {
        s = (uint32_t)(u0 / a.n_per);
    }
    uint32_t n_outside = 0;
    auto count = [&](int32_t sym) {
        const uint32_t b = (uint32_t)sym - (uint32_t)a.min_symbol;
        if (b < a.n_symbols) atomicAdd(&row[b], 1u); else ++n_outside;
    };
    uint64_t pos = u0;
    for (; pos < u1 && s < a.n_streams; ++s) {
        const uint64_t s_begin = fit_ps_begin(a, s);
        const uint64_t s_end = fit_ps_begin(a, s + 1);
        const uint64_t e = s_end < u1 ? s_end : u1;
        if (e <= pos) continue;                     // an empty stream: its row stays zero
        for (uint32_t i = lane; i < a.n_symbols; i += kWave) row[i] = 0u;
        fit_wave_fence();
        const int32_t* p = a.symbols + pos;
        const uint32_t len = (uint32_t)(e - pos);
        const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u);
        uint32_t head = (4u - mis) & 3u;
        if (head > len) head = len;
        const uint32_t n_vec = (len - head) / 4u, tail0 = head + 4u * n_vec;
        if (lane < head) count(p[lane]);
        if (lane < len - tail0) count(p[tail0 + lane]);
        const v4i* vec = reinterpret_cast<const v4i*>(p + head);
        for (uint32_t j = lane; j < n_vec; j += kWave) {
            const v4i v = __builtin_nontemporal_load(vec + j);
            count(v.x); count(v.y); count(v.z); count(v.w);
        }
        fit_wave_fence();
        uint32_t* out = a.counts + (size_t)s * a.n_symbols;
        const bool whole = pos == s_begin && e == s_end;
        for (uint32_t i = lane; i < a.n_symbols; i += kWave) {
            const uint32_t v = row[i];
            if (whole) out[i] = v;
            else if (v) atomicAdd(&out[i], v);
        }
        fit_wave_fence();
        pos = e;
    }
    fit_add_outside(a.outside, n_outside);
}

// counts -> the f64 weights the quantisers take; a row without a count becomes a row of ones (empty[r] = 1).  One workgroup per row.
__global__ __launch_bounds__(kBlock) void fit_weights_kernel(const uint32_t* __restrict__ counts, uint32_t n_symbols, double* __restrict__ weights,
                                                              int32_t* __restrict__ empty) {
    const uint32_t* c = counts + (size_t)blockIdx.x * n_symbols;
    double* w = weights + (size_t)blockIdx.x * n_symbols;
    int any = 0;
    for (uint32_t i = threadIdx.x; i < n_symbols; i += kBlock) any |= c[i] != 0u;
    any = __syncthreads_or(any);
    for (uint32_t i = threadIdx.x; i < n_symbols; i += kBlock) w[i] = any ? (double)c[i] : 1.0;
    if (empty && threadIdx.x == 0) empty[blockIdx.x] = any ? 0 : 1;
}

static int cu_count_now() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 64;
    return cus;
}

template <bool LDS>
static void launch_fit_count(const FitCountArgs& a, int32_t index_bytes, unsigned blocks, size_t lds, hipStream_t hs) {
    if (!a.indices) hipLaunchKernelGGL((fit_count_kernel<LDS, 0>), dim3(blocks), dim3(kBlock), lds, hs, a);
    else if (index_bytes == 1) hipLaunchKernelGGL((fit_count_kernel<LDS, 1>), dim3(blocks), dim3(kBlock), lds, hs, a);
    else hipLaunchKernelGGL((fit_count_kernel<LDS, 4>), dim3(blocks), dim3(kBlock), lds, hs, a);
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_count_symbols(const int32_t* d_symbols, size_t n_total, int32_t min_symbol, int32_t n_symbols, const void* d_indices,
                             int32_t index_bytes, int32_t n_tables, uint32_t* d_counts, uint32_t* d_outside, void* stream) {
    if (!d_counts || !d_outside || (n_total > 0 && !d_symbols)) return CST_ERR_INVALID_ARGUMENT;
    if (n_tables < 1 || n_tables > 256 || n_symbols < 2 || n_symbols > 65536 || n_total >= ((size_t)1 << 31)) return CST_ERR_INVALID_ARGUMENT;
    if (d_indices ? (index_bytes != 1 && index_bytes != 4) : n_tables != 1) return CST_ERR_INVALID_ARGUMENT;
    if ((int64_t)min_symbol + n_symbols - 1 > INT32_MAX) return CST_ERR_INVALID_ARGUMENT;
    hipStream_t hs = (hipStream_t)stream;
    const size_t n_bins = (size_t)n_tables * (size_t)n_symbols;
    CST_HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * n_bins, hs));
    CST_HIP_TRY(hipMemsetAsync(d_outside, 0, 4, hs));
    if (n_total == 0) return CST_OK;
    FitCountArgs a{};
    a.symbols = d_symbols; a.indices = d_indices; a.n_total = (uint32_t)n_total; a.min_symbol = min_symbol;
    a.n_symbols = (uint32_t)n_symbols; a.n_tables = (uint32_t)n_tables; a.counts = d_counts; a.outside = d_outside;
    const bool lds = n_bins <= kFitLdsBins;
    // (CST_FIT_REPLICAS and CST_FIT_WAVE_UNIFORM, scripts/bench_fit.py: the same counts either way)
    uint32_t reps = 1;
    if (lds) {
        const uint32_t want = (uint32_t)knobs().fit_replicas;
        while (reps * 2 <= kFitMaxReplicas && reps * 2 <= want && n_bins * reps * 2 <= kFitLdsBins) reps *= 2;
    }
    while ((1u << a.rep_shift) < reps) ++a.rep_shift;
    a.wave_uniform = knobs().fit_wave_uniform ? 1u : 0u;
    const size_t lds_bytes = lds ? 4 * n_bins * reps : 0;
    // workgroups: what the CUs hold at once (LDS and 8 waves per SIMD bound it), no more than there are 16-byte loads to share
    size_t per_cu = 8;
    if (lds && (size_t)(160 * 1024) / lds_bytes < per_cu) per_cu = (size_t)(160 * 1024) / lds_bytes;
    size_t blocks = (size_t)cu_count_now() * per_cu;
    const size_t by_work = (n_total / 4 + kBlock - 1) / kBlock;
    if (blocks > by_work) blocks = by_work;
    if (blocks < 1) blocks = 1;
    if (lds) launch_fit_count<true>(a, index_bytes, (unsigned)blocks, lds_bytes, hs);
    else launch_fit_count<false>(a, index_bytes, (unsigned)blocks, 0, hs);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel(lds ? "fit_count_kernel<lds>" : "fit_count_kernel<global>", CST_OK);
}

cst_status cst_count_symbols_per_stream(const int32_t* d_symbols, const uint64_t* d_sym_offsets, size_t n_streams, size_t n_per_stream,
                                        int32_t min_symbol, int32_t n_symbols, uint32_t* d_counts, uint32_t* d_outside, void* stream) {
    if (!d_counts || !d_outside || n_streams == 0 || n_streams >= ((size_t)1 << 31)) return CST_ERR_INVALID_ARGUMENT;
    if (n_symbols < 2 || n_symbols > kFitPsMaxSymbols || (int64_t)min_symbol + n_symbols - 1 > INT32_MAX) return CST_ERR_INVALID_ARGUMENT;
    if (!d_sym_offsets) {
        if (n_per_stream >= ((size_t)1 << 31) || n_streams * n_per_stream >= ((size_t)1 << 31)) return CST_ERR_INVALID_ARGUMENT;
        if (n_per_stream > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    }
    hipStream_t hs = (hipStream_t)stream;
    CST_HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * n_streams * (size_t)n_symbols, hs));
    CST_HIP_TRY(hipMemsetAsync(d_outside, 0, 4, hs));
    FitPsArgs a{};
    a.symbols = d_symbols; a.offsets = d_sym_offsets; a.n_streams = (uint32_t)n_streams; a.n_per = (uint32_t)n_per_stream;
    a.min_symbol = min_symbol; a.n_symbols = (uint32_t)n_symbols; a.counts = d_counts; a.outside = d_outside;
    uint64_t total = n_streams * n_per_stream;
    if (d_sym_offsets) {      // the flat range [offsets[0], offsets[n_streams]) sizes the grid
        uint64_t ends[2] = {0, 0};
        CST_HIP_TRY(hipMemcpyAsync(&ends[0], d_sym_offsets, 8, hipMemcpyDeviceToHost, hs));
        CST_HIP_TRY(hipMemcpyAsync(&ends[1], d_sym_offsets + n_streams, 8, hipMemcpyDeviceToHost, hs));
        CST_HIP_TRY(hipStreamSynchronize(hs));
        if (ends[1] < ends[0] || ends[1] - ends[0] >= ((uint64_t)1 << 31)) return CST_ERR_INVALID_ARGUMENT;
        a.base = ends[0];
        total = ends[1] - ends[0];
        if (total > 0 && !d_symbols) return CST_ERR_INVALID_ARGUMENT;
    }
    if (total == 0) return CST_OK;
    a.n_total = (uint32_t)total;
    const size_t units = (total + kFitUnit - 1) / kFitUnit, waves = kBlock / kWave;
    hipLaunchKernelGGL(fit_count_ps_kernel, dim3((unsigned)((units + waves - 1) / waves)), dim3(kBlock), 4 * waves * (size_t)n_symbols, hs, a);
    CST_HIP_TRY(hipGetLastError());
    return note_kernel("fit_count_ps_kernel", CST_OK);
}

static cst_status check_fit_rows_args(int32_t precision, int32_t perfect, const void* counts, int32_t n_symbols, const void* rows) {
    if (!counts || !rows || precision < 1 || precision > 31) return CST_ERR_INVALID_ARGUMENT;
    if (n_symbols < 2) return CST_ERR_MODEL;
    if (perfect ? (n_symbols > CST_CATEGORICAL_PERFECT_MAX_K || (uint64_t)n_symbols > ((uint64_t)1 << precision))
                : (uint64_t)n_symbols >= ((uint64_t)1 << precision) - 1) return CST_ERR_MODEL;      // (the quantisers' own limits)
    return CST_OK;
}

cst_status cst_fit_cdf_rows(int32_t precision, int32_t perfect, const uint32_t* d_counts, size_t n_rows, int32_t n_symbols, uint32_t* d_rows,
                            int32_t* d_empty, void* stream) {
    if (cst_status st = check_fit_rows_args(precision, perfect, d_counts, n_symbols, d_rows)) return st;
    if (n_rows >= ((size_t)1 << 31)) return CST_ERR_INVALID_ARGUMENT;
    if (n_rows == 0) return CST_OK;
    hipStream_t hs = (hipStream_t)stream;
    double* d_weights = nullptr;
    CST_HIP_TRY(hipMallocAsync((void**)&d_weights, 8 * n_rows * (size_t)n_symbols, hs));
    hipLaunchKernelGGL(fit_weights_kernel, dim3((unsigned)n_rows), dim3(kBlock), 0, hs, d_counts, (uint32_t)n_symbols, d_weights, d_empty);
    cst_status st = hipGetLastError() == hipSuccess ? CST_OK : CST_ERR_HIP;
    if (st == CST_OK)
        st = perfect ? cst_categorical_perfect_cdf_rows(precision, d_weights, 8, n_rows, n_symbols, d_rows, nullptr, nullptr, stream)
                     : cst_categorical_fast_cdf_rows(precision, d_weights, 8, n_rows, n_symbols, d_rows, nullptr, stream);
    (void)hipFreeAsync(d_weights, hs);
    return st;
}

cst_status cst_fit_cdf_rows_host(int32_t precision, int32_t perfect, const uint32_t* h_counts, size_t n_rows, int32_t n_symbols, uint32_t* h_rows,
                                 int32_t* h_empty) {
    if (cst_status st = check_fit_rows_args(precision, perfect, h_counts, n_symbols, h_rows)) return st;
    const size_t K = (size_t)n_symbols;
    std::vector<double> w(K);
    for (size_t r = 0; r < n_rows; ++r) {
        bool any = false;
        for (size_t i = 0; i < K; ++i) any |= h_counts[r * K + i] != 0u;
        for (size_t i = 0; i < K; ++i) w[i] = any ? (double)h_counts[r * K + i] : 1.0;
        if (h_empty) h_empty[r] = any ? 0 : 1;
        const cst_status st = perfect ? cst_categorical_perfect_cdf_host(precision, w.data(), 8, 1, n_symbols, h_rows + r * (K + 1), nullptr, nullptr)
                                      : cst_categorical_fast_cdf_host(precision, w.data(), 8, 1, n_symbols, h_rows + r * (K + 1), nullptr);
        if (st != CST_OK) return st;
    }
    return CST_OK;
}

} // extern "C"
