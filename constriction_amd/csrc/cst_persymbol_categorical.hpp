// cst_persymbol_categorical.hpp -- what the two units of the per-symbol Categorical coders share (cst_persymbol.hpp has the map of the
// per-symbol files): the geometry of the wave-private row tile, its staging loop, and pass 1 of the encoders.
// categorical_entries_kernel<F> is launched from both units -- cst_persymbol_categorical.hip over a matrix of the symbols' shape,
// cst_persymbol_categorical_ragged.hip over the flat rows of a ragged batch -- and is the one kernel that both instantiate: a template,
// so the copies fold at link time on the host side, and each unit's code object carries its own (two small kernels).
#pragma once
#include "cst_persymbol.hpp"
#include "cst_categorical.hpp"

namespace cst {

constexpr int kCatChunk = 64;                          // C: columns of a row staged at a time
constexpr int kCatPitch = kCatChunk + 1;               // elements from one row of the tile to the next: odd, so that the 64 lanes
                                                       // reading one column of 64 rows hit different banks (f32 and f64)
template <class F> constexpr size_t kCatTileBytes = (size_t)kWave * kCatPitch * sizeof(F);      // 16 640 B (f32) / 33 280 B (f64)

template <class F> struct CatVec;
template <> struct CatVec<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int n = 4; };
template <> struct CatVec<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int n = 2; };

// 16-byte loads need rows that start on 16 bytes
template <class F>
__device__ __forceinline__ bool cat_vec_ok(const F* probs, size_t K) {
    return (K * sizeof(F)) % 16 == 0 && (reinterpret_cast<uintptr_t>(probs) & 15) == 0;
}

// Columns [c0, c0 + n_here) of the wave's rows -> tile[r * kCatPitch + j].  Row r of the wave (r < n_rows) is row
// first + r * step of the matrix [rows][K].  `vec`: 16 bytes per lane (n_here is then a multiple of the vector), 4 (f32) or 2
// (f64) rows per load instruction; else one element per lane, one row per instruction.  The loads are unconditional, from an
// address that is always valid (a conditional load is waited for at once); what lies outside the tile is not stored.
template <class F>
__device__ __forceinline__ void cat_stage(F* tile, const F* __restrict__ probs, size_t first, size_t step, int n_rows, size_t K, size_t c0,
                                          int n_here, bool vec, int lane) {
    if (vec) {
        using V = typename CatVec<F>::type;
        constexpr int kV = CatVec<F>::n, kLanesPerRow = kCatChunk / kV, kRowsPerLoad = kWave / kLanesPerRow;
        const int col = (lane % kLanesPerRow) * kV, r0 = lane / kLanesPerRow;
        const bool col_ok = col < n_here;
        const F* src = probs + c0 + (size_t)(col_ok ? col : 0);
#pragma unroll 8
        for (int it = 0; it < kWave / kRowsPerLoad; ++it) {
            const int r = it * kRowsPerLoad + r0;
            const bool ok = r < n_rows && col_ok;
            const V v = *reinterpret_cast<const V*>(src + (first + (size_t)(r < n_rows ? r : 0) * step) * K);
            if (ok) {
#pragma unroll
                for (int k = 0; k < kV; ++k) tile[r * kCatPitch + col + k] = v[k];
            }
        }
    } else {
        const bool col_ok = lane < n_here;
        const F* src = probs + c0 + (size_t)(col_ok ? lane : 0);
#pragma unroll 8
        for (int r = 0; r < kWave; ++r) {
            const F v = src[(first + (size_t)(r < n_rows ? r : 0) * step) * K];
            if (r < n_rows && col_ok) tile[r * kCatPitch + lane] = v;
        }
    }
}

// encoder pass 1: entry i of the symbol matrix (flat: either layout) from row i of the probability matrix
template <class F>
__global__ __launch_bounds__(kWave) void categorical_entries_kernel(int P, uint32_t K, const int32_t* __restrict__ sym,
                                                                    const F* __restrict__ probs, size_t n, EncEntry* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    F* tile = reinterpret_cast<F*>(smem);
    const int lane = threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * kWave;
    if (i0 >= n) return;
    const int n_rows = (int)(n - i0 < (size_t)kWave ? n - i0 : (size_t)kWave);
    const bool active = lane < n_rows;
    const uint32_t sy = active ? (uint32_t)sym[i0 + lane] : 0u;         // (a negative symbol: beyond every column)
    const bool vec = cat_vec_ok(probs, K);
    const F* my = tile + lane * kCatPitch;
    CatSum<F> sum;
    F cum_left = F(0), cum_right = F(0);
    for (size_t c0 = 0; c0 < K; c0 += kCatChunk) {
        const int n_here = (int)(K - c0 < (size_t)kCatChunk ? K - c0 : (size_t)kCatChunk);
        wave_lds_fence();                                               // (the previous chunk has been walked)
        cat_stage(tile, probs, i0, 1, n_rows, K, c0, n_here, vec, lane);
        wave_lds_fence();
        const uint32_t rel = sy - (uint32_t)c0;                         // the symbol's column of this chunk, if it is in it
#pragma unroll 8
        for (int j = 0; j < n_here; ++j) {
            const F p = my[j];
            cum_left = (uint32_t)j == rel ? sum.cum : cum_left;
            sum.add(p);
            cum_right = (uint32_t)j == rel ? sum.cum : cum_right;
        }
    }
    if (!active) return;
    uint32_t c = 0, p = 0;
    if (!sum.bad() && sy < K) cat_interval<F>(P, K, sy, cum_left, cum_right, cat_scale<F>(P, K, sum.cum), c, p);
    out[i0 + lane] = make_entry(c, p);
}

} // namespace cst
