// cst_family_policy.hpp -- what the per-symbol coders (cst_persymbol*.hip) need to know about a model FAMILY, at compile time.
//
// The reference's flagship call  coder.encode_reverse(symbols, Family(lo, hi), param_a, param_b)  is the same for
// QuantizedGaussian, QuantizedLaplace and QuantizedCauchy (src/pybindings/stream/model.rs:600-900): every symbol gets its own
// LeakyQuantizer<f64, i32, u32, P> over the family's CDF (quantize.rs:525-568),
//     L[0] = 0,   L[i] = (f64 as u32)(free_weight * cdf(lo + i - 0.5)) + i,   L[n] = 2^P,   free_weight = (2^P - 1) - (n - 1).
// A policy provides
//     valid(a, b)                     the parameter test (an invalid model fails its stream: CST_STREAM_IMPOSSIBLE_SYMBOL)
//     lcp(sym, ...)                   (left, prob) of one symbol: the encoders
//     left<INNER>(i, ...)             L[i]: the decoders' probes
//     left3(g, ...)                   L[g - 1], L[g], L[g + 1] at once, 1 <= g <= n - 1: the lane decoder's first look
//     guess_z(tail) / guess_z_coarse  the standardised quantile of the LOWER tail (<= 0) in f32, tail in (0, 0.5]: the three
//                                     families are symmetric location-scale families, so the real number whose cdf is u lies
//                                     near  a + b * (u < 1/2 ? z : -z).  A STARTING POINT for the decoders' bracket search: a guess
//                                     that is off costs probes, never correctness -- the decoded symbol is the unique i with
//                                     L[i] <= q < L[i + 1] whatever the search.
//     kErfTab                         whether the kernels stage the erf tables of cst_math.hpp in LDS (the Gaussian only)
// Every `tab` argument is that table (null for the other families).
#pragma once
#include "cst_math.hpp"
#include "cst_family_math.hpp"

namespace cst {

// Acklam's rational approximation of the inverse normal CDF in f32 with the hardware's approximate log, sqrt and
// reciprocal: a STARTING POINT for the search (a guess that is off costs probes, never correctness).
// `tail` = min(p, 1 - p) in (0, 0.5]; returns the (negative) quantile of the lower tail.
__device__ __forceinline__ float ndtri_lower_f32(float tail) {
    constexpr float a1 = -3.969683028665376e+01f, a2 = 2.209460984245205e+02f, a3 = -2.759285104469687e+02f, a4 = 1.383577518672690e+02f,
        a5 = -3.066479806614716e+01f, a6 = 2.506628277459239e+00f, b1 = -5.447609879822406e+01f, b2 = 1.615858368580409e+02f,
        b3 = -1.556989798598866e+02f, b4 = 6.680131188771972e+01f, b5 = -1.328068155288572e+01f, c1 = -7.784894002430293e-03f,
        c2 = -3.223964580411365e-01f, c3 = -2.400758277161838e+00f, c4 = -2.549732539343734e+00f, c5 = 4.374664141464968e+00f,
        c6 = 2.938163982698783e+00f, d1 = 7.784695709041462e-03f, d2 = 3.224671290700398e-01f, d3 = 2.445134137142996e+00f,
        d4 = 3.754408661907416e+00f;
    // both branches, then a select: cheaper than diverging over 25 instructions
    // (explicit fused multiply-adds: the library is built with -ffp-contract=off for its bit-exact f64 paths, and a guess
    // has no bits to keep)
    auto f = [](float a, float b, float c) { return __builtin_fmaf(a, b, c); };
    const float q = __builtin_amdgcn_sqrtf(-1.3862943611f * __builtin_amdgcn_logf(tail));          // sqrt(-2 ln(tail))
    const float zt = f(f(f(f(f(c1, q, c2), q, c3), q, c4), q, c5), q, c6) * __builtin_amdgcn_rcpf(f(f(f(f(d1, q, d2), q, d3), q, d4), q, 1.0f));
    const float u = tail - 0.5f, r = u * u;
    const float zc = f(f(f(f(f(a1, r, a2), r, a3), r, a4), r, a5), r, a6) * u * __builtin_amdgcn_rcpf(f(f(f(f(f(b1, r, b2), r, b3), r, b4), r, b5), r, 1.0f));
    return tail < 0.02425f ? zt : zc;
}

// The same quantile from Abramowitz & Stegun 26.2.23 (|error| < 4.5e-4 over the whole lower half): a third of the instructions.
// Good for a first probe as long as 4.5e-4 sigma stays well below half a symbol; the lane decoder uses it when no lane of the
// wave has sigma >= 200.
__device__ __forceinline__ float ndtri_lower_coarse_f32(float tail) {
    const float t = __builtin_amdgcn_sqrtf(-1.3862943611f * __builtin_amdgcn_logf(tail));          // sqrt(-2 ln(tail))
    const float num = __builtin_fmaf(__builtin_fmaf(0.010328f, t, 0.802853f), t, 2.515517f);
    const float den = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(0.001308f, t, 0.189269f), t, 1.432788f), t, 1.0f);
    return __builtin_fmaf(num, __builtin_amdgcn_rcpf(den), -t);
}

// `assert!(std > 0.0)` and finite parameters (pybindings/stream/model.rs:654-657; the Laplace and Cauchy constructors assert the
// same of their scale, model.rs:771-774, 871-874)
__device__ __forceinline__ bool family_params_valid(double a, double b) {
    return b > 0.0 && b <= 1.7976931348623157e308 && fabs(a) <= 1.7976931348623157e308;
}

struct GaussianFamily {
    static constexpr bool kGaussian = true, kErfTab = true;
    __device__ static __forceinline__ bool valid(double mu, double sd) { return family_params_valid(mu, sd); }
    __device__ static __forceinline__ bool lcp(int32_t sym, int32_t lo, int32_t hi, int P, double mu, double sd, uint32_t& left, uint32_t& prob,
                                               const double2* tab) {
        return leaky_gaussian_lcp_quick(sym, lo, hi, P, 32, mu, sd, left, prob, tab);
    }
    template <bool INNER = false>
    __device__ static __forceinline__ uint32_t left(int32_t i, int32_t lo, int32_t n, int P, double mu, double sd, const double2* tab) {
        return leaky_gaussian_left_quick<INNER>(i, lo, n, P, 32, mu, sd, tab);
    }
    __device__ static __forceinline__ void left3(uint32_t g, int32_t lo, uint32_t n, int P, double mu, double sd, const double2* tab, uint32_t (&v)[3]) {
        leaky_gaussian_left3_quick(g, lo, n, P, mu, sd, tab, v);
    }
    __device__ static __forceinline__ float guess_z(float tail) { return ndtri_lower_f32(tail); }
    __device__ static __forceinline__ float guess_z_coarse(float tail) { return ndtri_lower_coarse_f32(tail); }
};

// free_weight * cdf(x), the reference's f64, OUT OF LINE: the exact exp and atan are branchy and long (atan: four argument
// reductions with a division each), and inlined at the five places a lane decoder evaluates a left cumulative they would be
// most of its code and its registers (see the comment above decode_lane_kernel).  One copy per family and translation unit.
static __device__ __attribute__((noinline)) double laplace_left_f64(double x, double mu, double b, double free_weight) {
    return free_weight * laplace_cdf_exact(x, mu, b);
}
static __device__ __attribute__((noinline)) double cauchy_left_f64(double x, double x0, double gamma, double free_weight) {
    return free_weight * cauchy_cdf_exact(x, x0, gamma);
}

// Laplace and Cauchy have no cheap evaluation with a proven bound (the Gaussian's is cst_math.hpp's fast erf): every left
// cumulative is the exact one.  CDF::left_f64 is one of the two functions above, CDF::z the f32 quantile.
template <class CDF>
struct ExactFamily {
    static constexpr bool kGaussian = false, kErfTab = false;
    __device__ static __forceinline__ bool valid(double a, double b) { return family_params_valid(a, b); }
    __device__ static __forceinline__ uint32_t total(int P) { return P >= 32 ? 0u : (1u << P); }
    // (f64 as u32)(free_weight * cdf(lo + i - 0.5)): x is a finite number, the parameters are valid -- no NaN comes out of
    // either CDF then, and the conversion saturates like Rust's
    __device__ static __forceinline__ uint32_t value(uint32_t i, int32_t lo, uint32_t n, int P, double a, double b) {
        const double free_weight = (double)((total(P) - 1u) - (n - 1u));
        const double x = (double)(int32_t)((uint32_t)lo + i) - 0.5;
        return f64_as_u32_hw(CDF::left_f64(x, a, b, free_weight));
    }
    template <bool INNER = false>
    __device__ static __forceinline__ uint32_t left(int32_t i, int32_t lo, int32_t n, int P, double a, double b, const double2*) {
        if constexpr (!INNER) {
            if (i <= 0) return 0u;
            if (i >= n) return total(P);
        }
        return value((uint32_t)i, lo, (uint32_t)n, P, a, b) + (uint32_t)i;
    }
    // (a rolled loop over one call site: three inlined argument set-ups buy nothing next to the call)
    __device__ static __forceinline__ void left3(uint32_t g, int32_t lo, uint32_t n, int P, double a, double b, const double2*, uint32_t (&v)[3]) {
#pragma unroll 1
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t i = g - 1u + k;                                  // 0 <= i <= n
            const uint32_t ic = min(max(i, 1u), n - 1u);                    // (the ends are not evaluated: 0 and 2^P)
            const uint32_t val = value(ic, lo, n, P, a, b) + ic;
            const uint32_t r = i == 0u ? 0u : i >= n ? total(P) : val;
            if (k == 0) v[0] = r; else if (k == 1) v[1] = r; else v[2] = r;
        }
    }
    // left_cumulative_and_probability (quantize.rs:525-568); a symbol outside [lo, hi] is evaluated as `lo` and reported by the
    // return value, as leaky_gaussian_lcp_quick does.  prob == 0 (or a wrapped one) marks a degenerate distribution.
    __device__ static __forceinline__ bool lcp(int32_t sym, int32_t lo, int32_t hi, int P, double a, double b, uint32_t& left_out, uint32_t& prob,
                                               const double2*) {
        const bool inside = sym >= lo && sym <= hi;
        const uint32_t n = (uint32_t)hi - (uint32_t)lo + 1u;
        const uint32_t i = inside ? (uint32_t)sym - (uint32_t)lo : 0u;
        uint32_t e[2];
#pragma unroll 1
        for (uint32_t k = 0; k < 2; ++k) {
            const uint32_t j = i + k;                                       // 0 <= j <= n
            const uint32_t jc = min(max(j, 1u), n - 1u);
            const uint32_t val = value(jc, lo, n, P, a, b) + jc;
            const uint32_t r = j == 0u ? 0u : j >= n ? total(P) : val;
            if (k == 0) e[0] = r; else e[1] = r;
        }
        left_out = e[0];
        prob = e[1] - e[0];
        return inside;
    }
    __device__ static __forceinline__ float guess_z(float tail) { return CDF::z(tail); }
    __device__ static __forceinline__ float guess_z_coarse(float tail) { return CDF::z(tail); }
};

struct LaplaceCdf {
    __device__ static __forceinline__ double left_f64(double x, double mu, double b, double fw) { return laplace_left_f64(x, mu, b, fw); }
    // cdf = exp(z) / 2 below the mean:  z = ln(2 tail) = ln 2 * log2(2 tail), with the hardware's log2
    __device__ static __forceinline__ float z(float tail) { return 0.69314718f * __builtin_amdgcn_logf(2.0f * tail); }
};
struct CauchyCdf {
    __device__ static __forceinline__ double left_f64(double x, double x0, double g, double fw) { return cauchy_left_f64(x, x0, g, fw); }
    // cdf = atan(z) / pi + 1/2:  z = tan(pi (tail - 1/2)) = -cot(pi tail).  The hardware's sin and cos take revolutions; far out
    // in the tail, where sin(pi tail) has few good bits left, the series 1 / (pi tail) - pi tail / 3 takes over.
    __device__ static __forceinline__ float z(float tail) {
        const float pt = 3.14159265f * tail;
        const float far = __builtin_fmaf(pt, -0.33333333f, __builtin_amdgcn_rcpf(pt));
        const float near = __builtin_amdgcn_cosf(0.5f * tail) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sinf(0.5f * tail));
        return -(tail < 0.03125f ? far : near);
    }
};
using LaplaceFamily = ExactFamily<LaplaceCdf>;
using CauchyFamily = ExactFamily<CauchyCdf>;

} // namespace cst
