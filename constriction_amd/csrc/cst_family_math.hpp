// cst_family_math.hpp -- the libm-crate (musl / FreeBSD msun) elementary functions behind the Laplace and Cauchy families and the
// `probability` crate's two CDFs over them, bit for bit.  Shared by the table builder (cst_families.hip, which names the sources
// and keeps the Binomial's functions) and the per-symbol coders (cst_persymbol*.hip).  Like everything in cst_math.hpp this needs
// -ffp-contract=off: each operation rounds once, in the order written.
#pragma once
#include "cst_math.hpp"

#define CST_HD __host__ __device__ __forceinline__

namespace cst {

CST_HD uint64_t bits_of(double x) { return __builtin_bit_cast(uint64_t, x); }
CST_HD double from_bits(uint64_t u) { return __builtin_bit_cast(double, u); }
CST_HD uint32_t top_word(double x) { return (uint32_t)(bits_of(x) >> 32); }
CST_HD double replace_top(double x, uint32_t hi) { return from_bits(((uint64_t)hi << 32) | (bits_of(x) & 0xffffffffull)); }

// The shared tail of msun's log and log1p: x = 2^k (1 + f) with sqrt(2)/2 <= 1 + f < sqrt(2),
// log(x) = k ln2 + f - f^2/2 + s (f^2/2 + R(s^2)), s = f / (2 + f); `corr` is log1p's correction term (0 for log,
// where `dk * ln2_lo + 0.0` is the same number)
CST_HD double log_tail(double f, int k, double corr) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01, L3 = 2.857142874366239149e-01,
                     L4 = 2.222219843214978396e-01, L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
                     L7 = 1.479819860511658591e-01;
    const double hfsq = 0.5 * f * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double even = w * (L2 + w * (L4 + w * L6));
    const double odd = z * (L1 + w * (L3 + w * (L5 + w * L7)));
    const double R = odd + even;
    const double dk = (double)k;
    return s * (hfsq + R) + (dk * ln2_lo + corr) - hfsq + f + dk * ln2_hi;
}

// libm `log` (FreeBSD e_log.c)
CST_HD double log_exact(double x) {
    uint32_t hx = top_word(x);
    int k = 0;
    if (hx < 0x00100000u || (hx >> 31)) {
        if ((bits_of(x) << 1) == 0) return -1.0 / (x * x);
        if (hx >> 31) return (x - x) / 0.0;
        k = -54;                                     // subnormal: scale up
        x *= 0x1p54;
        hx = top_word(x);
    } else if (hx >= 0x7ff00000u) {
        return x;
    } else if (bits_of(x) == 0x3ff0000000000000ull) {
        return 0.0;
    }
    hx += 0x3ff00000u - 0x3fe6a09eu;                 // into [sqrt(2)/2, sqrt(2))
    k += (int)(hx >> 20) - 0x3ff;
    const double m = replace_top(x, (hx & 0x000fffffu) + 0x3fe6a09eu);
    return log_tail(m - 1.0, k, 0.0);
}

// libm `log1p` (FreeBSD s_log1p.c as arranged by musl)
CST_HD double log1p_exact(double x) {
    const uint32_t hx = top_word(x);
    if (hx < 0x3fda827au || (hx >> 31)) {            // 1 + x < sqrt(2)
        if (hx >= 0xbff00000u) return x == -1.0 ? x / 0.0 : (x - x) / 0.0;
        if ((hx << 1) < (0x3ca00000u << 1)) return x;                        // |x| < 2^-53
        if (hx <= 0xbfd2bec4u) return log_tail(x, 0, 0.0);                   // sqrt(2)/2 <= 1 + x: no reduction
    } else if (hx >= 0x7ff00000u) {
        return x;
    }
    const double u = 1.0 + x;
    uint32_t hu = top_word(u) + (0x3ff00000u - 0x3fe6a09eu);
    const int k = (int)(hu >> 20) - 0x3ff;
    double corr = 0.0;                               // log(1 + x) - log(u), from the rounding error of 1 + x
    if (k < 54) corr = (k >= 2 ? 1.0 - (u - x) : x - (u - 1.0)) / u;
    const double m = replace_top(u, (hu & 0x000fffffu) + 0x3fe6a09eu);
    return log_tail(m - 1.0, k, corr);
}

// libm `atan` (FreeBSD s_atan.c): argument reduction against atan(0.5), atan(1), atan(1.5), atan(inf)
__device__ inline double atan_exact(double x) {
    constexpr double hi_part[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
                                   1.57079632679489655800e+00};
    constexpr double lo_part[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
                                   6.12323399573676603587e-17};
    constexpr double T0 = 3.33333333333329318027e-01, T1 = -1.99999999998764832476e-01, T2 = 1.42857142725034663711e-01,
                     T3 = -1.11111104054623557880e-01, T4 = 9.09088713343650656196e-02, T5 = -7.69187620504482999495e-02,
                     T6 = 6.66107313738753120669e-02, T7 = -5.83357013379057348645e-02, T8 = 4.97687799461593236017e-02,
                     T9 = -3.65315727442169155270e-02, T10 = 1.62858201153657823623e-02;
    const uint32_t hx = top_word(x), ix = hx & 0x7fffffffu;
    const bool neg = (hx >> 31) != 0;
    if (ix >= 0x44100000u) {                         // |x| >= 2^66
        if (x != x) return x;
        const double z = hi_part[3] + (double)0x1p-120f;
        return neg ? -z : z;
    }
    int id = -1;
    double r = x;
    if (ix >= 0x3fdc0000u) {                         // |x| >= 0.4375
        const double ax = fabs(x);
        if (ix < 0x3fe60000u) { id = 0; r = (2.0 * ax - 1.0) / (2.0 + ax); }
        else if (ix < 0x3ff30000u) { id = 1; r = (ax - 1.0) / (ax + 1.0); }
        else if (ix < 0x40038000u) { id = 2; r = (ax - 1.5) / (1.0 + 1.5 * ax); }
        else { id = 3; r = -1.0 / ax; }
    } else if (ix < 0x3e400000u) {                   // |x| < 2^-27
        return x;
    }
    const double z = r * r, w = z * z;
    const double s1 = z * (T0 + w * (T2 + w * (T4 + w * (T6 + w * (T8 + w * T10)))));
    const double s2 = w * (T1 + w * (T3 + w * (T5 + w * (T7 + w * T9))));
    if (id < 0) return r - r * (s1 + s2);
    const double y = hi_part[id] - (r * (s1 + s2) - lo_part[id] - r);
    return neg ? -y : y;
}

// ---- probability 0.20.3 `distribution` (the CDFs) ----

__device__ inline double laplace_cdf_exact(double x, double mu, double b) {
    return x <= mu ? 0.5 * exp_exact((x - mu) / b) : 1.0 - 0.5 * exp_exact((mu - x) / b);
}

__device__ inline double cauchy_cdf_exact(double x, double x0, double gamma) {
    constexpr double pi = 3.14159265358979323846264338327950288;
    return atan_exact((x - x0) / gamma) / pi + 0.5;
}

} // namespace cst
