// cst_categorical.hpp -- the "fast" quantisation of a row of floating-point probabilities, ONE implementation for host and device:
// fast_quantized_cdf (src/stream/model/categorical.rs:16-54) and LazyContiguousCategoricalEntropyModel
// (src/stream/model/categorical/lazy_contiguous.rs:131-331), which build the same table (the first tabulates it, the second
// evaluates the entries it needs), restated exactly:
//
//   cum_0 = 0,  cum_(i+1) = cum_i + p_i           in F, in index order: the ONE running sum is the normalisation (after the last
//                                                 entry) and every left cumulative.  Float addition is not associative: a tree sum
//                                                 or a wave-wide scan builds other tables, so one lane walks a row.
//   scale   = F(2^P - K) / norm                   one correctly rounded division
//   left(i) = trunc_saturating(cum_i * scale) + i Rust's `as u32` (saturates at u32::MAX, NaN -> 0); the addition wraps
//   right(K - 1) = 2^P                            whatever cum_K * scale gives
//
// No product may be contracted into an FMA (the build passes -ffp-contract=off) and f32 denormals are kept (softmax tails are
// subnormal).  Nothing here repairs a table: an f32 row whose last entry is exactly 0 can have left(K - 1) == 2^P, an empty last
// interval, and so has the reference's.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CST_CAT_HD __host__ __device__ __forceinline__
#else
#define CST_CAT_HD inline
#endif

namespace cst {

template <class F> struct CatFloat;
template <> struct CatFloat<float> {
    static constexpr float kMinNormal = 1.17549435e-38f, kMax = 3.4028234e38f;
};
template <> struct CatFloat<double> {
    static constexpr double kMinNormal = 2.2250738585072014e-308, kMax = 1.7976931348623157e308;
};

// Rust's `as u32` of a float: towards zero, saturating, NaN -> 0
template <class F>
CST_CAT_HD uint32_t cat_as_u32(F v) {
    if (!(v > F(0))) return 0u;
    if (v >= F(4294967296.0)) return 0xffffffffu;
    return (uint32_t)v;
}

// The running sum of a row and what makes the row a bad model.  The reference returns Err for a sum that is not normal or not
// positive (a NaN entry makes the sum NaN); a negative entry cannot give increasing cumulatives.
template <class F>
struct CatSum {
    F cum = F(0);
    F lowest = F(0);                                   // the smallest entry so far, NaN entries skipped (they spoil `cum`)
    CST_CAT_HD void add(F p) {
        lowest = p < lowest ? p : lowest;
        cum = cum + p;
    }
    CST_CAT_HD bool bad() const { return !(cum >= CatFloat<F>::kMinNormal) || cum > CatFloat<F>::kMax || lowest < F(0); }
};

template <class F>
CST_CAT_HD F cat_scale(int P, uint32_t K, F norm) { return F((1u << P) - K) / norm; }

// left cumulative of entry i, given the running sum in front of it
template <class F>
CST_CAT_HD uint32_t cat_left(F cum, F scale, uint32_t i) { return cat_as_u32<F>(cum * scale) + i; }

// The whole quantised row: cdf[0 .. K] with cdf[K] = 2^P.  Returns false for a bad model, whose row is written as
// cdf[0] = 0xffffffff (no quantile lies in it) followed by 2^P.
template <class F>
CST_CAT_HD bool cat_fast_cdf_row(int P, const F* probs, uint32_t K, uint32_t* cdf) {
    CatSum<F> sum;
    for (uint32_t i = 0; i < K; ++i) sum.add(probs[i]);
    const uint32_t total = 1u << P;
    if (sum.bad()) {
        cdf[0] = 0xffffffffu;
        for (uint32_t i = 1; i <= K; ++i) cdf[i] = total;
        return false;
    }
    const F scale = cat_scale<F>(P, K, sum.cum);
    F cum = F(0);
    for (uint32_t i = 0; i < K; ++i) {
        cdf[i] = cat_left<F>(cum, scale, i);
        cum = cum + probs[i];
    }
    cdf[K] = total;
    return true;
}

// (left, probability) of `symbol` as LazyContiguousCategoricalEntropyModel::left_cumulative_and_probability gives them, from the
// running sums in front of and behind the symbol's entry; probability 0: an impossible symbol (an empty or wrapped interval --
// the reference panics with "leakiness should guarantee nonzero probabilities")
template <class F>
CST_CAT_HD void cat_interval(int P, uint32_t K, uint32_t symbol, F cum_left, F cum_right, F scale, uint32_t& left, uint32_t& prob) {
    const uint32_t total = 1u << P;
    left = cat_left<F>(cum_left, scale, symbol);
    const uint32_t right = symbol == K - 1u ? total : cat_left<F>(cum_right, scale, symbol + 1u);
    prob = (right > left && right <= total) ? right - left : 0u;
}

} // namespace cst
