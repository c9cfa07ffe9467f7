// cst_categorical_perfect.hpp -- the launchers of the device quantiser behind Categorical(perfect=True)
// (cst_categorical_perfect.hip), for the per-symbol coders' host glue in cst_persymbol_categorical.hip and, with the
// ragged addressing, in cst_persymbol_categorical_ragged.hip.
#pragma once
#include "cst_common.hpp"

namespace cst {

constexpr int kCatPerfectMaxK = CST_CATEGORICAL_PERFECT_MAX_K;

// One wave quantises one row.  The rows are addressed as the rows of categorical_rows_kernel are: output row
// o = s * count + (t - t0) comes from the probabilities of (stream s, position t), t0 <= t < t0 + count.
//   rows != null     the tabulated row: `pitch` >= K + 1 words, the K left cumulatives and then 2^P up to the pitch; a bad or
//                    non-converged row is 0xffffffff followed by 2^P
//   entries != null  "entry" mode (t0 = 0, count = N): only the encoder entry of symbols[s][t], at the symbol's place in the
//                    matrix; probability 0 (impossible) for a bad row and for a symbol outside [0, K)
// bad (0 good, 1 bad model, 2 not converged) and moves (unit moves of the search) are optional, one per output row.
struct CatPerfectArgs {
    const void* probs;          // [the symbols' shape][K], f32 or f64
    int32_t prob_bytes;
    uint32_t K; int32_t P, layout;
    size_t n_streams, N, t0, count;
    uint32_t* rows; size_t pitch;
    const int32_t* symbols; EncEntry* entries;
    int32_t* bad; uint32_t* moves;
};

// checks nothing but the grid: the callers have checked 2 <= K <= kCatPerfectMaxK, K <= 2^P and P <= 31
cst_status launch_categorical_perfect(const CatPerfectArgs& a, hipStream_t hs);

// where a stream's symbols lie, judged before anything becomes an address: a range that runs backwards or is too long for one coder
// (CST_STREAM_CAPACITY, as the other ragged calls say), or one that reaches beyond the n_total rows there are (CST_STREAM_INVALID_DATA).
// Either way the stream has NO symbols for the kernel.  (Here because the ragged Categorical coders of both quantisers judge by it:
// cst_persymbol_categorical_ragged.hip and the ragged mode of the quantiser below.)
struct CatRaggedSpan {
    uint64_t lo; uint32_t len; bool too_long, beyond;
    __device__ __forceinline__ CatRaggedSpan(uint64_t sym_lo, uint64_t sym_hi, uint64_t n_total) {
        too_long = sym_hi < sym_lo || sym_hi - sym_lo > 0xffffffffull;
        beyond = !too_long && sym_hi > sym_lo && sym_hi > n_total;
        lo = sym_lo;
        len = too_long || beyond ? 0u : (uint32_t)(sym_hi - sym_lo);
    }
    __device__ __forceinline__ int32_t status(int32_t coded) const {
        return too_long ? (int32_t)CST_STREAM_CAPACITY : beyond ? (int32_t)CST_STREAM_INVALID_DATA : coded;
    }
};

// The quantiser's RAGGED addressing (tabulation only): the rows of a flat matrix [n_total][K] that belong to a group of
// `n_streams` UNITS, slots [u0, u0 + n_streams) -- a unit is a stream of a ragged batch (slot i is stream order[i], null: i; its rows
// [sym_offsets[s], sym_offsets[s + 1])) or, where sym_lo is not null, an entry of a jump table with its rows given outright
// (sym_lo[i], len[i]).  Output row o = u * count + (t - t0) comes from flat row lo_u + t, t0 <= t < t0 + count; a wave whose
// t >= len_u writes nothing.  A unit that CatRaggedSpan refuses, one that names no stream, and one longer than max_len have no rows.
struct CatPerfectRaggedArgs : CatPerfectArgs {
    uint64_t n_total;
    size_t u0, n_all;                // the group's first slot; all slots (streams, or table entries)
    const uint64_t* sym_offsets;     // [n_all + 1]
    const uint32_t* order;           // null, or [n_all]
    const uint64_t* sym_lo;          // null, or [n_all] with len
    const uint32_t* len;
    uint64_t max_len;
};
cst_status launch_categorical_perfect_ragged(const CatPerfectRaggedArgs& a, hipStream_t hs);

// the name note_kernel() gets from the callers
extern const char* const kCatPerfectKernelName;

} // namespace cst
