// cst_categorical_perfect.hpp -- the launcher of the device quantiser behind Categorical(perfect=True)
// (cst_categorical_perfect.hip), for the per-symbol coders' host glue in cst_persymbol_categorical.hip.
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

// the name note_kernel() gets from the callers
extern const char* const kCatPerfectKernelName;

} // namespace cst
