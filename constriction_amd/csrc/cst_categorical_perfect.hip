// cst_categorical_perfect.hip -- Categorical(perfect=True) quantised on the device:
// `perfectly_quantized_probabilities` (src/stream/model/categorical.rs:56-177) plus the cumulation of contiguous.rs:301-313, the
// words of the host function cst_categorical_perfect_cdf (cst_families.hip), for many rows at once.
//
// The search moves one unit of weight at a time and every move depends on the one before, so ONE WAVE owns one row and the
// parallelism inside a move is its two selections over the K slots.  The reference keeps a vector of slots that it stable-sorts
// and then scans with max_by / min_by; here a slot stays at its index and carries its POSITION in that vector:
//   stable sort by win descending  =  the total order (win descending, previous position ascending): a slot's new position is
//                                     the number of slots in front of it, counted;
//   max_by(win) keeps the last maximum, min_by(loss) the first minimum  =  the maximum of (win, position) and the minimum of
//                                     (loss, position), total orders too, so a butterfly reduction is well defined
//                                     (-0.0 == 0.0 as in the reference: such ties go to the position).
// Slots live in wave-private LDS as five arrays (prob, win, loss: f64; weight, position: u32; 32 bytes a slot); lane l holds the
// slots l, l + 64, ...: consecutive lanes read consecutive addresses.  One wave per workgroup; the capacity is a template
// parameter (64 / 256 / 1024 slots = 2 / 8 / 32 KiB: 32 / 20 / 5 waves on a CU's 160 KiB).  No atomics, nothing crosses waves.
#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>
#include <vector>

#include "cst_categorical_perfect.hpp"
#include "cst_ans_kernels.hpp"
#include "cst_family_math.hpp"
#include "cst_categorical.hpp"

namespace cst {

const char* const kCatPerfectKernelName = "categorical_perfect_kernel";

// the search of a row stops after this many unit moves: a safety condition (the proven bound, K * 2^P, is no bound in practice;
// rows of every kind tried stay below K moves)
CST_HD uint32_t perfect_move_cap(uint32_t K) { return 16u * K + 1024u; }
// ... and the distribution of the left-over weight after this many rounds.  What truncation leaves over is below
// K + (2^P - K) * K * 2^-52 < K + 1 units, the sum of K fractional parts and of the rounding errors of norm and the shares:
// two rounds at the most.
constexpr int kPerfectMaxRounds = 4;

CST_HD double perfect_gain(double prob, uint32_t weight) { return prob * log1p_exact(1.0 / (double)weight); }
CST_HD double perfect_cost(double prob, uint32_t weight) {
    return weight == 1u ? std::numeric_limits<double>::infinity() : -prob * log1p_exact(-1.0 / (double)weight);
}
CST_HD bool perfect_norm_ok(double norm) { return norm >= CatFloat<double>::kMinNormal && norm <= CatFloat<double>::kMax; }

// floor(2^64 / p) as the coders' entries carry it (make_entry of cst_persymbol.hpp)
__device__ __forceinline__ EncEntry perfect_entry(uint32_t c, uint32_t p) {
    uint64_t m = 0;
    if (p == 1) m = ~0ull;
    else if (p > 1) {
        const uint64_t q = (~0ull) / p;
        const uint64_t r = (~0ull) - q * p;
        m = q + ((r + 1 == p) ? 1 : 0);
    }
    return EncEntry{c, p, (uint32_t)m, (uint32_t)(m >> 32)};
}

template <int CAP>
struct PerfectSlots {
    double prob[CAP], win[CAP], loss[CAP];
    uint32_t weight[CAP], pos[CAP];
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, kWave);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m, kWave);
    return v;
}

// RAGGED: the addressing of CatPerfectRaggedArgs (cst_categorical_perfect.hpp) -- `s` is then a unit of the group, and its wave leaves
// at once where the unit has no position t.  A template parameter, so the rectangular kernels stay the code they were.
template <class F, int CAP, bool RAGGED = false>
__global__ __launch_bounds__(kWave) void categorical_perfect_kernel(const std::conditional_t<RAGGED, CatPerfectRaggedArgs, CatPerfectArgs> a) {
    static_assert(CAP % kWave == 0, "a lane holds CAP / 64 slots");
    constexpr int kPer = CAP / kWave;
    __shared__ PerfectSlots<CAP> sl;
    const int lane = threadIdx.x;
    const uint32_t K = a.K;                                              // <= CAP (the launcher's choice)
    const size_t o = blockIdx.x;
    const size_t s = o / a.count, t = a.t0 + (o - s * a.count);
    size_t in_row;
    if constexpr (RAGGED) {
        const size_t slot = a.u0 + s;                                    // (< n_all: the launcher's group)
        uint64_t lo = 0, hi = 0;
        if (a.sym_lo) { lo = a.sym_lo[slot]; hi = lo + (uint64_t)a.len[slot]; }
        else {
            const size_t stream = a.order ? (size_t)a.order[slot] : slot;
            if (stream < a.n_all) { lo = a.sym_offsets[stream]; hi = a.sym_offsets[stream + 1]; }
        }
        const CatRaggedSpan span(lo, hi, a.n_total);
        if ((uint64_t)t >= (uint64_t)span.len || (uint64_t)span.len > a.max_len) return;      // (the same for the whole wave)
        in_row = (size_t)span.lo + t;                                    // (< n_total: the span lies inside the matrix)
    } else {
        in_row = a.layout == CST_LAYOUT_SYMBOL_MAJOR ? t * a.n_streams + s : s * a.N + t;
    }
    const F* src = reinterpret_cast<const F*>(a.probs) + in_row * (size_t)K;
    const uint32_t total = 1u << a.P;
    const double inf = std::numeric_limits<double>::infinity();

    // 1. initial weights
    bool negative = false;
    for (uint32_t i = lane; i < K; i += kWave) {
        const double p = (double)src[i];
        sl.prob[i] = p;
        negative = negative || p < 0.0;
    }
    wave_lds_fence();
    double norm = 0.0;                                                   // THE sequential sum, by every lane alike
#pragma unroll 8
    for (uint32_t i = 0; i < K; ++i) norm += sl.prob[i];
    int32_t code = (__any(negative) || !perfect_norm_ok(norm)) ? 1 : 0;
    uint32_t moves = 0;
    if (code == 0) {
        uint32_t left_over = total - K;
        const double scale = (double)left_over / norm;
        uint64_t extras = 0;
        for (uint32_t i = lane; i < K; i += kWave) {
            const double p = sl.prob[i];
            const uint32_t extra = cat_as_u32<double>(p * scale);
            extras += extra;
            const uint32_t w = extra + 1u;
            sl.weight[i] = w;
            sl.win[i] = perfect_gain(p, w);
            sl.loss[i] = perfect_cost(p, w);
            sl.pos[i] = i;
        }
        extras = wave_sum_u64(extras);
        // (the host function compares share by share with what is left: shares are not negative, so some prefix exceeds it
        // exactly if the whole sum does)
        if (extras > (uint64_t)left_over) code = 1;
        else left_over -= (uint32_t)extras;
        wave_lds_fence();

        // 2. what truncation left over: one unit each to the slots of the largest wins, the slots re-sorted every round
        for (int round = 0; code == 0 && left_over != 0u; ++round) {
            if (round == kPerfectMaxRounds) { code = 2; break; }
            double w[kPer];
            uint32_t p[kPer], in_front[kPer];
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const uint32_t i = (uint32_t)lane + (uint32_t)k * kWave;
                const bool mine = i < K;
                w[k] = mine ? sl.win[i] : 0.0;
                p[k] = mine ? sl.pos[i] : 0u;
                in_front[k] = 0u;
            }
            for (uint32_t j = 0; j < K; ++j) {
                const double wj = sl.win[j];                            // (every lane the same address: a broadcast)
                const uint32_t pj = sl.pos[j];
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    if ((uint32_t)k * kWave < K) in_front[k] += (wj > w[k] || (wj == w[k] && pj < p[k])) ? 1u : 0u;
                }
            }
            wave_lds_fence();                                            // (every position has been read)
            const uint32_t batch = left_over < K ? left_over : K;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const uint32_t i = (uint32_t)lane + (uint32_t)k * kWave;
                if (i < K) {
                    sl.pos[i] = in_front[k];
                    if (in_front[k] < batch) {
                        const uint32_t wt = sl.weight[i] + 1u;
                        const double pr = sl.prob[i];
                        sl.weight[i] = wt;
                        sl.win[i] = perfect_gain(pr, wt);
                        sl.loss[i] = perfect_cost(pr, wt);              // (wt >= 2)
                    }
                }
            }
            left_over -= batch;
            wave_lds_fence();
        }

        // 3. single units from the cheapest seller to the best buyer while that lowers the cross entropy
        const uint32_t cap = perfect_move_cap(K);
        while (code == 0) {
            double bw = -inf, sv = inf;                                 // a lane without slots: loses against every slot
            int32_t bp = -1, sp = 0x7fffffff;
            uint32_t bi = 0, si = 0;
            for (uint32_t i = lane; i < K; i += kWave) {
                const double wv = sl.win[i], lv = sl.loss[i];
                const int32_t ps = (int32_t)sl.pos[i];
                if (wv > bw || (wv == bw && ps > bp)) { bw = wv; bp = ps; bi = i; }
                if (lv < sv || (lv == sv && ps < sp)) { sv = lv; sp = ps; si = i; }
            }
#pragma unroll
            for (int m = kWave / 2; m > 0; m >>= 1) {
                const double ow = __shfl_xor(bw, m, kWave), ol = __shfl_xor(sv, m, kWave);
                const int32_t obp = __shfl_xor(bp, m, kWave), osp = __shfl_xor(sp, m, kWave);
                const uint32_t obi = (uint32_t)__shfl_xor((int)bi, m, kWave), osi = (uint32_t)__shfl_xor((int)si, m, kWave);
                if (ow > bw || (ow == bw && obp > bp)) { bw = ow; bp = obp; bi = obi; }
                if (ol < sv || (ol == sv && osp < sp)) { sv = ol; sp = osp; si = osi; }
            }
            if (bi == si || bw <= sv) break;
            if (moves == cap) { code = 2; break; }
            // (the same arithmetic on every lane; one lane stores)
            const uint32_t ws = sl.weight[si] - 1u, wb = sl.weight[bi] + 1u;        // (a seller's loss is finite: its weight >= 2)
            const double new_loss = perfect_cost(sl.prob[si], ws), new_win = perfect_gain(sl.prob[bi], wb);
            wave_lds_fence();
            if (lane == 0) {
                sl.weight[si] = ws; sl.win[si] = -inf; sl.loss[si] = new_loss;     // a weight that went down never goes up again,
                sl.weight[bi] = wb; sl.loss[bi] = inf; sl.win[bi] = new_win;       // and vice versa
            }
            wave_lds_fence();
            ++moves;
        }
    }

    // 4. output
    if (lane == 0) {
        if (a.bad) a.bad[o] = code;
        if (a.moves) a.moves[o] = moves;
    }
    if (a.entries) {
        const uint32_t sy = (uint32_t)a.symbols[in_row];                 // (a negative symbol: beyond every slot)
        const bool ok = code == 0 && sy < K;
        uint32_t part = 0;
        for (uint32_t i = lane; ok && i < sy; i += kWave) part += sl.weight[i];
        const uint32_t c = wave_sum_u32(part);
        if (lane == 0) a.entries[in_row] = ok ? perfect_entry(c, sl.weight[sy]) : perfect_entry(0u, 0u);
    }
    if (a.rows) {
        uint32_t* out = a.rows + o * a.pitch;
        uint32_t carry = 0;
        for (size_t c0 = 0; c0 < a.pitch; c0 += kWave) {
            const size_t i = c0 + (size_t)lane;
            const uint32_t w = (code == 0 && i < (size_t)K) ? sl.weight[i] : 0u;
            uint32_t incl = w;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d, kWave);
                if (lane >= d) incl += up;
            }
            uint32_t v = i < (size_t)K ? carry + incl - w : total;
            if (code != 0) v = i == 0 ? 0xffffffffu : total;
            if (i < a.pitch) out[i] = v;
            carry += (uint32_t)__shfl((int)incl, kWave - 1, kWave);
        }
    }
}

template <class F>
static void launch_perfect(const CatPerfectArgs& a, unsigned blocks, hipStream_t hs) {
    if (a.K <= 64u) hipLaunchKernelGGL((categorical_perfect_kernel<F, 64>), dim3(blocks), dim3(kWave), 0, hs, a);
    else if (a.K <= 256u) hipLaunchKernelGGL((categorical_perfect_kernel<F, 256>), dim3(blocks), dim3(kWave), 0, hs, a);
    else hipLaunchKernelGGL((categorical_perfect_kernel<F, kCatPerfectMaxK>), dim3(blocks), dim3(kWave), 0, hs, a);
}

cst_status launch_categorical_perfect(const CatPerfectArgs& a, hipStream_t hs) {
    if (a.K < 2u || a.K > (uint32_t)kCatPerfectMaxK) return CST_ERR_MODEL;       // (the slots of the largest kernel)
    const size_t blocks = a.n_streams * a.count;
    if (blocks == 0) return CST_OK;
    if (blocks > 0x7fffffffull) return CST_ERR_INVALID_ARGUMENT;
    if (a.prob_bytes == 4) launch_perfect<float>(a, (unsigned)blocks, hs);
    else launch_perfect<double>(a, (unsigned)blocks, hs);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

template <class F>
static void launch_perfect_ragged(const CatPerfectRaggedArgs& a, unsigned blocks, hipStream_t hs) {
    if (a.K <= 64u) hipLaunchKernelGGL((categorical_perfect_kernel<F, 64, true>), dim3(blocks), dim3(kWave), 0, hs, a);
    else if (a.K <= 256u) hipLaunchKernelGGL((categorical_perfect_kernel<F, 256, true>), dim3(blocks), dim3(kWave), 0, hs, a);
    else hipLaunchKernelGGL((categorical_perfect_kernel<F, kCatPerfectMaxK, true>), dim3(blocks), dim3(kWave), 0, hs, a);
}

// a.n_streams units from slot a.u0 on, a.count positions each: a block per output row, as above
cst_status launch_categorical_perfect_ragged(const CatPerfectRaggedArgs& a, hipStream_t hs) {
    if (a.K < 2u || a.K > (uint32_t)kCatPerfectMaxK || !a.rows || a.pitch < (size_t)a.K + 1) return CST_ERR_MODEL;
    if (a.u0 > a.n_all || a.n_streams > a.n_all - a.u0) return CST_ERR_INVALID_ARGUMENT;   // (the group lies inside the slots)
    if (a.count != 0 && a.n_streams > 0x7fffffffull / a.count) return CST_ERR_INVALID_ARGUMENT;
    const size_t blocks = a.n_streams * a.count;
    if (blocks == 0) return CST_OK;
    if (a.prob_bytes == 4) launch_perfect_ragged<float>(a, (unsigned)blocks, hs);
    else launch_perfect_ragged<double>(a, (unsigned)blocks, hs);
    CST_HIP_TRY(hipGetLastError());
    return CST_OK;
}

// The kernel's formulation on the CPU: slots at their indices with their positions, new positions by counting, the selections
// as maxima and minima of (value, position), the same two stops.  Returns 0 / 1 / 2 as the kernel's d_bad.
template <class F>
static int32_t perfect_row_host(int P, const F* probs, uint32_t K, uint32_t* cdf, uint32_t* n_moves) {
    const uint32_t total = 1u << P;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> prob(K), win(K), loss(K);
    std::vector<uint32_t> weight(K), pos(K), in_front(K);
    uint32_t moves = 0;
    int32_t code = 0;
    bool negative = false;
    double norm = 0.0;
    for (uint32_t i = 0; i < K; ++i) {
        prob[i] = (double)probs[i];
        negative = negative || prob[i] < 0.0;
        norm += prob[i];
    }
    if (negative || !perfect_norm_ok(norm)) code = 1;
    if (code == 0) {
        uint32_t left_over = total - K;
        const double scale = (double)left_over / norm;
        uint64_t extras = 0;
        for (uint32_t i = 0; i < K; ++i) {
            const uint32_t extra = cat_as_u32<double>(prob[i] * scale);
            extras += extra;
            weight[i] = extra + 1u;
            win[i] = perfect_gain(prob[i], weight[i]);
            loss[i] = perfect_cost(prob[i], weight[i]);
            pos[i] = i;
        }
        if (extras > (uint64_t)left_over) code = 1;
        else left_over -= (uint32_t)extras;
        for (int round = 0; code == 0 && left_over != 0u; ++round) {
            if (round == kPerfectMaxRounds) { code = 2; break; }
            for (uint32_t i = 0; i < K; ++i) {
                uint32_t n = 0;
                for (uint32_t j = 0; j < K; ++j) n += (win[j] > win[i] || (win[j] == win[i] && pos[j] < pos[i])) ? 1u : 0u;
                in_front[i] = n;
            }
            const uint32_t batch = std::min(left_over, K);
            for (uint32_t i = 0; i < K; ++i) {
                pos[i] = in_front[i];
                if (pos[i] < batch) {
                    weight[i] += 1u;
                    win[i] = perfect_gain(prob[i], weight[i]);
                    loss[i] = perfect_cost(prob[i], weight[i]);
                }
            }
            left_over -= batch;
        }
        const uint32_t cap = perfect_move_cap(K);
        while (code == 0) {
            uint32_t bi = 0, si = 0;
            for (uint32_t i = 1; i < K; ++i) {
                if (win[i] > win[bi] || (win[i] == win[bi] && pos[i] > pos[bi])) bi = i;
                if (loss[i] < loss[si] || (loss[i] == loss[si] && pos[i] < pos[si])) si = i;
            }
            if (bi == si || win[bi] <= loss[si]) break;
            if (moves == cap) { code = 2; break; }
            weight[si] -= 1u; win[si] = -inf; loss[si] = perfect_cost(prob[si], weight[si]);
            weight[bi] += 1u; loss[bi] = inf; win[bi] = perfect_gain(prob[bi], weight[bi]);
            ++moves;
        }
    }
    if (code != 0) {
        cdf[0] = 0xffffffffu;
        for (uint32_t i = 1; i <= K; ++i) cdf[i] = total;
    } else {
        uint32_t acc = 0;
        for (uint32_t i = 0; i < K; ++i) { cdf[i] = acc; acc += weight[i]; }
        cdf[K] = acc;
    }
    if (n_moves) *n_moves = moves;
    return code;
}

static cst_status check_perfect_rows_args(int32_t precision, const void* probs, int32_t prob_bytes, int32_t n_symbols, const void* rows) {
    if (!probs || !rows || (prob_bytes != 4 && prob_bytes != 8) || precision < 1 || precision > 31) return CST_ERR_INVALID_ARGUMENT;
    if (n_symbols < 2 || n_symbols > kCatPerfectMaxK || (uint64_t)n_symbols > ((uint64_t)1 << precision)) return CST_ERR_MODEL;
    return CST_OK;
}

} // namespace cst

using namespace cst;

extern "C" {

cst_status cst_categorical_perfect_cdf_rows(int32_t precision, const void* d_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                            uint32_t* d_rows, int32_t* d_bad, uint32_t* d_moves, void* stream) {
    if (cst_status st = check_perfect_rows_args(precision, d_probs, prob_bytes, n_symbols, d_rows)) return st;
    CatPerfectArgs a{};
    a.probs = d_probs; a.prob_bytes = prob_bytes; a.K = (uint32_t)n_symbols; a.P = precision; a.layout = CST_LAYOUT_STREAM_MAJOR;
    a.n_streams = 1; a.N = n_rows; a.t0 = 0; a.count = n_rows;
    a.rows = d_rows; a.pitch = (size_t)n_symbols + 1; a.bad = d_bad; a.moves = d_moves;
    return note_kernel(kCatPerfectKernelName, launch_categorical_perfect(a, (hipStream_t)stream));
}

cst_status cst_categorical_perfect_cdf_host(int32_t precision, const void* h_probs, int32_t prob_bytes, size_t n_rows, int32_t n_symbols,
                                            uint32_t* h_rows, int32_t* h_bad, uint32_t* h_moves) {
    if (cst_status st = check_perfect_rows_args(precision, h_probs, prob_bytes, n_symbols, h_rows)) return st;
    const size_t K = (size_t)n_symbols;
    for (size_t i = 0; i < n_rows; ++i) {
        uint32_t moves = 0;
        const int32_t code = prob_bytes == 4
            ? perfect_row_host<float>(precision, reinterpret_cast<const float*>(h_probs) + i * K, (uint32_t)K, h_rows + i * (K + 1), &moves)
            : perfect_row_host<double>(precision, reinterpret_cast<const double*>(h_probs) + i * K, (uint32_t)K, h_rows + i * (K + 1), &moves);
        if (h_bad) h_bad[i] = code;
        if (h_moves) h_moves[i] = moves;
    }
    return CST_OK;
}

} // extern "C"
