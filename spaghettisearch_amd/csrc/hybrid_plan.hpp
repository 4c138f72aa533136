// hybrid_plan.hpp — the part of ss_fuse_hits / ss_hybrid_topk (hybrid.hip) that needs no device: the checks of the
// fusion parameters and of the two windows, the fused score and the integer key that realises the defined order.  The score and the key
// are compiled for both sides (the kernels call them; tests/hybrid_plan_harness.cpp runs them on the host under ASan + UBSan).
// Includes nothing of HIP.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define SS_HYB_HD __host__ __device__
#else
#define SS_HYB_HD
#endif

namespace ss {
namespace hybrid {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2 };           // what a check returns; hybrid.hip maps them to the ABI's codes
constexpr int32_t MODE_RRF = 0, MODE_WEIGHTED = 1;       // SS_FUSE_RRF / SS_FUSE_WEIGHTED (hybrid.hip asserts the equality)
constexpr uint64_t NAN_BITS = 0x7FF8000000000000ull;     // how a NaN score is stored
constexpr uint64_t KEY_NAN = ~0ull;                      // the key of a NaN score: behind every other score's key

// The parameters of a fusion and the widths of its two windows and of its page.  `lex_name` / `vec_name`: the arguments' names in the
// caller's text (k_lex / k_vec, or k_window twice).  Writes the text of the first failed check to msg.
inline int check_fuse(char* msg, size_t cap, const char* entry, int32_t max_k, bool has_params, int32_t mode, int32_t rrf_c, double w_lex,
                      double w_vec, int32_t n_q, const char* lex_name, int32_t k_lex, const char* vec_name, int32_t k_vec, int32_t k,
                      int32_t first) {
    if (n_q < 0) { snprintf(msg, cap, "%s: n_q < 0", entry); return INVALID; }
    if (!has_params) { snprintf(msg, cap, "%s: fp is NULL", entry); return INVALID; }
    if (mode != MODE_RRF && mode != MODE_WEIGHTED) { snprintf(msg, cap, "%s: fp->mode = %d is neither SS_FUSE_RRF nor SS_FUSE_WEIGHTED", entry, mode); return INVALID; }
    if (rrf_c < 1) { snprintf(msg, cap, "%s: fp->rrf_c = %d must be >= 1", entry, rrf_c); return INVALID; }
    if (!std::isfinite(w_lex) || !std::isfinite(w_vec)) { snprintf(msg, cap, "%s: fp->w_lex or fp->w_vec is not finite", entry); return INVALID; }
    if (k_lex < 1) { snprintf(msg, cap, "%s: %s = %d must be >= 1", entry, lex_name, k_lex); return INVALID; }
    if (k_vec < 1) { snprintf(msg, cap, "%s: %s = %d must be >= 1", entry, vec_name, k_vec); return INVALID; }
    if (k < 1) { snprintf(msg, cap, "%s: k = %d must be >= 1", entry, k); return INVALID; }
    if (first < 0) { snprintf(msg, cap, "%s: first = %d must be >= 0", entry, first); return INVALID; }
    if (k_lex > max_k) { snprintf(msg, cap, "%s: %s = %d exceeds SS_MAX_TOPK = %d", entry, lex_name, k_lex, max_k); return UNSUPPORTED; }
    if (k_vec > max_k) { snprintf(msg, cap, "%s: %s = %d exceeds SS_MAX_TOPK = %d", entry, vec_name, k_vec, max_k); return UNSUPPORTED; }
    if (k > max_k) { snprintf(msg, cap, "%s: k = %d exceeds SS_MAX_TOPK = %d", entry, k, max_k); return UNSUPPORTED; }
    return OK;
}

// The fused score of a candidate with these ranks (0 = absent from the list), FinalRank and vector score.  Every operation is one
// rounding: the library and the harness are built with -ffp-contract=off.
SS_HYB_HD inline double fuse_score(int32_t mode, int32_t rrf_c, double w_lex, double w_vec, uint32_t lex_rank, uint32_t vec_rank, double fin,
                                   int32_t vec_score) {
    if (mode == MODE_RRF) {
        const double a = lex_rank ? w_lex / (double)((int64_t)rrf_c + (int64_t)lex_rank) : 0.0;
        const double b = vec_rank ? w_vec / (double)((int64_t)rrf_c + (int64_t)vec_rank) : 0.0;
        return a + b;
    }
    const double a = w_lex * fin;
    const double b = w_vec * (double)vec_score;
    return a + b;
}

SS_HYB_HD inline uint64_t double_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

// Ascending key order = the defined order of scores: the larger score has the smaller key, -0.0 and 0.0 share one, every NaN has
// KEY_NAN, which no other score reaches.  Candidates of equal key are ordered by doc (the caller's second word).
SS_HYB_HD inline uint64_t order_key(double score) {
    if (score != score) return KEY_NAN;
    if (score == 0.0) score = 0.0;                        // -0.0 -> 0.0
    const uint64_t u = double_bits(score);
    const uint64_t asc = (u >> 63) ? ~u : (u | (1ull << 63));   // ascending with the value
    return ~asc;                                          // (~asc == KEY_NAN only for asc == 0: u all ones, a NaN)
}

// the 8 bytes a score is stored as
SS_HYB_HD inline uint64_t stored_bits(double score) { return score != score ? NAN_BITS : double_bits(score); }

}  // namespace hybrid
}  // namespace ss
