// maxsim_plan.hpp — the part of ss_scorer_set_doc_tokens, ss_hit_maxsim_scores and ss_rerank_hits_by_maxsim (maxsim.hip)
// that needs no device: the checks of tok_ptr, qt_ptr and dim, how many tiles of 16 query-token slots a call's kernel holds, the LDS it
// asks for, the window rows of one workgroup and the grid that covers every (query, row) once, and the clamping of option
// "maxsim.wide_tokens".  tests/maxsim_plan_harness.cpp runs all of it on the host under ASan + UBSan.  Includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace ss {
namespace msp {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2 };            // what a check returns; maxsim.hip maps them to the ABI's codes
constexpr uint32_t MAX_QUERY_TOKENS = 64;                 // SS_MAX_QUERY_TOKENS (maxsim.hip asserts the equality)
constexpr uint32_t MAX_DIM = 1024;                        // SS_MAX_VEC_DIM (likewise)
constexpr uint32_t MAX_WINDOW = 1024;                     // SS_MAX_TOPK (likewise)
constexpr uint32_t ROW_PAD = 16;                          // bytes between the query-token rows of the LDS image (rows of dim bytes would all start in bank 0)
constexpr uint32_t WAVES = 4, TPB = 64 * WAVES;           // a workgroup of k_maxsim_scores
constexpr uint32_t TILE_TOKENS = 16, ITER_TOKENS = 64;    // doc tokens of one MFMA tile and of one iteration (four tiles)
constexpr uint32_t MAX_WG_ROWS = 64;                      // window rows of one workgroup: one ballot of a wave finds its wide rows
constexpr uint32_t DEFAULT_WIDE_TOKENS = 1024;            // option "maxsim.wide_tokens" (DESIGN.md K4x has the sweep it comes from)
constexpr uint32_t MAX_WIDE_TOKENS = 1u << 30;
constexpr uint64_t MAX_DOC_TOKENS = (1ull << 31) - 1;     // T_d the kernel's 32-bit token counters hold

// dim of a token table: a multiple of 64 in [64, MAX_DIM]
constexpr bool dim_ok(int64_t dim) { return dim >= 64 && dim <= (int64_t)MAX_DIM && dim % 64 == 0; }

// tok_ptr [n_docs + 1]: starts at 0, never decreases, no doc of more than MAX_DOC_TOKENS tokens.  The text of a refusal goes to msg.
inline int check_tok_ptr(char* msg, size_t cap, const char* entry, const uint64_t* tok_ptr, uint64_t n_docs) {
    if (tok_ptr[0] != 0) {
        std::snprintf(msg, cap, "%s: tok_ptr[0] = %llu must be 0", entry, (unsigned long long)tok_ptr[0]);
        return INVALID;
    }
    for (uint64_t d = 0; d < n_docs; d++)
        if (tok_ptr[d + 1] < tok_ptr[d]) {
            std::snprintf(msg, cap, "%s: tok_ptr not non-decreasing at doc %llu", entry, (unsigned long long)d);
            return INVALID;
        }
    for (uint64_t d = 0; d < n_docs; d++)
        if (tok_ptr[d + 1] - tok_ptr[d] > MAX_DOC_TOKENS) {
            std::snprintf(msg, cap, "%s: doc %llu has %llu tokens, 2^31 or more", entry, (unsigned long long)d,
                          (unsigned long long)(tok_ptr[d + 1] - tok_ptr[d]));
            return UNSUPPORTED;
        }
    return OK;
}

// qt_ptr [n_q + 1]: never decreases (INVALID), no query of more than MAX_QUERY_TOKENS tokens (UNSUPPORTED).  *max_m: the largest m_q.
inline int check_qt_ptr(char* msg, size_t cap, const char* entry, const uint32_t* qt_ptr, uint64_t n_q, uint32_t* max_m) {
    *max_m = 0;
    for (uint64_t q = 0; q < n_q; q++)
        if (qt_ptr[q + 1] < qt_ptr[q]) {
            std::snprintf(msg, cap, "%s: qt_ptr not non-decreasing", entry);
            return INVALID;
        }
    for (uint64_t q = 0; q < n_q; q++) {
        const uint32_t m = qt_ptr[q + 1] - qt_ptr[q];
        if (m > MAX_QUERY_TOKENS) {
            std::snprintf(msg, cap, "%s: query %llu has %u tokens, more than SS_MAX_QUERY_TOKENS = %u", entry, (unsigned long long)q, m, MAX_QUERY_TOKENS);
            return UNSUPPORTED;
        }
        if (m > *max_m) *max_m = m;
    }
    return OK;
}

// tiles of 16 query-token slots the kernel of a call holds, from the call's largest m_q <= MAX_QUERY_TOKENS: 1, 2 or 4
constexpr uint32_t qt_of(uint32_t max_m) { return max_m <= 16 ? 1u : max_m <= 32 ? 2u : 4u; }
// dynamic LDS of k_maxsim_scores<qt>: the query's token rows, and one maximum per wave and slot for the rows the waves share
constexpr uint32_t row_stride(uint32_t dim) { return dim + ROW_PAD; }
constexpr uint32_t lds_bytes(uint32_t qt, uint32_t dim) { return 16 * qt * row_stride(dim) + WAVES * 16 * qt * (uint32_t)sizeof(int32_t); }

// The grid: workgroup b belongs to query b / wgs_per_query and the window rows [r0, r0 + wg_rows) below k_in, r0 = (b % wgs_per_query) *
// wg_rows.  wg_rows is a multiple of WAVES, at most MAX_WG_ROWS; a call of few queries gets short runs so that about four workgroups
// per compute unit exist.
struct Grid {
    uint32_t wg_rows = 0, wgs_per_query = 0;
    uint64_t n_wgs = 0;
    bool ok = false;                                      // false: more workgroups than one launch holds
};
inline Grid grid(uint64_t n_q, uint32_t k_in, uint32_t cu_count) {
    Grid g;
    if (n_q == 0 || k_in == 0) return g;
    const uint64_t target = 4ull * (cu_count ? cu_count : 1);
    uint64_t want = (target + n_q - 1) / n_q;             // workgroups per query that would reach the target
    const uint32_t most = (k_in + WAVES - 1) / WAVES;
    if (want > most) want = most;
    if (want < 1) want = 1;
    uint32_t rows = (uint32_t)((k_in + want - 1) / want);
    if (rows > MAX_WG_ROWS) rows = MAX_WG_ROWS;
    uint32_t per_q = (k_in + rows - 1) / rows;
    rows = ((k_in + per_q - 1) / per_q + WAVES - 1) / WAVES * WAVES;   // the same number of workgroups, evenly filled
    per_q = (k_in + rows - 1) / rows;
    g.wg_rows = rows;
    g.wgs_per_query = per_q;
    g.n_wgs = n_q * per_q;
    g.ok = g.n_wgs <= 0x7FFFFFFFull;
    return g;
}

// the option's value: what the caller set, anything below 1 as the default, at most MAX_WIDE_TOKENS
constexpr uint32_t wide_tokens_of(int64_t option) {
    return option < 1 ? DEFAULT_WIDE_TOKENS : option > (int64_t)MAX_WIDE_TOKENS ? MAX_WIDE_TOKENS : (uint32_t)option;
}

}  // namespace msp
}  // namespace ss
