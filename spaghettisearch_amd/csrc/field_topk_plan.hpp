// field_topk_plan.hpp — the part of ss_field_topk (field_topk.hip) that needs no device and is the call's own: the checks
// of its arguments with their messages, the key that orders docs by a field value, the bytes of the candidate buffer and of the partial
// lists, and how many queries share the partial lists.  The blocks, runs, groups, launches and the best-K's size and order are
// match_set_plan.hpp's.  The constexpr functions are compiled for both sides (the kernels call them;
// tests/field_topk_plan_harness.cpp runs them on the host under ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include "match_set_plan.hpp"

#include <cstdio>

namespace ss {
namespace ftopk {

using namespace mset;                              // the shared names stay reachable under this namespace

constexpr uint64_t DEFAULT_SCRATCH_BYTES = 256ull << 20;    // option "ftopk.scratch_bytes"
constexpr uint64_t ENTRY_BYTES = 12;                        // a partial entry: 8 bytes of key, 4 of doc id
constexpr uint64_t RUN_BYTES = 8;                           // per run: its match count and the length of its list

// ---- the key.  A doc sorts by (vkey, doc) ascending, both unsigned: vkey = the value with its sign bit flipped (signed order becomes
// unsigned order), complemented for descending (unsigned order reversed, no overflow at either end); the doc id is never complemented,
// so docs of equal value come in ascending doc id in both directions (mset::key_less).  A doc id is below 2^32 - 1, so no entry is the
// pad entry.
constexpr uint64_t SIGN = 0x8000000000000000ull;
constexpr uint64_t value_key(int64_t value, bool descending) {
    const uint64_t u = (uint64_t)value ^ SIGN;
    return descending ? ~u : u;
}
constexpr int64_t key_value(uint64_t vkey, bool descending) { return (int64_t)((descending ? ~vkey : vkey) ^ SIGN); }

// ---- the candidate buffer: mset::buffer_entries(K) entries of a key and a doc id
constexpr uint32_t buffer_lds_bytes(uint32_t K) { return mset::buffer_entries(K) * (uint32_t)ENTRY_BYTES; }

// ---- groups.  The partial lists of a group of queries are [group][R][K] entries plus RUN_BYTES per run; the groups of a call re-use
// one scratch block in stream order.  As many queries as fit into scratch_bytes, at least one, at most n_active and MAX_GRID.
constexpr uint64_t query_bytes(uint32_t R, uint32_t K) { return (uint64_t)R * ((uint64_t)K * ENTRY_BYTES + RUN_BYTES); }
constexpr uint64_t scratch_bytes_of(int64_t option) { return option < 1 ? DEFAULT_SCRATCH_BYTES : (uint64_t)option; }
constexpr uint32_t group_queries(uint64_t n_active, uint32_t R, uint32_t K, uint64_t scratch_bytes) {
    uint64_t g = scratch_bytes / query_bytes(R ? R : 1, K ? K : 1);
    if (g < 1) g = 1;
    if (g > mset::MAX_GRID) g = mset::MAX_GRID;
    if (g > n_active) g = n_active;
    return (uint32_t)g;
}

// ---- the call's own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code)
inline int check_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_docs_out, bool has_n_out, int32_t field,
                      int32_t first, int32_t k, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return mset::INVALID; }
    if (n_q == 0) return mset::OK;                  // an empty batch is SS_OK whatever the other arguments say: nothing is read
    if (k < 1 || first < 0) { std::snprintf(msg, cap, "%s: k = %d must be >= 1 and first = %d >= 0", entry, k, first); return mset::INVALID; }
    if ((int64_t)first + (int64_t)k > (int64_t)mset::MAX_K) {
        std::snprintf(msg, cap, "%s: first + k = %lld exceeds SS_MAX_TOPK = %d (a deeper page: a range clause on the last value seen)", entry,
                      (long long)first + (long long)k, mset::MAX_K);
        return mset::UNSUPPORTED;
    }
    if (!has_q_ptr || !has_docs_out || !has_n_out) { std::snprintf(msg, cap, "%s: q_ptr, docs_out or n_out is NULL", entry); return mset::INVALID; }
    if (n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return mset::STATE; }
    if (field < 0 || field >= n_fields) { std::snprintf(msg, cap, "%s: field %d (the scorer has %d fields)", entry, field, n_fields); return mset::INVALID; }
    return mset::OK;
}

}  // namespace ftopk
}  // namespace ss
