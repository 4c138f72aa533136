// group_topk_plan.hpp — the part of ss_top_groups (group_topk.hip) that needs no device and is the call's own: the
// checks of its arguments with their messages, the key that orders groups by count, the choice between the two counting paths, the
// stride of a query's counter row and how many queries have their rows inside the scratch bound.  The blocks, runs, groups, launches
// and the best-K's size and order are match_set_plan.hpp's.  The constexpr functions are compiled for both sides (the kernels call
// them; tests/group_topk_plan_harness.cpp runs them on the host under ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include "match_set_plan.hpp"

#include <cstdio>

namespace ss {
namespace gtopk {

using namespace mset;                              // the shared names stay reachable under this namespace

constexpr uint32_t NO_RANK = 0xFFFFFFFFu;                   // grank[d] of a doc whose group is SS_NO_GROUP
constexpr uint32_t EXTRA_SLOTS = 2;                         // behind a row's n_groups counters: the matches, the SS_NO_GROUP matches
constexpr uint32_t MAX_LDS_GROUPS = 8192;                   // the LDS histogram's counters: 32 KB beside the 4 KB image and 2 KB of cursors
constexpr int64_t DEFAULT_LDS_GROUPS = 8192;                // option "gtopk.lds_groups"
constexpr uint64_t DEFAULT_SCRATCH_BYTES = 256ull << 20;    // option "gtopk.scratch_bytes"

// ---- the key.  Groups sort by count descending, equal counts by rank ascending (rank ascending is value ascending): one unsigned key,
// ascending.  A count is at least 1, so no key is mset::PAD_KEY.
constexpr uint64_t pack_key(uint32_t count, uint32_t rank) { return (uint64_t)(0xFFFFFFFFu - count) << 32 | rank; }
constexpr uint32_t key_count(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key >> 32); }
constexpr uint32_t key_rank(uint64_t key) { return (uint32_t)key; }
constexpr uint32_t buffer_lds_bytes(uint32_t K) { return mset::buffer_entries(K) * (uint32_t)sizeof(uint64_t); }

// ---- the path.  The LDS histogram when the table has at most `option` distinct values (0 or less: never) and they fit the histogram.
constexpr bool use_lds(uint32_t n_groups, int64_t option) {
    return option > 0 && (int64_t)n_groups <= option && n_groups <= MAX_LDS_GROUPS;
}
constexpr uint32_t hist_lds_bytes(uint32_t n_groups) { return ((n_groups + 3u) & ~3u) * (uint32_t)sizeof(uint32_t); }

// ---- the counter row of a query: n_groups counters, the two extra slots, padded to whole 16-byte loads (rows then start aligned)
constexpr uint64_t row_stride(uint32_t n_groups) { return ((uint64_t)n_groups + EXTRA_SLOTS + 3u) & ~(uint64_t)3u; }
constexpr uint64_t slot_match(uint32_t n_groups) { return n_groups; }
constexpr uint64_t slot_ungrouped(uint32_t n_groups) { return (uint64_t)n_groups + 1; }

// ---- groups.  As many queries as have their rows inside scratch_bytes, at least one (a row larger than the bound goes alone), at most
// n_active and MAX_GRID.
constexpr uint64_t scratch_bytes_of(int64_t option) { return option < 1 ? DEFAULT_SCRATCH_BYTES : (uint64_t)option; }
constexpr uint32_t group_queries(uint64_t n_active, uint32_t n_groups, uint64_t scratch_bytes) {
    uint64_t g = scratch_bytes / (row_stride(n_groups) * sizeof(uint32_t));
    if (g < 1) g = 1;
    if (g > mset::MAX_GRID) g = mset::MAX_GRID;
    if (g > n_active) g = n_active;
    return (uint32_t)g;
}

// ---- the call's own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code)
inline int check_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_groups_out, bool has_n_out, int32_t first,
                      int32_t m, bool has_table) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return mset::INVALID; }
    if (n_q == 0) return mset::OK;                  // an empty batch is SS_OK whatever the other arguments say: nothing is read
    if (m < 1 || first < 0) { std::snprintf(msg, cap, "%s: m = %d must be >= 1 and first = %d >= 0", entry, m, first); return mset::INVALID; }
    if ((int64_t)first + (int64_t)m > (int64_t)mset::MAX_K) {
        std::snprintf(msg, cap, "%s: first + m = %lld exceeds SS_MAX_TOPK = %d", entry, (long long)first + (long long)m, mset::MAX_K);
        return mset::UNSUPPORTED;
    }
    if (!has_q_ptr || !has_groups_out || !has_n_out) { std::snprintf(msg, cap, "%s: q_ptr, groups_out or n_out is NULL", entry); return mset::INVALID; }
    if (!has_table) { std::snprintf(msg, cap, "%s: no group table registered (ss_scorer_set_doc_groups)", entry); return mset::STATE; }
    return mset::OK;
}

}  // namespace gtopk
}  // namespace ss
