// facet_plan.hpp — the part of ss_facet_counts (facet.hip) that needs no device and is the call's own: the checks of its
// arguments with their messages, the elementary intervals of the buckets' bounds and the interval-to-bucket map.  The doc-block and
// word arithmetic of k_facet_counts and the launches that cover a call are match_set_plan.hpp's.  The constexpr functions are compiled
// for both sides (the kernel calls them; tests/facet_plan_harness.cpp runs them on the host under ASan + UBSan).  Includes nothing of
// HIP.
//
// The match set of a query is never written out, so there is no scratch to budget and no grouping of queries: what a call needs
// beyond the allowed sets of the scoring path is its list table (16 bytes per posting list of the batch) and one BucketTable.
#pragma once
#include "match_set_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace ss {
namespace facetp {

using namespace mset;                              // the shared names stay reachable under this namespace

constexpr int32_t MAX_BUCKETS = 64;                         // SS_MAX_FACET_BUCKETS (facet.hip asserts the equality)
constexpr uint32_t MAX_CUTS = 2 * MAX_BUCKETS;              // a bucket adds at most two cuts to its field's axis
constexpr uint32_t MAX_FIELDS = 4;                          // SS_MAX_DOC_FIELDS (likewise)
constexpr uint32_t NO_INTERVAL = 0xFFFFFFFFu;

// a bucket as the ABI passes it: the layout of ss_doc_range (facet.hip asserts size and offsets)
struct Range { int32_t field, pad; int64_t lo, hi; };

// ---- the call's own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code)
inline int check_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_n_match, int32_t n_buckets, bool has_buckets,
                      bool has_bucket_out, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return mset::INVALID; }
    if (n_buckets < 0) { std::snprintf(msg, cap, "%s: n_buckets < 0", entry); return mset::INVALID; }
    if (n_buckets > MAX_BUCKETS) { std::snprintf(msg, cap, "%s: n_buckets %d > SS_MAX_FACET_BUCKETS %d", entry, n_buckets, MAX_BUCKETS); return mset::UNSUPPORTED; }
    if (n_q == 0) return mset::OK;
    if (!has_q_ptr || !has_n_match) { std::snprintf(msg, cap, "%s: q_ptr or n_match_out is NULL", entry); return mset::INVALID; }
    if (n_buckets > 0 && (!has_buckets || !has_bucket_out)) { std::snprintf(msg, cap, "%s: buckets or bucket_counts_out is NULL", entry); return mset::INVALID; }
    if (n_buckets > 0 && n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return mset::STATE; }
    return mset::OK;
}
inline int check_buckets(char* msg, size_t cap, const char* entry, const Range* buckets, int32_t n_buckets, int32_t n_fields) {
    for (int32_t b = 0; b < n_buckets; b++)
        if (buckets[b].field < 0 || buckets[b].field >= n_fields) {
            std::snprintf(msg, cap, "%s: bucket %d names field %d (the scorer has %d fields)", entry, b, buckets[b].field, n_fields);
            return mset::INVALID;
        }
    return mset::OK;
}

// ---- buckets -> elementary intervals
// The axis of a field is cut where a bucket of that field begins (at lo) and behind where it ends (at hi + 1, unless hi is
// INT64_MAX: nothing lies behind it).  Between two neighbouring cuts every bucket either holds all values or none, so a matched doc
// needs ONE search per field — the interval of its value — whatever the number of buckets, and a bucket's count is the sum of
// the intervals it spans.  Interval i of a field: [cuts[i], cuts[i + 1] - 1], the last one up to INT64_MAX; a value below the first
// cut is in no bucket.  The cuts of all fields stand in one array, field after field; interval numbers index that array.
struct BucketTable {
    int64_t cuts[MAX_CUTS];
    uint32_t field_begin[MAX_FIELDS + 1];       // the cuts of field f: [field_begin[f], field_begin[f + 1])
    uint32_t lo_idx[MAX_BUCKETS], hi_end[MAX_BUCKETS];   // bucket b = the intervals [lo_idx[b], hi_end[b]); lo > hi: none
    uint32_t n_cuts, n_buckets, field_mask, pad;          // field_mask bit f: a bucket with lo <= hi names field f
};

// the interval of value v among the cuts [b, e): the last cut <= v, NO_INTERVAL when v lies below them all
constexpr uint32_t interval_of(const int64_t* cuts, uint32_t b, uint32_t e, int64_t v) {
    const uint32_t b0 = b;
    while (b < e) {                              // upper bound: the first cut > v
        const uint32_t mid = b + ((e - b) >> 1);
        if (cuts[mid] <= v) b = mid + 1;
        else e = mid;
    }
    return b == b0 ? NO_INTERVAL : b - 1;
}

// n_buckets <= MAX_BUCKETS, every field in [0, MAX_FIELDS): check_args / check_buckets have seen to both
inline void build_bucket_table(const Range* buckets, int32_t n_buckets, BucketTable& t) {
    t = BucketTable{};
    t.n_buckets = (uint32_t)n_buckets;
    for (uint32_t f = 0; f < MAX_FIELDS; f++) {
        const uint32_t begin = t.field_begin[f] = t.n_cuts;
        for (int32_t b = 0; b < n_buckets; b++) {
            if ((uint32_t)buckets[b].field != f || buckets[b].lo > buckets[b].hi) continue;
            t.cuts[t.n_cuts++] = buckets[b].lo;
            if (buckets[b].hi != INT64_MAX) t.cuts[t.n_cuts++] = buckets[b].hi + 1;      // (no overflow: hi < INT64_MAX)
            t.field_mask |= 1u << f;
        }
        std::sort(t.cuts + begin, t.cuts + t.n_cuts);
        t.n_cuts = (uint32_t)(std::unique(t.cuts + begin, t.cuts + t.n_cuts) - t.cuts);
    }
    t.field_begin[MAX_FIELDS] = t.n_cuts;
    for (int32_t b = 0; b < n_buckets; b++) {
        if (buckets[b].lo > buckets[b].hi) continue;                                      // (lo_idx == hi_end == 0: no interval)
        const uint32_t f = (uint32_t)buckets[b].field;
        const int64_t* const fb = t.cuts + t.field_begin[f];
        const int64_t* const fe = t.cuts + t.field_begin[f + 1];
        t.lo_idx[b] = (uint32_t)(std::lower_bound(fb, fe, buckets[b].lo) - t.cuts);      // lo is a cut
        t.hi_end[b] = buckets[b].hi == INT64_MAX ? t.field_begin[f + 1] : (uint32_t)(std::lower_bound(fb, fe, buckets[b].hi + 1) - t.cuts);
    }
}

}  // namespace facetp
}  // namespace ss
