// facet_plan.hpp — the part of ss_facet_counts (facet.hip) that needs no device: the checks of the call's own arguments
// with their messages, the elementary intervals of the buckets' bounds and the interval-to-bucket map, the doc-block and word
// arithmetic of k_facet_counts (last partial block and last partial word included) and the launches that cover a call.  The constexpr
// functions are compiled for both sides (the kernel calls them; tests/facet_plan_harness.cpp runs them on the host under
// ASan + UBSan).  Includes nothing of HIP.
//
// The match set of a query is never written out, so there is no scratch to budget and no grouping of queries: what a call needs
// beyond the allowed sets of the scoring path is its list table (16 bytes per posting list of the batch) and one BucketTable.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ss {
namespace facetp {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2, STATE = 3 };   // what a check returns; facet.hip maps them to the ABI's codes
constexpr uint32_t BLOCK_WORDS = 1024;                      // words of the doc image of one workgroup (k_constraint_masks' block)
constexpr uint32_t BLOCK_DOCS = BLOCK_WORDS * 32;           // 32768 docs
constexpr int32_t MAX_BUCKETS = 64;                         // SS_MAX_FACET_BUCKETS (facet.hip asserts the equality)
constexpr uint32_t MAX_CUTS = 2 * MAX_BUCKETS;              // a bucket adds at most two cuts to its field's axis
constexpr uint32_t MAX_FIELDS = 4;                          // SS_MAX_DOC_FIELDS (likewise)
constexpr uint32_t MAX_LISTS = 128;                         // SS_MAX_QUERY_TERMS terms x 2 tables (likewise)
constexpr uint32_t NO_INTERVAL = 0xFFFFFFFFu;
constexpr uint32_t MAX_GRID = 0x7FFFFFFFu;                  // workgroups of one launch

// a bucket as the ABI passes it: the layout of ss_doc_range (facet.hip asserts size and offsets)
struct Range { int32_t field, pad; int64_t lo, hi; };

// ---- geometry
constexpr uint64_t words(uint64_t n_docs) { return (n_docs + 31) / 32; }
constexpr uint32_t blocks(uint64_t n_docs) { return (uint32_t)((n_docs + BLOCK_DOCS - 1) / BLOCK_DOCS); }
// words of block `blk` that hold a doc below n_docs (BLOCK_WORDS for every block but the last, 0 past the end)
constexpr uint32_t block_words(uint32_t blk, uint64_t n_docs) {
    const uint64_t w0 = (uint64_t)blk * BLOCK_WORDS, nw = words(n_docs);
    return nw <= w0 ? 0u : nw - w0 < BLOCK_WORDS ? (uint32_t)(nw - w0) : BLOCK_WORDS;
}
// the bits of word w that stand for docs below n_docs: all ones, a low part in the last word, nothing past it
constexpr uint32_t word_valid(uint64_t w, uint64_t n_docs) {
    const uint64_t first = w * 32;
    return first >= n_docs ? 0u : n_docs - first >= 32 ? 0xFFFFFFFFu : (1u << (uint32_t)(n_docs - first)) - 1u;
}

// the launches of a call, in stream order: doc blocks [first, first + count) times every active query, at most MAX_GRID workgroups each
struct Launch { uint32_t first, count; };
inline std::vector<Launch> launches(uint32_t n_blocks, uint32_t n_active) {
    std::vector<Launch> out;
    if (!n_blocks || !n_active) return out;
    const uint32_t per = std::max<uint32_t>(1u, MAX_GRID / n_active);
    for (uint32_t b = 0; b < n_blocks; b += per) out.push_back(Launch{b, std::min(per, n_blocks - b)});
    return out;
}

// ---- the call's own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code)
inline int check_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_n_match, int32_t n_buckets, bool has_buckets,
                      bool has_bucket_out, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return INVALID; }
    if (n_buckets < 0) { std::snprintf(msg, cap, "%s: n_buckets < 0", entry); return INVALID; }
    if (n_buckets > MAX_BUCKETS) { std::snprintf(msg, cap, "%s: n_buckets %d > SS_MAX_FACET_BUCKETS %d", entry, n_buckets, MAX_BUCKETS); return UNSUPPORTED; }
    if (n_q == 0) return OK;
    if (!has_q_ptr || !has_n_match) { std::snprintf(msg, cap, "%s: q_ptr or n_match_out is NULL", entry); return INVALID; }
    if (n_buckets > 0 && (!has_buckets || !has_bucket_out)) { std::snprintf(msg, cap, "%s: buckets or bucket_counts_out is NULL", entry); return INVALID; }
    if (n_buckets > 0 && n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return STATE; }
    return OK;
}
inline int check_buckets(char* msg, size_t cap, const char* entry, const Range* buckets, int32_t n_buckets, int32_t n_fields) {
    for (int32_t b = 0; b < n_buckets; b++)
        if (buckets[b].field < 0 || buckets[b].field >= n_fields) {
            std::snprintf(msg, cap, "%s: bucket %d names field %d (the scorer has %d fields)", entry, b, buckets[b].field, n_fields);
            return INVALID;
        }
    return OK;
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
