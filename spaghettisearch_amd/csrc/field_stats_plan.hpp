// field_stats_plan.hpp — the part of ss_field_stats and ss_field_histogram (field_stats.hip) that needs no device and is
// the calls' own: the checks of their arguments with their messages, the bin of a value (the exact divider for a fixed width, the search
// over explicit edges), the choice between the two counting paths, the stride of a query's counter row, the bytes of a query's partial
// entries and how many queries fit the scratch bound.  The blocks, runs, groups and launches are match_set_plan.hpp's.  The constexpr
// functions are compiled for both sides (the kernels call them; tests/field_stats_plan_harness.cpp runs them on the host under
// ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include "match_set_plan.hpp"

#include <cstdio>

namespace ss {
namespace fstats {

using namespace mset;                              // the shared names stay reachable under this namespace

constexpr int64_t NO_VALUE = INT64_MIN;                     // SS_NO_FIELD_VALUE: in these two calls, "the doc has no value"
constexpr int32_t MAX_STAT_FIELDS = 4;                      // SS_MAX_DOC_FIELDS (field_stats.hip asserts the equality)
constexpr int32_t MAX_HIST_BINS = 65536;                    // SS_MAX_HIST_BINS (likewise)
constexpr uint32_t STAT_BYTES = 40;                         // sizeof(ss_field_stat) (likewise)
constexpr uint32_t TAIL_SLOTS = 4;                          // behind a row's n_bins counters: below, above, missing, matches (ss_hist_tail's order)
constexpr uint32_t MAX_LDS_BINS = 8192;                     // the LDS histogram's counters: 32 KB beside the 4 KB image and 2 KB of cursors
constexpr int64_t DEFAULT_LDS_BINS = 8192;                  // option "fstats.lds_bins"
constexpr uint32_t MAX_LDS_EDGES = 1025;                    // most edges (n_bins + 1) copied to LDS beside the histogram: 8200 bytes
constexpr uint64_t DEFAULT_SCRATCH_BYTES = 256ull << 20;    // option "fstats.scratch_bytes"

// ---- the divider.  u / width for every 64-bit u and every width >= 1 without a hardware divide: a shift when the width is a power of
// two; otherwise magic = floor(2^64 / width) (= floor((2^64 - 1) / width), as no such width divides 2^64), q = the high 64 bits of
// u * magic, which is the quotient or one less (u * magic / 2^64 lies in (u / width - 1, u / width]), and one fix-up by the remainder.
constexpr uint64_t mul_hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
struct Divider {
    uint64_t width, magic;            // magic: 0 for a power of two
    uint32_t shift;                   // log2(width) for a power of two
};
constexpr Divider make_divider(uint64_t width) {
    Divider d{width, 0, 0};
    if ((width & (width - 1)) == 0) {
        while (d.shift < 63 && (1ull << d.shift) < width) d.shift++;
    } else {
        d.magic = ~0ull / width;
    }
    return d;
}
enum { DIV_ANY = 0, DIV_SHIFT = 1, DIV_RECIPROCAL = 2, DIV_PLAIN = 3 };   // which form a caller compiles in (DIV_ANY: by the divider's magic)
constexpr int divider_kind(const Divider& d) { return d.magic == 0 ? DIV_SHIFT : DIV_RECIPROCAL; }
template <int KIND = DIV_ANY>
constexpr uint64_t divide(const Divider& d, uint64_t u) {
    if (KIND == DIV_PLAIN) return u / d.width;
    if (KIND == DIV_SHIFT || (KIND == DIV_ANY && d.magic == 0)) return u >> d.shift;
    uint64_t q = mul_hi(u, d.magic);
    if (u - q * d.width >= d.width) q++;            // (q * width <= u: no wrap)
    return q;
}

// ---- the bin of a value.  A slot of the query's counter row: [0, n_bins) a bin, then below, above, missing (and the matches, which
// no value maps to).  span = n_bins * width; when that is 2^64 or more no value is above (sat).
constexpr uint32_t slot_below(uint32_t n_bins) { return n_bins; }
constexpr uint32_t slot_above(uint32_t n_bins) { return n_bins + 1; }
constexpr uint32_t slot_missing(uint32_t n_bins) { return n_bins + 2; }
constexpr uint32_t slot_match(uint32_t n_bins) { return n_bins + 3; }
struct Binner {
    int64_t origin;
    Divider div;
    uint64_t span;                    // n_bins * width, 2^64 - 1 when sat
    uint32_t n_bins;
    bool sat;
};
constexpr Binner make_binner(int64_t origin, uint64_t width, uint32_t n_bins) {
    const unsigned __int128 span = (unsigned __int128)n_bins * width;
    const bool sat = (span >> 64) != 0;
    return Binner{origin, make_divider(width), sat ? ~0ull : (uint64_t)span, n_bins, sat};
}
// KIND: DIV_PLAIN is the quotient by `/` (option "fstats.plain_divide", and what the harness compares the divider with)
template <int KIND = DIV_ANY>
constexpr uint32_t bin_fixed(const Binner& b, int64_t v) {
    if (v == NO_VALUE) return slot_missing(b.n_bins);
    if (v < b.origin) return slot_below(b.n_bins);
    const uint64_t u = (uint64_t)v - (uint64_t)b.origin;
    if (!b.sat && u >= b.span) return slot_above(b.n_bins);
    const uint64_t q = divide<KIND>(b.div, u);
    return q >= b.n_bins ? slot_above(b.n_bins) : (uint32_t)q;      // (only when sat: below the span the quotient is a bin)
}
// edges [n_bins + 1], strictly ascending: bin b is edges[b] <= v < edges[b + 1]
template <typename Edges>
constexpr uint32_t bin_edges(const Edges& edges, uint32_t n_bins, int64_t v) {
    if (v == NO_VALUE) return slot_missing(n_bins);
    if (v < edges[0]) return slot_below(n_bins);
    if (v >= edges[n_bins]) return slot_above(n_bins);
    uint32_t lo = 0, hi = n_bins;                   // edges[lo] <= v < edges[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (edges[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}
inline bool edges_ascending(const int64_t* edges, uint32_t n_bins) {
    for (uint32_t i = 0; i < n_bins; i++)
        if (!(edges[i] < edges[i + 1])) return false;
    return true;
}

// ---- the path.  The LDS histogram when n_bins is at most `option` (0 or less: never) and fits the histogram; the edges beside it when
// they are few.
constexpr bool use_lds(uint32_t n_bins, int64_t option) { return option > 0 && (int64_t)n_bins <= option && n_bins <= MAX_LDS_BINS; }
constexpr uint32_t hist_lds_bytes(uint32_t n_bins) { return ((n_bins + 3u) & ~3u) * (uint32_t)sizeof(uint32_t); }
constexpr bool edges_in_lds(uint32_t n_bins) { return n_bins + 1 <= MAX_LDS_EDGES; }
constexpr uint32_t edges_lds_bytes(uint32_t n_bins) { return edges_in_lds(n_bins) ? (n_bins + 1) * (uint32_t)sizeof(int64_t) : 0u; }

// ---- the counter row of a query: n_bins counters, the four extra slots, padded to whole 16-byte loads
constexpr uint64_t row_stride(uint32_t n_bins) { return ((uint64_t)n_bins + TAIL_SLOTS + 3u) & ~(uint64_t)3u; }

// ---- groups.  As many queries as have their counter rows (histogram) or their R x n_stat_fields partial entries (stats) inside
// scratch_bytes, at least one, at most n_active and MAX_GRID.
constexpr uint64_t scratch_bytes_of(int64_t option) { return option < 1 ? DEFAULT_SCRATCH_BYTES : (uint64_t)option; }
constexpr uint64_t hist_query_bytes(uint32_t n_bins) { return row_stride(n_bins) * sizeof(uint32_t); }
constexpr uint64_t stats_query_bytes(uint32_t R, uint32_t n_stat_fields) { return (uint64_t)(R ? R : 1) * (n_stat_fields ? n_stat_fields : 1) * STAT_BYTES; }
constexpr uint32_t group_queries(uint64_t n_active, uint64_t query_bytes, uint64_t scratch_bytes) {
    uint64_t g = scratch_bytes / query_bytes;
    if (g < 1) g = 1;
    if (g > mset::MAX_GRID) g = mset::MAX_GRID;
    if (g > n_active) g = n_active;
    return (uint32_t)g;
}

// ---- the calls' own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code).  fields: the
// host's copy, read only when everything before it has passed (NULL with has_fields: the counts alone are judged).
inline int check_stats_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_stats_out, int32_t n_stat_fields,
                            bool has_fields, const int32_t* fields, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return mset::INVALID; }
    if (n_q == 0) return mset::OK;                  // an empty batch is SS_OK whatever the other arguments say: nothing is read
    if (!has_q_ptr || !has_stats_out) { std::snprintf(msg, cap, "%s: q_ptr or stats_out is NULL", entry); return mset::INVALID; }
    if (n_stat_fields < 1 || !has_fields) { std::snprintf(msg, cap, "%s: n_stat_fields = %d must be >= 1 and fields not NULL", entry, n_stat_fields); return mset::INVALID; }
    if (n_stat_fields > MAX_STAT_FIELDS) {
        std::snprintf(msg, cap, "%s: n_stat_fields = %d exceeds SS_MAX_DOC_FIELDS = %d", entry, n_stat_fields, MAX_STAT_FIELDS);
        return mset::UNSUPPORTED;
    }
    if (n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return mset::STATE; }
    for (int32_t i = 0; fields && i < n_stat_fields; i++)
        if (fields[i] < 0 || fields[i] >= n_fields) {
            std::snprintf(msg, cap, "%s: fields[%d] = %d (the scorer has %d fields)", entry, i, fields[i], n_fields);
            return mset::INVALID;
        }
    return mset::OK;
}
// edges: the host's copy, read only when everything before it has passed (NULL with has_edges: the rest alone is judged)
inline int check_hist_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_counts_out, int32_t field, uint64_t width,
                           bool has_edges, const int64_t* edges, int32_t n_bins, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return mset::INVALID; }
    if (n_q == 0) return mset::OK;
    if (!has_q_ptr || !has_counts_out) { std::snprintf(msg, cap, "%s: q_ptr or counts_out is NULL", entry); return mset::INVALID; }
    if (n_bins < 1) { std::snprintf(msg, cap, "%s: n_bins = %d must be >= 1", entry, n_bins); return mset::INVALID; }
    if (n_bins > MAX_HIST_BINS) { std::snprintf(msg, cap, "%s: n_bins = %d exceeds SS_MAX_HIST_BINS = %d", entry, n_bins, MAX_HIST_BINS); return mset::UNSUPPORTED; }
    if (!has_edges && width == 0) { std::snprintf(msg, cap, "%s: width is 0 and edges is NULL", entry); return mset::INVALID; }
    if (n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return mset::STATE; }
    if (field < 0 || field >= n_fields) { std::snprintf(msg, cap, "%s: field %d (the scorer has %d fields)", entry, field, n_fields); return mset::INVALID; }
    if (edges && !edges_ascending(edges, (uint32_t)n_bins)) { std::snprintf(msg, cap, "%s: edges are not strictly ascending", entry); return mset::INVALID; }
    return mset::OK;
}

}  // namespace fstats
}  // namespace ss
