// hit_window_plan.hpp — the host-only part of the calls that take a window of result rows (hits [n_q][k_in], n_hits [n_q]) and
// post-process it: ss_explain_hits, ss_best_passages, ss_collapse_hits, ss_score_topk_collapsed, ss_dedup_hits, ss_sort_hits_by_field,
// ss_hit_fields, ss_hit_vector_scores, ss_rerank_hits_by_vector, ss_diversify_hits.  The paging checks, the overlap test of hits and hits_out, the search
// for a host count outside the window, and the copy of exactly the entries a kernel wrote.  hit_window.hpp holds the HIP side.  No HIP
// call and no HIP header: tests/hit_window_plan_harness.cpp compiles this file alone (with a sanitizer).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace ss {
namespace hitwin {

constexpr int32_t OK = 0, INVALID = 1, UNSUPPORTED = 2;   // what a refusal is: the caller maps them to SS_ERR_INVALID / SS_ERR_UNSUPPORTED
constexpr size_t NONE = ~(size_t)0;

// The arguments of a paged call.  `window`: the name of the width argument ("k_in", "k_window"); `extra`: the name of one more argument
// that must be >= 1 ("g", "min_match"), NULL = there is none.  A refusal's text goes to msg.
inline int32_t check_paging(char* msg, size_t msg_cap, const char* entry, const char* window, int32_t max_topk, int32_t n_q, int32_t k_in,
                            int32_t k, int32_t first, const char* extra = nullptr, int32_t extra_v = 1) {
    if (n_q < 0) {
        std::snprintf(msg, msg_cap, "%s: n_q < 0", entry);
        return INVALID;
    }
    if (k_in < 1 || k < 1 || (extra && extra_v < 1) || first < 0) {
        if (extra)
            std::snprintf(msg, msg_cap, "%s: %s = %d, k = %d, %s = %d must be >= 1 and first = %d >= 0", entry, window, k_in, k, extra, extra_v, first);
        else std::snprintf(msg, msg_cap, "%s: %s = %d, k = %d must be >= 1 and first = %d >= 0", entry, window, k_in, k, first);
        return INVALID;
    }
    if (k_in > max_topk || k > max_topk) {
        std::snprintf(msg, msg_cap, "%s: %s = %d or k = %d exceeds SS_MAX_TOPK = %d", entry, window, k_in, k, max_topk);
        return UNSUPPORTED;
    }
    return OK;
}

// whether the byte ranges [in, in + in_bytes) and [out, out + out_bytes) share a byte (an output that starts where the input ends: no)
inline bool overlaps(const void* in, size_t in_bytes, const void* out, size_t out_bytes) {
    const uintptr_t ib = (uintptr_t)in, ie = ib + in_bytes, ob = (uintptr_t)out, oe = ob + out_bytes;
    return ib < oe && ob < ie;
}

// the first q with n_hits[q] outside 0 .. k_in, NONE if there is none
inline size_t first_bad_count(const int32_t* n_hits, size_t n_q, int32_t k_in) {
    for (size_t q = 0; q < n_q; q++)
        if (n_hits[q] < 0 || n_hits[q] > k_in) return q;
    return NONE;
}

// dst and src: [n_q][stride][inner_stride] elements of `elem` bytes.  Of query q the rows below counts[q] (clamped to 0 .. stride) were
// written, and of each such row the first inner_ptr[q + 1] - inner_ptr[q] elements (no more than inner_stride; inner_ptr NULL: all
// inner_stride).  Exactly those bytes are copied; no other byte of dst is touched.
inline void copy_written(void* dst, const void* src, size_t n_q, size_t stride, size_t elem, const int32_t* counts, size_t inner_stride = 1,
                         const uint32_t* inner_ptr = nullptr) {
    unsigned char* const d = static_cast<unsigned char*>(dst);
    const unsigned char* const s = static_cast<const unsigned char*>(src);
    for (size_t q = 0; q < n_q; q++) {
        const size_t cnt = counts[q] < 0 ? 0 : (size_t)counts[q] > stride ? stride : (size_t)counts[q];
        size_t inner = inner_stride;
        if (inner_ptr && inner_ptr[q + 1] - inner_ptr[q] < inner_stride) inner = inner_ptr[q + 1] - inner_ptr[q];
        if (!cnt || !inner) continue;
        const size_t o = q * stride * inner_stride * elem;
        if (inner == inner_stride) {                          // (whole rows: one run)
            std::memcpy(d + o, s + o, cnt * inner_stride * elem);
            continue;
        }
        for (size_t j = 0; j < cnt; j++) std::memcpy(d + o + j * inner_stride * elem, s + o + j * inner_stride * elem, inner * elem);
    }
}

}  // namespace hitwin
}  // namespace ss
