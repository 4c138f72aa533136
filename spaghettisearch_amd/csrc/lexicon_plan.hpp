// lexicon_plan.hpp — the host-only part of the term lexicon (lexicon.hip): validation of the pointer arrays, the sort
// order of the words, and the layout the suggest kernel reads — term ids grouped by word length, the words of a group re-packed at
// one fixed stride.  No HIP call and no HIP header: tests/lexicon_plan_harness.cpp compiles this file alone (with a sanitizer).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ss {
namespace lex {

constexpr uint32_t MAX_WORD = 64;                 // SS_MAX_WORD_BYTES: longer words are listed by prefix, never suggested
constexpr uint32_t N_GROUPS = MAX_WORD + 1;       // lengths 0 .. 64
constexpr uint32_t N_STARTS = N_GROUPS + 1;       // start[L] for L = 0 .. 64, start[65] = number of grouped words

// word_ptr [n + 1]: starts at 0 and never decreases
inline bool word_ptr_ok(const uint64_t* ptr, uint64_t n) {
    if (ptr[0] != 0) return false;
    for (uint64_t t = 0; t < n; t++)
        if (ptr[t + 1] < ptr[t]) return false;
    return true;
}
// a pointer array of a call (p_ptr / w_ptr, [n + 1]): never decreases; it may start anywhere, as q_ptr of ss_score_topk may
inline bool call_ptr_ok(const uint32_t* ptr, uint64_t n) {
    for (uint64_t q = 0; q < n; q++)
        if (ptr[q + 1] < ptr[q]) return false;
    return true;
}

// words as arrays of UNSIGNED bytes, lexicographically, a proper prefix first (memcmp compares unsigned char); equal words by id
inline bool word_before(const uint8_t* bytes, const uint64_t* ptr, uint32_t a, uint32_t b) {
    const uint64_t la = ptr[a + 1] - ptr[a], lb = ptr[b + 1] - ptr[b];
    const uint64_t n = la < lb ? la : lb;
    const int c = n ? std::memcmp(bytes + ptr[a], bytes + ptr[b], (size_t)n) : 0;
    if (c != 0) return c < 0;
    if (la != lb) return la < lb;
    return a < b;
}
inline void build_order(uint64_t n, const uint64_t* ptr, const uint8_t* bytes, std::vector<uint32_t>& order) {
    order.resize((size_t)n);
    for (uint64_t t = 0; t < n; t++) order[(size_t)t] = (uint32_t)t;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return word_before(bytes, ptr, a, b); });
}

inline uint32_t stride_words(uint32_t len) { return (len + 3u) >> 2; }   // dwords a word of `len` bytes takes in its group

// The grouped layout: gterm = the ids of the words of at most MAX_WORD bytes ordered by (length, id); start[L] = the first grouped
// index of length L; base[L] = the dword at which group L's words begin in gwords, each word zero-padded to stride_words(L) dwords
// (little-endian: byte i of a word is bits 8 * (i & 3) of its dword i >> 2); base[65] = the dwords in all.
struct Groups {
    std::vector<uint32_t> gterm, gwords;
    uint32_t start[N_STARTS];
    uint64_t base[N_STARTS];
};
inline void build_groups(uint64_t n, const uint64_t* ptr, const uint8_t* bytes, Groups& g) {
    uint64_t count[N_GROUPS] = {};
    for (uint64_t t = 0; t < n; t++) {
        const uint64_t len = ptr[t + 1] - ptr[t];
        if (len <= MAX_WORD) count[len]++;
    }
    uint64_t at = 0, dw = 0;
    for (uint32_t L = 0; L < N_GROUPS; L++) {
        g.start[L] = (uint32_t)at;
        g.base[L] = dw;
        at += count[L];
        dw += count[L] * stride_words(L);
    }
    g.start[N_GROUPS] = (uint32_t)at;
    g.base[N_GROUPS] = dw;
    g.gterm.assign((size_t)at, 0u);
    g.gwords.assign((size_t)dw, 0u);
    uint64_t fill[N_GROUPS] = {};
    for (uint64_t t = 0; t < n; t++) {                    // ascending id: a group's ids ascend
        const uint64_t len = ptr[t + 1] - ptr[t];
        if (len > MAX_WORD) continue;
        const uint64_t i = fill[len]++;
        g.gterm[(size_t)(g.start[len] + i)] = (uint32_t)t;
        if (len) std::memcpy(reinterpret_cast<uint8_t*>(g.gwords.data() + g.base[len] + i * stride_words((uint32_t)len)), bytes + ptr[t], (size_t)len);
    }
}

// the grouped indices [lo, hi) a query word of `len` bytes is compared with at `max_dist`: the groups len - max_dist .. len + max_dist
inline void suggest_range(const uint32_t* start, uint64_t len, uint32_t max_dist, uint32_t* lo, uint32_t* hi) {
    if (len > MAX_WORD) { *lo = *hi = 0; return; }
    const uint32_t l0 = (uint32_t)len > max_dist ? (uint32_t)len - max_dist : 0u;
    const uint32_t l1 = std::min((uint32_t)len + max_dist, MAX_WORD);
    *lo = start[l0];
    *hi = start[l1 + 1];
}
inline uint64_t n_chunks(uint32_t lo, uint32_t hi, uint32_t chunk) { return ((uint64_t)(hi - lo) + chunk - 1) / chunk; }

// ---- completions (ss_lexicon_complete): the range [lb, ub) of sort positions of every prefix of a call is cut into the same number
// P of near-equal parts, one wave each.  P comes from the number of prefixes alone (the ranges are known on the device only): about
// COMPLETE_WAVES waves per call, so 1024 prefixes make a few thousand waves, and at most DEFAULT_COMPLETE_PARTS parts for a few
// prefixes: more parts stream a long range faster but make the merge of a short one slower (measured: DESIGN.md K4k).
#if defined(__HIPCC__)
#define SS_LEX_HD __host__ __device__
#else
#define SS_LEX_HD
#endif
constexpr uint32_t MAX_COMPLETE_PARTS = 256;
constexpr uint32_t DEFAULT_COMPLETE_PARTS = 64;
constexpr uint64_t COMPLETE_WAVES = 4096;
// forced = option "lexicon.complete_parts": a value in 1 .. MAX_COMPLETE_PARTS is taken as it is, any other means "from n_q"
SS_LEX_HD inline uint32_t complete_parts(uint64_t n_q, int64_t forced) {
    if (forced >= 1 && forced <= (int64_t)MAX_COMPLETE_PARTS) return (uint32_t)forced;
    const uint64_t p = n_q ? COMPLETE_WAVES / n_q : DEFAULT_COMPLETE_PARTS;
    return p < 1 ? 1u : p > DEFAULT_COMPLETE_PARTS ? DEFAULT_COMPLETE_PARTS : (uint32_t)p;
}
// part `part` of P covers positions [*begin, *end) of [lb, ub): the parts tile the range in order, their lengths differ by at most
// one (len < 2^32 and part <= 256: the products stay below 2^41)
SS_LEX_HD inline void complete_part(uint32_t lb, uint32_t ub, uint32_t P, uint32_t part, uint32_t* begin, uint32_t* end) {
    const uint64_t len = ub - lb;
    *begin = lb + (uint32_t)(len * part / P);
    *end = lb + (uint32_t)(len * (part + 1) / P);
}

}  // namespace lex
}  // namespace ss
