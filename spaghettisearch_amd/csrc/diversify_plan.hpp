// diversify_plan.hpp — the part of ss_diversify_hits (diversify.hip) that needs no device: the pitch of a window's Gram
// matrix, the walk over its upper tile triangle, how many queries share the Gram scratch, the launches that cover a call, the checks
// of the weights, and the 64-bit key that makes one block arg-max choose the largest value and then the smallest window index.  The
// constexpr functions are compiled for both sides (the kernels call them; tests/diversify_plan_harness.cpp runs them on the host under
// ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ss {
namespace divp {

enum { OK = 0, INVALID = 1 };                             // what a check returns; diversify.hip maps them to the ABI's codes
constexpr uint32_t TILE = 64;                             // a wave of k_div_gram owns TILE x TILE entries
constexpr int32_t WEIGHT_MAX = 65536;                     // SS_DIV_WEIGHT_MAX (diversify.hip asserts the equality)
constexpr uint32_t MAX_WINDOW = 1024;                     // SS_MAX_TOPK (likewise)
constexpr uint64_t DEFAULT_SCRATCH_BYTES = 256ull << 20;  // option "div.scratch_bytes"
constexpr uint32_t MAX_GROUP = 65535;                     // queries of one launch: the grid's second dimension

// rows and columns of a query's Gram matrix: k_in rounded up to whole tiles
constexpr uint32_t pitch(uint32_t k_in) { return (k_in + TILE - 1) / TILE * TILE; }
// bytes of one query's Gram matrix (at most 4 MB)
constexpr uint64_t query_bytes(uint32_t k_in) { return (uint64_t)pitch(k_in) * pitch(k_in) * sizeof(int32_t); }
// tiles (ti, tj) with ti <= tj < n_tiles
constexpr uint32_t tile_pairs(uint32_t n_tiles) { return n_tiles * (n_tiles + 1) / 2; }

// pair number p < tile_pairs(n_tiles) -> (ti, tj), row by row of the upper triangle: (0,0) (0,1) .. (0,T-1) (1,1) ..
struct TilePair { uint32_t ti, tj; };
constexpr TilePair tile_of_pair(uint32_t p, uint32_t n_tiles) {
    uint32_t ti = 0;
    while (ti + 1 < n_tiles && p >= n_tiles - ti) {
        p -= n_tiles - ti;
        ti++;
    }
    return TilePair{ti, ti + p};
}

// value(j) = w_rel * rel - w_div * pen as the key of the arg-max.  |rel| and |pen| <= 2^24 and the weights <= 2^16, so |value| <= 2^41:
// value + 2^42 is positive and below 2^43; 1023 - j below it makes the larger key the larger value, then the smaller j.  No key is 0.
constexpr int64_t VALUE_BIAS = (int64_t)1 << 42;
constexpr int64_t value_of(int32_t w_rel, int32_t rel, int32_t w_div, int32_t pen) { return (int64_t)w_rel * rel - (int64_t)w_div * pen; }
constexpr uint64_t select_key(int64_t value, uint32_t j) { return (uint64_t)(value + VALUE_BIAS) << 10 | (uint64_t)(MAX_WINDOW - 1 - j); }
constexpr uint32_t key_row(uint64_t key) { return MAX_WINDOW - 1 - (uint32_t)(key & (MAX_WINDOW - 1)); }

// queries whose Gram matrices share the scratch: as many as fit into scratch_bytes, at least one, at most n_q and MAX_GROUP
inline uint32_t group_queries(uint64_t n_q, uint32_t k_in, uint64_t scratch_bytes) {
    uint64_t g = scratch_bytes / query_bytes(k_in);
    if (g < 1) g = 1;
    if (g > MAX_GROUP) g = MAX_GROUP;
    if (g > n_q) g = n_q;
    return (uint32_t)g;
}

// the launches of a call, in stream order: queries [first, first + count), every query once
struct Launch { uint32_t first, count; };
inline std::vector<Launch> launches(uint64_t n_q, uint32_t group) {
    std::vector<Launch> out;
    for (uint64_t q = 0; q < n_q; q += group) out.push_back(Launch{(uint32_t)q, (uint32_t)(n_q - q < group ? n_q - q : group)});
    return out;
}

// the weights (the paging checks are hit_window_plan.hpp's); the text of a refusal goes to msg
inline int check_weights(char* msg, size_t cap, const char* entry, int32_t w_rel, int32_t w_div) {
    if (w_rel < 0 || w_rel > WEIGHT_MAX || w_div < 0 || w_div > WEIGHT_MAX) {
        std::snprintf(msg, cap, "%s: w_rel = %d or w_div = %d outside 0 .. SS_DIV_WEIGHT_MAX = %d", entry, w_rel, w_div, WEIGHT_MAX);
        return INVALID;
    }
    return OK;
}
// the option's value: what the caller set, anything below 1 as the default
inline uint64_t scratch_bytes_of(int64_t option) { return option < 1 ? DEFAULT_SCRATCH_BYTES : (uint64_t)option; }

}  // namespace divp
}  // namespace ss
