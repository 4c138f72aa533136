// links_plan.hpp — the host-only part of ss_graph_top_links / ss_graph_hit_links (links.hip): the option values as
// the kernels use them and the sizes of the call's temporaries, from what the host knows without asking the device — the number of
// requested rows, m, and the largest degree of the direction.  Row lengths themselves stay on the device: the split is planned
// there (k_links_count, k_links_scan).  No HIP call and no HIP header: tests/links_plan_harness.cpp compiles this file alone (with
// a sanitizer).
#pragma once

#include <cstdint>

namespace ss {
namespace links {

constexpr int64_t WAVE_MAX_DEFAULT = 1024, CHUNK_DEFAULT = 1024;   // options "links.wave_max" / "links.chunk_edges" 
constexpr int64_t OPT_MIN = 32, OPT_MAX = 4096;                    // both options are clamped to this range
constexpr uint32_t LDS_ENTRY_BYTES = 12;                           // a staged edge: ordered key u64 + node id u32

inline uint32_t clamp_opt(int64_t v) { return (uint32_t)(v < OPT_MIN ? OPT_MIN : v > OPT_MAX ? OPT_MAX : v); }

struct Bounds {
    uint32_t wave_max = 0, chunk = 0;
    uint32_t lds_entries = 0;      // edges one select work item stages at most: max(wave_max, chunk)
    uint64_t items_per_row = 0;    // work items one requested row can become at most
    uint64_t items = 0;            // ... all rows: the partial winners take items * m ids
    bool too_large = false;        // items * m * 4 bytes does not fit 2^62: SS_ERR_OOM without asking the allocator
};

// A row of at most wave_max edges is one work item; a longer one is cut into ceil(len / chunk) items.
inline uint64_t items_of_row(uint64_t len, uint32_t wave_max, uint32_t chunk) {
    if (len == 0) return 0;
    if (len <= wave_max) return 1;
    return (len + chunk - 1) / chunk;
}

inline Bounds bounds(uint64_t n_rows, uint32_t m, uint64_t max_degree, int64_t opt_wave_max, int64_t opt_chunk) {
    Bounds b;
    b.wave_max = clamp_opt(opt_wave_max);
    b.chunk = clamp_opt(opt_chunk);
    b.lds_entries = b.wave_max > b.chunk ? b.wave_max : b.chunk;
    b.items_per_row = items_of_row(max_degree, b.wave_max, b.chunk);
    if (b.items_per_row == 0) b.items_per_row = 1;                  // (an edge-less graph: the blocks keep a size)
    // n_rows * m < 2^31 and items_per_row < 2^32 / 32 + 1: the product stays below 2^62 / 4 only if checked
    const uint64_t per_row_ids = b.items_per_row * (uint64_t)m;     // < 2^27 * 2^6 + ...: no overflow
    if (n_rows && per_row_ids > ((uint64_t)1 << 60) / n_rows) { b.too_large = true; return b; }
    b.items = n_rows * b.items_per_row;
    return b;
}

}  // namespace links
}  // namespace ss
