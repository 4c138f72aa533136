// field_topk_plan.hpp — the part of ss_field_topk (field_topk.hip) that needs no device: the checks of the call's own
// arguments with their messages, the key that orders docs by a field value, the runs a query's doc blocks are cut into and how many
// of them a query gets, the size of the candidate buffer, the groups of queries that share the partial lists, and the launches that
// cover a group.  The constexpr functions are compiled for both sides (the kernels call them; tests/field_topk_plan_harness.cpp runs
// them on the host under ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ss {
namespace ftopk {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2, STATE = 3 };   // what a check returns; field_topk.hip maps them to the ABI's codes
constexpr uint32_t BLOCK_WORDS = 1024;                      // words of the doc image of one block (k_facet_counts' block)
constexpr uint32_t BLOCK_DOCS = BLOCK_WORDS * 32;           // 32768 docs
constexpr uint32_t THREADS = 256;                           // threads of both kernels
constexpr int32_t MAX_K = 1024;                             // SS_MAX_TOPK (field_topk.hip asserts the equality)
constexpr uint32_t MAX_LISTS = 128;                         // SS_MAX_QUERY_TERMS terms x 2 tables (likewise)
constexpr uint32_t MAX_GRID = 0x7FFFFFFFu;                  // workgroups of one launch
constexpr uint32_t MAX_AUTO_RUNS = 64;                      // most runs per query the plan chooses by itself (a forced R may go to n_blocks)
constexpr uint32_t WG_PER_CU = 64;                          // workgroups per compute unit the plan aims at (measured: DESIGN.md K4t)
constexpr uint64_t DEFAULT_SCRATCH_BYTES = 256ull << 20;    // option "ftopk.scratch_bytes"
constexpr uint64_t ENTRY_BYTES = 12;                        // a partial entry: 8 bytes of key, 4 of doc id
constexpr uint64_t RUN_BYTES = 8;                           // per run: its match count and the length of its list

// ---- geometry (facet_plan.hpp's, restated: the two calls cut the docs alike)
constexpr uint32_t blocks(uint64_t n_docs) { return (uint32_t)((n_docs + BLOCK_DOCS - 1) / BLOCK_DOCS); }
constexpr uint32_t word_valid(uint64_t w, uint64_t n_docs) {
    const uint64_t first = w * 32;
    return first >= n_docs ? 0u : n_docs - first >= 32 ? 0xFFFFFFFFu : (1u << (uint32_t)(n_docs - first)) - 1u;
}

// ---- the key.  A doc sorts by (vkey, doc) ascending, both unsigned: vkey = the value with its sign bit flipped (signed order becomes
// unsigned order), complemented for descending (unsigned order reversed, no overflow at either end); the doc id is never complemented,
// so docs of equal value come in ascending doc id in both directions.
constexpr uint64_t SIGN = 0x8000000000000000ull;
constexpr uint64_t value_key(int64_t value, bool descending) {
    const uint64_t u = (uint64_t)value ^ SIGN;
    return descending ? ~u : u;
}
constexpr int64_t key_value(uint64_t vkey, bool descending) { return (int64_t)((descending ? ~vkey : vkey) ^ SIGN); }
// (a, da) sorts before (b, db)
constexpr bool key_less(uint64_t a, uint32_t da, uint64_t b, uint32_t db) { return a < b || (a == b && da < db); }
// the key no doc has (a doc id is below 2^32 - 1): it pads a sort and is the threshold that lets everything pass
constexpr uint64_t PAD_KEY = ~0ull;
constexpr uint32_t PAD_DOC = ~0u;

// ---- the candidate buffer.  A workgroup keeps the K = first + k smallest keys seen so far plus what has arrived since the last
// compaction.  A thread that finds the buffer full keeps its candidate and waits for the compaction, so nothing is lost; the buffer
// must hold K keys and leave room for progress.  Entries: a power of two (the compaction is a bitonic sort), at least 2 K and 512.
constexpr uint32_t pow2_at_least(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
constexpr uint32_t buffer_entries(uint32_t K) {
    const uint32_t c = 2 * pow2_at_least(K);
    return c < 512 ? 512 : c;
}
constexpr uint32_t buffer_lds_bytes(uint32_t K) { return buffer_entries(K) * (uint32_t)ENTRY_BYTES; }

// ---- runs.  A query's blocks [0, n_blocks) are cut into R runs of consecutive blocks, one workgroup each.  The plan's own choice
// fills the device: WG_PER_CU workgroups per compute unit over all active queries, at most MAX_AUTO_RUNS (the merge reads R lists).
// forced > 0 (option "ftopk.runs") replaces it.  Always 1 <= R <= n_blocks.
constexpr uint32_t runs_per_query(uint32_t n_blocks, uint64_t n_active, uint32_t n_cu, int64_t forced) {
    if (n_blocks == 0) return 0;
    uint64_t r = 0;
    if (forced > 0) r = (uint64_t)forced;
    else {
        const uint64_t want = (uint64_t)WG_PER_CU * (n_cu ? n_cu : 1), act = n_active ? n_active : 1;
        r = (want + act - 1) / act;
        if (r > MAX_AUTO_RUNS) r = MAX_AUTO_RUNS;
    }
    if (r < 1) r = 1;
    if (r > n_blocks) r = n_blocks;
    return (uint32_t)r;
}
// run r of R covers the blocks [run_begin(r), run_begin(r + 1)): never empty for R <= n_blocks, and the runs tile [0, n_blocks)
constexpr uint32_t run_begin(uint32_t r, uint32_t R, uint32_t n_blocks) { return (uint32_t)((uint64_t)r * n_blocks / R); }

// ---- groups.  The partial lists of a group of queries are [group][R][K] entries plus RUN_BYTES per run; the groups of a call re-use
// one scratch block in stream order.  As many queries as fit into scratch_bytes, at least one, at most n_active and MAX_GRID.
constexpr uint64_t query_bytes(uint32_t R, uint32_t K) { return (uint64_t)R * ((uint64_t)K * ENTRY_BYTES + RUN_BYTES); }
constexpr uint64_t scratch_bytes_of(int64_t option) { return option < 1 ? DEFAULT_SCRATCH_BYTES : (uint64_t)option; }
constexpr uint32_t group_queries(uint64_t n_active, uint32_t R, uint32_t K, uint64_t scratch_bytes) {
    uint64_t g = scratch_bytes / query_bytes(R ? R : 1, K ? K : 1);
    if (g < 1) g = 1;
    if (g > MAX_GRID) g = MAX_GRID;
    if (g > n_active) g = n_active;
    return (uint32_t)g;
}
struct Group { uint32_t first, count; };                    // active queries [first, first + count)
inline std::vector<Group> groups(uint64_t n_active, uint32_t group) {
    std::vector<Group> out;
    for (uint64_t a = 0; group && a < n_active; a += group) out.push_back(Group{(uint32_t)a, (uint32_t)(n_active - a < group ? n_active - a : group)});
    return out;
}
// the selection launches of one group, in stream order: runs [first, first + count) times the group's queries, at most MAX_GRID
// workgroups each
struct Launch { uint32_t first, count; };
inline std::vector<Launch> launches(uint32_t R, uint32_t n_group) {
    std::vector<Launch> out;
    if (!R || !n_group) return out;
    const uint32_t per = MAX_GRID / n_group < 1 ? 1u : MAX_GRID / n_group;
    for (uint32_t r = 0; r < R; r += per) out.push_back(Launch{r, R - r < per ? R - r : per});
    return out;
}

// ---- the call's own arguments (the query, mask, constraint and range arrays are checked by the scoring path's code)
inline int check_args(char* msg, size_t cap, const char* entry, int32_t n_q, bool has_q_ptr, bool has_docs_out, bool has_n_out, int32_t field,
                      int32_t first, int32_t k, int32_t n_fields) {
    if (n_q < 0) { std::snprintf(msg, cap, "%s: n_q < 0", entry); return INVALID; }
    if (n_q == 0) return OK;                        // an empty batch is SS_OK whatever the other arguments say: nothing is read
    if (k < 1 || first < 0) { std::snprintf(msg, cap, "%s: k = %d must be >= 1 and first = %d >= 0", entry, k, first); return INVALID; }
    if ((int64_t)first + (int64_t)k > (int64_t)MAX_K) {
        std::snprintf(msg, cap, "%s: first + k = %lld exceeds SS_MAX_TOPK = %d (a deeper page: a range clause on the last value seen)", entry,
                      (long long)first + (long long)k, MAX_K);
        return UNSUPPORTED;
    }
    if (!has_q_ptr || !has_docs_out || !has_n_out) { std::snprintf(msg, cap, "%s: q_ptr, docs_out or n_out is NULL", entry); return INVALID; }
    if (n_fields == 0) { std::snprintf(msg, cap, "%s: no field table registered (ss_scorer_set_doc_fields)", entry); return STATE; }
    if (field < 0 || field >= n_fields) { std::snprintf(msg, cap, "%s: field %d (the scorer has %d fields)", entry, field, n_fields); return INVALID; }
    return OK;
}

}  // namespace ftopk
}  // namespace ss
