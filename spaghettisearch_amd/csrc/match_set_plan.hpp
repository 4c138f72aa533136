// match_set_plan.hpp — what the calls over a query's whole match set M(q) share and that needs no device (ss_facet_counts, ss_field_topk,
// ss_top_groups, ss_field_stats / ss_field_histogram; DESIGN.md "K4s–u shared match-set code"): the codes a check returns, the cut of the
// docs into 32768-doc blocks and of a query's blocks into runs, the groups of queries that share a scratch block, the launches that
// cover a grid, and the size and order of the running best-K.  facet_plan.hpp, field_topk_plan.hpp, group_topk_plan.hpp and
// field_stats_plan.hpp add what is their own.  The constexpr functions are compiled for both sides (match_set.hpp's device code calls
// them; the plan harnesses under tests/ run them on the host under ASan + UBSan).  Includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ss {
namespace mset {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2, STATE = 3 };   // what a check returns; match_set.hpp's plan_code maps them to the ABI's codes
constexpr uint32_t BLOCK_WORDS = 1024;                      // words of the doc image of one block (k_constraint_masks' block)
constexpr uint32_t BLOCK_DOCS = BLOCK_WORDS * 32;           // 32768 docs
constexpr uint32_t THREADS = 256;                           // threads of every match-set kernel
constexpr uint32_t WORDS_PER_THREAD = 4;                    // words of a thread (one 16-byte LDS / global load)
constexpr uint32_t MAX_LISTS = 128;                         // SS_MAX_QUERY_TERMS terms x 2 tables (match_set.hpp asserts the equality)
constexpr int32_t MAX_K = 1024;                             // SS_MAX_TOPK (likewise)
constexpr uint32_t MAX_GRID = 0x7FFFFFFFu;                  // workgroups of one launch
constexpr uint32_t MAX_AUTO_RUNS = 64;                      // most runs per query the plan chooses by itself (a forced R may go to n_blocks)
constexpr uint32_t WG_PER_CU = 64;                          // workgroups per compute unit the plan aims at (measured: DESIGN.md K4t)
static_assert(THREADS * WORDS_PER_THREAD == BLOCK_WORDS && THREADS == 2 * MAX_LISTS, "block geometry");

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

// ---- runs.  A query's blocks [0, n_blocks) are cut into R runs of consecutive blocks, one workgroup each.  The plan's own choice
// fills the device: WG_PER_CU workgroups per compute unit over all active queries, at most MAX_AUTO_RUNS (a merge reads R lists).
// forced > 0 (options "ftopk.runs", "gtopk.runs", "fstats.runs") replaces it.  Always 1 <= R <= n_blocks.
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

// ---- groups: the active queries [first, first + count) that share one scratch block; the groups of a call re-use it in stream order
struct Group { uint32_t first, count; };
inline std::vector<Group> groups(uint64_t n_active, uint32_t group) {
    std::vector<Group> out;
    for (uint64_t a = 0; group && a < n_active; a += group) out.push_back(Group{(uint32_t)a, (uint32_t)(n_active - a < group ? n_active - a : group)});
    return out;
}
// ---- launches, in stream order: the rows [first, first + count) of a grid of n_rows rows (doc blocks for ss_facet_counts, runs for
// the other two) times n_per_row queries each, at most MAX_GRID workgroups a launch
struct Launch { uint32_t first, count; };
inline std::vector<Launch> launches(uint32_t n_rows, uint32_t n_per_row) {
    std::vector<Launch> out;
    if (!n_rows || !n_per_row) return out;
    const uint32_t per = MAX_GRID / n_per_row < 1 ? 1u : MAX_GRID / n_per_row;
    for (uint32_t r = 0; r < n_rows; r += per) out.push_back(Launch{r, n_rows - r < per ? n_rows - r : per});
    return out;
}

// ---- the running best-K (match_set.hpp's BestK).  A workgroup keeps the K smallest entries seen so far plus what has arrived since
// the last compaction.  A thread that finds the buffer full keeps its candidate and waits for the compaction, so nothing is lost; the
// buffer must hold K entries and leave room for progress.  Entries: a power of two (the compaction is a bitonic sort), at least 2 K
// and 512.  An entry is a key, or a key and a doc id: (a, da) sorts before (b, db) by key_less.
constexpr uint32_t pow2_at_least(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
constexpr uint32_t buffer_entries(uint32_t K) {
    const uint32_t c = 2 * pow2_at_least(K);
    return c < 512 ? 512 : c;
}
constexpr bool key_less(uint64_t a, uint32_t da, uint64_t b, uint32_t db) { return a < b || (a == b && da < db); }
// the entry no candidate equals (the callers' keys see to that): it pads a sort and is the threshold that lets everything pass
constexpr uint64_t PAD_KEY = ~0ull;
constexpr uint32_t PAD_DOC = ~0u;

}  // namespace mset
}  // namespace ss
