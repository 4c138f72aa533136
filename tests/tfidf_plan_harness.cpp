// tests/tfidf_plan_harness.cpp — spaghettisearch_amd/csrc/tfidf_plan.hpp on its own: host compiler, no device header, ASan + UBSan
// (built and run by tests/test_tfidf_plan_cpu.py).  Prints the geometry constants, then reads lines of
//   n_docs n_post blocks bucket_shift head_min_run bucket_min
// on stdin and prints every field of the plan for each, after checking the plan's invariants on it.
#include "tfidf_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>

using namespace ss::tfidf;

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            std::fprintf(stderr, "line %llu (%" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "): %s\n", line, n_docs, n_post, \
                         o.blocks, o.bucket_shift, o.head_min_run, o.bucket_min, #cond);                                     \
            return 1;                                                                                                        \
        }                                                                                                                    \
    } while (0)

int main() {
    std::printf("const CH %d SC_TPB %d SC_PT %d SC_CH %d SC_WIN %d SC_PF %d SC_BPT_MAX %d NB_MAX %d HEAD_CAP %d HEAD_LEVELS %d HEAD_PIECE %d\n", CH, SC_TPB,
                SC_PT, SC_CH, SC_WIN, SC_PF, SC_BPT_MAX, NB_MAX, HEAD_CAP, HEAD_LEVELS, HEAD_PIECE);
    const Options dflt;
    std::printf("default blocks %" PRId64 " bucket_shift %" PRId64 " head_min_run %" PRId64 " bucket_min %" PRId64 "\n", dflt.blocks, dflt.bucket_shift,
                dflt.head_min_run, dflt.bucket_min);
    uint64_t n_docs, n_post;
    Options o;
    unsigned long long line = 0;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &n_docs, &n_post, &o.blocks, &o.bucket_shift, &o.head_min_run,
                      &o.bucket_min) == 6) {
        line++;
        const Plan p = make_plan(n_docs, n_post, o);
        CHECK(p.shift >= 10 && p.shift <= 14 && (!p.shift_forced || p.shift == 14));
        CHECK((uint64_t)p.nb << p.shift >= n_docs && (p.nb <= 1 || (uint64_t)(p.nb - 1) << p.shift < n_docs));
        if (p.bucketed) {
            CHECK(n_post >= 1 && n_post < ((uint64_t)1 << 32) && p.nb <= (uint32_t)NB_MAX);
            CHECK(p.per > 0 && p.per % CH == 0 && p.per % SC_CH == 0);                      // whole chunks of both passes
            CHECK((uint64_t)p.nblk * p.per >= n_post && n_post > (uint64_t)(p.nblk - 1) * p.per);
            CHECK(p.bpt % 2 == 0 && (uint64_t)p.bpt * SC_TPB >= p.nb);
            CHECK(p.nbt % 2 == 0 && p.nbt >= p.nb && p.nbt <= p.nb + 1);
            CHECK(p.head_thr == 0 || p.head_thr > 2 * (uint64_t)SC_CH);                     // a head list is longer than two chunks of either
            CHECK(p.head_thr == 0 || p.head_thr > 2 * (uint64_t)CH);                        // pass (head_skip relies on it)
            CHECK(p.bpt_inst == 2 || p.bpt_inst == 4 || p.bpt_inst == SC_BPT_MAX);
            CHECK(p.too_many_buckets || (uint32_t)p.bpt_inst >= p.bpt);                     // the instance's cursor registers hold the thread's buckets
            CHECK(p.too_many_buckets == (p.bpt > (uint32_t)SC_BPT_MAX));
            CHECK(p.scatter_lds_bytes == scatter_lds_bytes(p.nbt) && p.bucket_lds_bytes == bucket_lds_bytes(p.shift));
        } else {
            CHECK(p.per == 0 && p.nblk == 0 && p.head_thr == 0 && p.bpt == 0 && p.nbt == 0 && p.bpt_inst == 0 && p.scatter_lds_bytes == 0 &&
                  p.bucket_lds_bytes == 0 && !p.too_many_buckets);
        }
        std::printf("%d %d %d %u %" PRIu64 " %u %" PRIu64 " %u %u %d %zu %zu %d\n", (int)p.bucketed, p.shift, (int)p.shift_forced, p.nb, p.per, p.nblk,
                    p.head_thr, p.bpt, p.nbt, p.bpt_inst, p.scatter_lds_bytes, p.bucket_lds_bytes, (int)p.too_many_buckets);
    }
    if (!std::feof(stdin)) {
        std::fprintf(stderr, "line %llu: not six integers\n", line + 1);
        return 1;
    }
    std::printf("ok %llu\n", line);
    return 0;
}
