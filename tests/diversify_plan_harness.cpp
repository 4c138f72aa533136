// diversify_plan_harness.cpp — drives spaghettisearch_amd/csrc/diversify_plan.hpp on the host (tests/test_diversify_cpu.py compiles it with
// -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   g n_q k_in scratch_option   -> "pitch query_bytes group n_launches covered first:count ..."  (covered: 1 if the launches hold every
//                                  query exactly once, in order, each of 1 .. group queries)
//   w w_rel w_div               -> the check's code (0 OK, 1 INVALID)
//   t n_tiles                   -> "n_pairs ti:tj ti:tj ..." for every pair number in order
//   k w_rel rel w_div pen j     -> "value key(hex) row"
// A last line "ok <n> lines" is printed at end of input.
#include "diversify_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

namespace dp = ss::divp;

int main() {
    char line[512];
    long n_lines = 0;
    while (std::fgets(line, sizeof(line), stdin)) {
        long long a = 0, b = 0, c = 0, d = 0, e = 0;
        if (line[0] == 'g' && std::sscanf(line + 1, "%lld %lld %lld", &a, &b, &c) == 3) {
            const uint64_t n_q = (uint64_t)a;
            const uint32_t k_in = (uint32_t)b;
            const uint32_t group = dp::group_queries(n_q, k_in, dp::scratch_bytes_of((int64_t)c));
            const std::vector<dp::Launch> ls = dp::launches(n_q, group);
            uint64_t next = 0;
            bool covered = true;
            for (const dp::Launch& l : ls) {
                covered = covered && l.first == next && l.count >= 1 && l.count <= group;
                next += l.count;
            }
            covered = covered && next == n_q;
            std::printf("%u %" PRIu64 " %u %zu %d", dp::pitch(k_in), dp::query_bytes(k_in), group, ls.size(), covered ? 1 : 0);
            for (const dp::Launch& l : ls) std::printf(" %u:%u", l.first, l.count);
            std::printf("\n");
        } else if (line[0] == 'w' && std::sscanf(line + 1, "%lld %lld", &a, &b) == 2) {
            char msg[256] = "";
            const int rc = dp::check_weights(msg, sizeof(msg), "harness", (int32_t)a, (int32_t)b);
            if ((rc != dp::OK) != (std::strlen(msg) > 0)) return 3;                // a refusal, and only a refusal, has a text
            std::printf("%d\n", rc);
        } else if (line[0] == 't' && std::sscanf(line + 1, "%lld", &a) == 1) {
            const uint32_t n_tiles = (uint32_t)a, n_pairs = dp::tile_pairs(n_tiles);
            std::printf("%u", n_pairs);
            for (uint32_t p = 0; p < n_pairs; p++) {
                const dp::TilePair tp = dp::tile_of_pair(p, n_tiles);
                std::printf(" %u:%u", tp.ti, tp.tj);
            }
            std::printf("\n");
        } else if (line[0] == 'k' && std::sscanf(line + 1, "%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) == 5) {
            const int64_t value = dp::value_of((int32_t)a, (int32_t)b, (int32_t)c, (int32_t)d);
            const uint64_t key = dp::select_key(value, (uint32_t)e);
            std::printf("%" PRId64 " %016" PRIx64 " %u\n", value, key, dp::key_row(key));
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
