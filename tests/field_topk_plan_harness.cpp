// field_topk_plan_harness.cpp — drives spaghettisearch_amd/csrc/field_topk_plan.hpp on the host (tests/test_field_topk_cpu.py compiles
// it with -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   k value descending                     -> "vkey(hex) value_back"      (the key of a value and the value read back from the key)
//   c va da vb db descending               -> 1 if (va, doc da) sorts before (vb, doc db) by their keys, else 0
//   r n_blocks n_active n_cu forced        -> "R tiles begin ..."         (tiles: 1 if the R runs are non-empty and tile [0, n_blocks);
//                                             then the first block of every run, at most 8 of them)
//   b K                                    -> "entries lds_bytes"         (the candidate buffer)
//   s n_active R K scratch_option          -> "group n_groups covered bytes_per_query"  (covered: 1 if the groups hold every active
//                                             query exactly once, in order, none empty and none above `group`)
//   l R n_group                            -> "n_launches covered max_grid"  (covered: every run once, in order)
//   a n_q has_q_ptr has_docs_out has_n_out field first k n_fields -> the check's code (0 OK, 1 INVALID, 2 UNSUPPORTED, 3 STATE)
// A last line "ok <n> lines" is printed at end of input.
#include "field_topk_plan.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <sstream>

namespace tp = ss::ftopk;

int main() {
    char line[4096];
    long n_lines = 0;
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line + 1);
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0, g = 0, h = 0;
        if (line[0] == 'k' && (in >> a >> b)) {
            const uint64_t key = tp::value_key((int64_t)a, b != 0);
            std::printf("%016" PRIx64 " %" PRId64 "\n", key, tp::key_value(key, b != 0));
        } else if (line[0] == 'c' && (in >> a >> b >> c >> d >> e)) {
            std::printf("%d\n", tp::key_less(tp::value_key((int64_t)a, e != 0), (uint32_t)b, tp::value_key((int64_t)c, e != 0), (uint32_t)d) ? 1 : 0);
        } else if (line[0] == 'r' && (in >> a >> b >> c >> d)) {
            const uint32_t nb = (uint32_t)a, R = tp::runs_per_query(nb, (uint64_t)b, (uint32_t)c, (int64_t)d);
            bool tiles = nb == 0 ? R == 0 : (R >= 1 && R <= nb && tp::run_begin(0, R, nb) == 0 && tp::run_begin(R, R, nb) == nb);
            for (uint32_t r = 0; r < R; r++) tiles = tiles && tp::run_begin(r, R, nb) < tp::run_begin(r + 1, R, nb);
            std::printf("%u %d", R, tiles ? 1 : 0);
            for (uint32_t r = 0; r < R && r < 8; r++) std::printf(" %u", tp::run_begin(r, R, nb));
            std::printf("\n");
        } else if (line[0] == 'b' && (in >> a)) {
            std::printf("%u %u\n", tp::buffer_entries((uint32_t)a), tp::buffer_lds_bytes((uint32_t)a));
        } else if (line[0] == 's' && (in >> a >> b >> c >> d)) {
            const uint32_t group = tp::group_queries((uint64_t)a, (uint32_t)b, (uint32_t)c, tp::scratch_bytes_of((int64_t)d));
            const std::vector<tp::Group> gs = tp::groups((uint64_t)a, group);
            uint64_t next = 0;
            bool covered = true;
            for (const tp::Group& x : gs) {
                covered = covered && x.first == next && x.count >= 1 && x.count <= group;
                next += x.count;
            }
            covered = covered && next == (uint64_t)a;
            std::printf("%u %zu %d %" PRIu64 "\n", group, gs.size(), covered ? 1 : 0, tp::query_bytes((uint32_t)b, (uint32_t)c));
        } else if (line[0] == 'l' && (in >> a >> b)) {
            const std::vector<tp::Launch> ls = tp::launches((uint32_t)a, (uint32_t)b);
            uint64_t next = 0, max_grid = 0;
            bool covered = true;
            for (const tp::Launch& l : ls) {
                covered = covered && l.first == next && l.count >= 1;
                next += l.count;
                max_grid = std::max<uint64_t>(max_grid, (uint64_t)l.count * (uint64_t)b);
            }
            covered = covered && (b == 0 || next == (uint64_t)a);
            std::printf("%zu %d %" PRIu64 "\n", ls.size(), covered ? 1 : 0, max_grid);
        } else if (line[0] == 'a' && (in >> a >> b >> c >> d >> e >> f >> g >> h)) {
            char msg[256] = "";
            const int rc = tp::check_args(msg, sizeof(msg), "harness", (int32_t)a, b != 0, c != 0, d != 0, (int32_t)e, (int32_t)f, (int32_t)g, (int32_t)h);
            if ((rc != tp::OK) != (msg[0] != 0)) return 3;      // a refusal has a message, and only a refusal
            std::printf("%d\n", rc);
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
