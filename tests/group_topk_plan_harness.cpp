// group_topk_plan_harness.cpp — drives spaghettisearch_amd/csrc/group_topk_plan.hpp on the host (tests/test_group_topk_cpu.py compiles
// it with -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   k count rank                           -> "key(hex) count_back rank_back"
//   p n_groups option                      -> "use_lds hist_lds_bytes"    (the counting path and the histogram's dynamic LDS)
//   w n_groups                             -> "stride slot_match slot_ungrouped"   (words of a counter row and its two extra slots)
//   b K                                    -> "entries lds_bytes"         (the candidate buffer of k_group_select: keys alone)
//   s n_active n_groups scratch_option     -> "group n_launch_groups covered row_bytes"  (covered: 1 if the groups hold every active
//                                             query exactly once, in order, none empty and none above `group`)
//   r n_blocks n_active n_cu forced        -> "R tiles begin ..."         (field_topk_plan.hpp's runs, reused)
//   l R n_group                            -> "n_launches covered max_grid"  (field_topk_plan.hpp's launches, reused)
//   a n_q has_q_ptr has_groups_out has_n_out first m has_table -> the check's code (0 OK, 1 INVALID, 2 UNSUPPORTED, 3 STATE)
// A last line "ok <n> lines" is printed at end of input.
#include "group_topk_plan.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <sstream>

namespace gp = ss::gtopk;

int main() {
    char line[4096];
    long n_lines = 0;
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line + 1);
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0, g = 0;
        if (line[0] == 'k' && (in >> a >> b)) {
            const uint64_t key = gp::pack_key((uint32_t)a, (uint32_t)b);
            if (key == gp::PAD_KEY) return 4;                   // no count >= 1 gives the pad key
            std::printf("%016" PRIx64 " %u %u\n", key, gp::key_count(key), gp::key_rank(key));
        } else if (line[0] == 'p' && (in >> a >> b)) {
            std::printf("%d %u\n", gp::use_lds((uint32_t)a, (int64_t)b) ? 1 : 0, gp::hist_lds_bytes((uint32_t)a));
        } else if (line[0] == 'w' && (in >> a)) {
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", gp::row_stride((uint32_t)a), gp::slot_match((uint32_t)a), gp::slot_ungrouped((uint32_t)a));
        } else if (line[0] == 'b' && (in >> a)) {
            std::printf("%u %u\n", gp::buffer_entries((uint32_t)a), gp::buffer_lds_bytes((uint32_t)a));
        } else if (line[0] == 's' && (in >> a >> b >> c)) {
            const uint32_t group = gp::group_queries((uint64_t)a, (uint32_t)b, gp::scratch_bytes_of((int64_t)c));
            const std::vector<gp::Group> gs = gp::groups((uint64_t)a, group);
            uint64_t next = 0;
            bool covered = true;
            for (const gp::Group& x : gs) {
                covered = covered && x.first == next && x.count >= 1 && x.count <= group;
                next += x.count;
            }
            covered = covered && next == (uint64_t)a;
            std::printf("%u %zu %d %" PRIu64 "\n", group, gs.size(), covered ? 1 : 0, gp::row_stride((uint32_t)b) * 4);
        } else if (line[0] == 'r' && (in >> a >> b >> c >> d)) {
            const uint32_t nb = (uint32_t)a, R = gp::runs_per_query(nb, (uint64_t)b, (uint32_t)c, (int64_t)d);
            bool tiles = nb == 0 ? R == 0 : (R >= 1 && R <= nb && gp::run_begin(0, R, nb) == 0 && gp::run_begin(R, R, nb) == nb);
            for (uint32_t r = 0; r < R; r++) tiles = tiles && gp::run_begin(r, R, nb) < gp::run_begin(r + 1, R, nb);
            std::printf("%u %d", R, tiles ? 1 : 0);
            for (uint32_t r = 0; r < R && r < 8; r++) std::printf(" %u", gp::run_begin(r, R, nb));
            std::printf("\n");
        } else if (line[0] == 'l' && (in >> a >> b)) {
            const std::vector<gp::Launch> ls = gp::launches((uint32_t)a, (uint32_t)b);
            uint64_t next = 0, max_grid = 0;
            bool covered = true;
            for (const gp::Launch& l : ls) {
                covered = covered && l.first == next && l.count >= 1;
                next += l.count;
                max_grid = std::max<uint64_t>(max_grid, (uint64_t)l.count * (uint64_t)b);
            }
            covered = covered && (b == 0 || next == (uint64_t)a);
            std::printf("%zu %d %" PRIu64 "\n", ls.size(), covered ? 1 : 0, max_grid);
        } else if (line[0] == 'a' && (in >> a >> b >> c >> d >> e >> f >> g)) {
            char msg[256] = "";
            const int rc = gp::check_args(msg, sizeof(msg), "harness", (int32_t)a, b != 0, c != 0, d != 0, (int32_t)e, (int32_t)f, g != 0);
            if ((rc != gp::OK) != (msg[0] != 0)) return 3;      // a refusal has a message, and only a refusal
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
