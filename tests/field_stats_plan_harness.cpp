// field_stats_plan_harness.cpp — drives spaghettisearch_amd/csrc/field_stats_plan.hpp on the host (tests/test_field_stats_cpu.py compiles
// it with -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   d u width                              -> "q_any q_kind q_plain kind"   (the divider by its magic, by the form the kernel compiles in
//                                             for it, and `/`; kind 1 shift, 2 reciprocal)
//   R seed n                               -> "mismatches"                (n seeded random (u, width) pairs of mixed magnitudes, divider against `/`)
//   n origin width n_bins                  -> "span sat"
//   b origin width n_bins v                -> "slot slot_plain"           (bin_fixed by the divider and by `/`)
//   e n_bins v e0 .. e_n_bins              -> "slot"                      (bin_edges)
//   E n_bins e0 .. e_n_bins                -> 3 (n_bins + 1) slots: of e - 1, e, e + 1 for every edge e ("x" where that is no int64)
//   c n_bins e0 .. e_n_bins                -> "1" if strictly ascending else "0"
//   p n_bins option                        -> "use_lds hist_lds_bytes edges_in_lds edges_lds_bytes"
//   w n_bins                               -> "stride below above missing match"
//   s kind n_active x y scratch_option     -> "group n_launch_groups covered query_bytes"  (kind 0: histogram rows of x bins; kind 1: stats
//                                             partials of x runs and y fields; covered as in group_topk_plan_harness.cpp)
//   a n_q has_q_ptr has_out n_stat_fields has_fields n_fields f0 f1 f2 f3 -> check_stats_args' code
//   h n_q has_q_ptr has_out field width has_edges n_bins n_fields [e0 .. e_n_bins] -> check_hist_args' code (edges read when given)
// A last line "ok <n> lines" is printed at end of input.
#include "field_stats_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>

namespace fp = ss::fstats;

static bool read_edges(std::istringstream& in, uint32_t n_bins, std::vector<int64_t>* out) {
    out->clear();
    long long e = 0;
    for (uint32_t i = 0; i <= n_bins; i++) {
        if (!(in >> e)) return false;
        out->push_back((int64_t)e);
    }
    return true;
}

int main() {
    static char line[2 << 20];
    long n_lines = 0;
    std::vector<int64_t> edges;
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line + 1);
        unsigned long long u = 0, w = 0;
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0, g = 0, h = 0, i = 0, j = 0;
        if (line[0] == 'd' && (in >> u >> w)) {
            const fp::Divider dv = fp::make_divider(w);
            const int kind = fp::divider_kind(dv);
            const uint64_t q_kind = kind == fp::DIV_SHIFT ? fp::divide<fp::DIV_SHIFT>(dv, u) : fp::divide<fp::DIV_RECIPROCAL>(dv, u);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", fp::divide(dv, u), q_kind, fp::divide<fp::DIV_PLAIN>(dv, u), kind);
        } else if (line[0] == 'R' && (in >> a >> b)) {
            std::mt19937_64 rng((uint64_t)a);
            long bad = 0;
            for (long long k = 0; k < b; k++) {
                const uint64_t uu = rng() >> (rng() % 64), ww = (rng() >> (rng() % 64)) | 1ull << (rng() % 64);   // every magnitude, width >= 1
                if (fp::divide(fp::make_divider(ww), uu) != uu / ww) bad++;
            }
            std::printf("%ld\n", bad);
        } else if (line[0] == 'n' && (in >> a >> w >> b)) {
            const fp::Binner bn = fp::make_binner((int64_t)a, w, (uint32_t)b);
            std::printf("%" PRIu64 " %d\n", bn.span, bn.sat ? 1 : 0);
        } else if (line[0] == 'b' && (in >> a >> w >> b >> c)) {
            const fp::Binner bn = fp::make_binner((int64_t)a, w, (uint32_t)b);
            std::printf("%u %u\n", fp::bin_fixed(bn, (int64_t)c), fp::bin_fixed<fp::DIV_PLAIN>(bn, (int64_t)c));
        } else if (line[0] == 'e' && (in >> a >> b) && read_edges(in, (uint32_t)a, &edges)) {
            std::printf("%u\n", fp::bin_edges(edges.data(), (uint32_t)a, (int64_t)b));
        } else if (line[0] == 'E' && (in >> a) && read_edges(in, (uint32_t)a, &edges)) {
            for (const int64_t x : edges) {
                if (x == INT64_MIN) std::printf("x ");
                else std::printf("%u ", fp::bin_edges(edges.data(), (uint32_t)a, x - 1));
                std::printf("%u ", fp::bin_edges(edges.data(), (uint32_t)a, x));
                if (x == INT64_MAX) std::printf("x ");
                else std::printf("%u ", fp::bin_edges(edges.data(), (uint32_t)a, x + 1));
            }
            std::printf("\n");
        } else if (line[0] == 'c' && (in >> a) && read_edges(in, (uint32_t)a, &edges)) {
            std::printf("%d\n", fp::edges_ascending(edges.data(), (uint32_t)a) ? 1 : 0);
        } else if (line[0] == 'p' && (in >> a >> b)) {
            std::printf("%d %u %d %u\n", fp::use_lds((uint32_t)a, (int64_t)b) ? 1 : 0, fp::hist_lds_bytes((uint32_t)a), fp::edges_in_lds((uint32_t)a) ? 1 : 0,
                        fp::edges_lds_bytes((uint32_t)a));
        } else if (line[0] == 'w' && (in >> a)) {
            const uint32_t nb = (uint32_t)a;
            std::printf("%" PRIu64 " %u %u %u %u\n", fp::row_stride(nb), fp::slot_below(nb), fp::slot_above(nb), fp::slot_missing(nb), fp::slot_match(nb));
        } else if (line[0] == 's' && (in >> a >> b >> c >> d >> e)) {
            const uint64_t bytes = a == 0 ? fp::hist_query_bytes((uint32_t)c) : fp::stats_query_bytes((uint32_t)c, (uint32_t)d);
            const uint32_t group = fp::group_queries((uint64_t)b, bytes, fp::scratch_bytes_of((int64_t)e));
            const std::vector<fp::Group> gs = fp::groups((uint64_t)b, group);
            uint64_t next = 0;
            bool covered = true;
            for (const fp::Group& x : gs) {
                covered = covered && x.first == next && x.count >= 1 && x.count <= group;
                next += x.count;
            }
            covered = covered && next == (uint64_t)b;
            std::printf("%u %zu %d %" PRIu64 "\n", group, gs.size(), covered ? 1 : 0, bytes);
        } else if (line[0] == 'a' && (in >> a >> b >> c >> d >> e >> f >> g >> h >> i >> j)) {
            char msg[256] = "";
            const int32_t fields[4] = {(int32_t)g, (int32_t)h, (int32_t)i, (int32_t)j};
            const int rc = fp::check_stats_args(msg, sizeof(msg), "harness", (int32_t)a, b != 0, c != 0, (int32_t)d, e != 0, e != 0 ? fields : nullptr, (int32_t)f);
            if ((rc != fp::OK) != (msg[0] != 0)) return 3;      // a refusal has a message, and only a refusal
            std::printf("%d\n", rc);
        } else if (line[0] == 'h' && (in >> a >> b >> c >> d >> w >> e >> f >> g)) {
            char msg[256] = "";
            const bool with_values = e != 0 && f >= 1 && f <= fp::MAX_HIST_BINS && read_edges(in, (uint32_t)f, &edges);
            const int rc = fp::check_hist_args(msg, sizeof(msg), "harness", (int32_t)a, b != 0, c != 0, (int32_t)d, w, e != 0, with_values ? edges.data() : nullptr,
                                               (int32_t)f, (int32_t)g);
            if ((rc != fp::OK) != (msg[0] != 0)) return 3;
            std::printf("%d\n", rc);
        } else {
            std::fprintf(stderr, "bad line: %.200s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
