// maxsim_plan_harness.cpp — drives spaghettisearch_amd/csrc/maxsim_plan.hpp on the host (tests/test_maxsim_cpu.py compiles it with
// -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   q max_m                 -> QT of a call whose largest query has max_m tokens
//   p n v0 v1 .. vn         -> "code max_m" of check_qt_ptr over n queries (0 OK, 1 INVALID, 2 UNSUPPORTED)
//   t n v0 v1 .. vn         -> the code of check_tok_ptr over n docs
//   d dim                   -> 1 if dim may be a token table's, else 0
//   w option                -> the clamped value of option "maxsim.wide_tokens"
//   l qt dim                -> "row_stride lds_bytes"
//   g n_q k_in cu_count     -> "wg_rows wgs_per_query n_wgs ok covered" (covered: 1 if the workgroups, mapped as the kernel maps them,
//                              hold every (query, row < k_in) exactly once, wg_rows is a multiple of 4 in 4 .. 64; 0 also for a grid
//                              of more than 2^24 workgroups, which is not walked)
// A last line "ok <n> lines" is printed at end of input.
#include "maxsim_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mp = ss::msp;

// "n v0 .. vn" -> the n + 1 values; false on a short line
static bool read_ptr(const char* s, std::vector<uint64_t>* out) {
    char* end = nullptr;
    const unsigned long long n = std::strtoull(s, &end, 10);
    if (end == s) return false;
    out->clear();
    for (unsigned long long i = 0; i <= n; i++) {
        s = end;
        const unsigned long long v = std::strtoull(s, &end, 10);
        if (end == s) return false;
        out->push_back(v);
    }
    return true;
}

int main() {
    static char line[1 << 16];
    long n_lines = 0;
    std::vector<uint64_t> vals;
    while (std::fgets(line, sizeof(line), stdin)) {
        long long a = 0, b = 0, c = 0;
        char msg[256] = "";
        if (line[0] == 'q' && std::sscanf(line + 1, "%lld", &a) == 1) {
            std::printf("%u\n", mp::qt_of((uint32_t)a));
        } else if (line[0] == 'p' && read_ptr(line + 1, &vals)) {
            std::vector<uint32_t> ptr(vals.begin(), vals.end());
            uint32_t max_m = 0;
            const int rc = mp::check_qt_ptr(msg, sizeof(msg), "harness", ptr.data(), ptr.size() - 1, &max_m);
            if ((rc != mp::OK) != (std::strlen(msg) > 0)) return 3;                // a refusal, and only a refusal, has a text
            std::printf("%d %u\n", rc, max_m);
        } else if (line[0] == 't' && read_ptr(line + 1, &vals)) {
            const int rc = mp::check_tok_ptr(msg, sizeof(msg), "harness", vals.data(), vals.size() - 1);
            if ((rc != mp::OK) != (std::strlen(msg) > 0)) return 3;
            std::printf("%d\n", rc);
        } else if (line[0] == 'd' && std::sscanf(line + 1, "%lld", &a) == 1) {
            std::printf("%d\n", mp::dim_ok(a) ? 1 : 0);
        } else if (line[0] == 'w' && std::sscanf(line + 1, "%lld", &a) == 1) {
            std::printf("%u\n", mp::wide_tokens_of((int64_t)a));
        } else if (line[0] == 'l' && std::sscanf(line + 1, "%lld %lld", &a, &b) == 2) {
            std::printf("%u %u\n", mp::row_stride((uint32_t)b), mp::lds_bytes((uint32_t)a, (uint32_t)b));
        } else if (line[0] == 'g' && std::sscanf(line + 1, "%lld %lld %lld", &a, &b, &c) == 3) {
            const uint64_t n_q = (uint64_t)a;
            const uint32_t k_in = (uint32_t)b;
            const mp::Grid g = mp::grid(n_q, k_in, (uint32_t)c);
            bool covered = g.ok && g.wg_rows >= mp::WAVES && g.wg_rows <= mp::MAX_WG_ROWS && g.wg_rows % mp::WAVES == 0 &&
                           g.n_wgs == n_q * g.wgs_per_query && g.n_wgs <= (1ull << 24);   // (larger grids are not walked)
            if (covered) {
                const uint64_t n_check = n_q < 64 ? n_q : 64;                      // the first queries and the last: the map is the same for all
                std::vector<uint32_t> seen((size_t)n_check * k_in, 0);
                for (uint64_t b2 = 0; b2 < g.n_wgs; b2++) {
                    const uint64_t q = b2 / g.wgs_per_query;
                    const uint64_t slot = q < n_check - 1 ? q : q == n_q - 1 ? n_check - 1 : n_check;
                    if (slot >= n_check) continue;
                    const uint32_t r0 = (uint32_t)(b2 - q * g.wgs_per_query) * g.wg_rows;
                    for (uint32_t i = 0; i < g.wg_rows && r0 + i < k_in; i++) seen[(size_t)slot * k_in + r0 + i]++;
                }
                for (uint32_t s : seen) covered = covered && s == 1;
            }
            std::printf("%u %u %" PRIu64 " %d %d\n", g.wg_rows, g.wgs_per_query, g.n_wgs, g.ok ? 1 : 0, covered ? 1 : 0);
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
