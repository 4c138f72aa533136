// links_plan_harness.cpp — spaghettisearch_amd/csrc/links_plan.hpp on its own: compiled by tests/test_links_plan_cpu.py with the host
// compiler, no device header on the include path, under AddressSanitizer + UBSan.  Reads lines "n_rows m max_degree wave_max chunk"
// and prints the bounds; checks the properties the kernels rely on itself.
#include <cstdio>
#include <cstdlib>

#include "links_plan.hpp"

static void require(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "links_plan_harness: %s\n", what);
        std::exit(1);
    }
}

int main() {
    using namespace ss::links;
    unsigned long long n_rows, m, max_degree;
    long long wave_max, chunk;
    int lines = 0;
    while (std::scanf("%llu %llu %llu %lld %lld", &n_rows, &m, &max_degree, &wave_max, &chunk) == 5) {
        const Bounds b = bounds(n_rows, (uint32_t)m, max_degree, wave_max, chunk);
        require(b.wave_max >= OPT_MIN && b.wave_max <= OPT_MAX && b.chunk >= OPT_MIN && b.chunk <= OPT_MAX, "an option left its range");
        require(b.lds_entries >= b.wave_max && b.lds_entries >= b.chunk, "the LDS does not hold a work item");
        require((uint64_t)b.lds_entries * LDS_ENTRY_BYTES <= 64 * 1024, "a work item needs more LDS than a workgroup may ask for");
        // every row of the graph becomes at most items_per_row items, and every item stages at most lds_entries edges
        const uint64_t probes[] = {0, 1, b.wave_max - 1ull, b.wave_max, b.wave_max + 1ull, b.chunk, b.chunk + 1ull, max_degree / 2, max_degree};
        for (uint64_t len : probes) {
            if (len > max_degree) continue;
            const uint64_t it = items_of_row(len, b.wave_max, b.chunk);
            require(it <= b.items_per_row, "a row makes more items than the bound");
            require((len == 0) == (it == 0), "only an empty row makes no item");
            if (it == 1 && len <= b.wave_max) require(len <= b.lds_entries, "an unsplit row overflows the LDS");
            if (len > b.wave_max) require((it - 1) * b.chunk < len && len <= it * b.chunk, "the chunks do not cover the row exactly");
        }
        if (!b.too_large) {
            require(b.items == n_rows * b.items_per_row, "items");
            require(b.items * m <= ((uint64_t)1 << 60), "the partial block's size overflows");
        }
        std::printf("%u %u %u %llu %llu %d\n", b.wave_max, b.chunk, b.lds_entries, (unsigned long long)b.items_per_row,
                    (unsigned long long)b.items, b.too_large ? 1 : 0);
        lines++;
    }
    std::printf("ok %d lines\n", lines);
    return 0;
}
