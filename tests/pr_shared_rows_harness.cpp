// Drives the shared-row planner of spaghettisearch_amd/csrc/pr_plan.hpp (plan_shared_rows, SharedRows::row_of) from stdin;
// tests/test_pr_shared_rows_cpu.py compiles this with the host compiler alone, under AddressSanitizer and UBSan, and checks what it prints.
//   <pos_nd> <n> <out-degree>...  <q> <queried out-degree>...
// prints: "table <table_rows> <zrow> <base>", "deg <distinct degrees, rising>", "rows <table row of each input degree>",
// "query <table row of each queried degree>"
#include "pr_plan.hpp"

#include <cstdio>
#include <iostream>

int main() {
    uint32_t pos_nd = 0;
    size_t n = 0, q = 0;
    std::cin >> pos_nd >> n;
    std::vector<uint32_t> od(n);
    for (auto& v : od) std::cin >> v;
    std::cin >> q;
    std::vector<uint32_t> ask(q);
    for (auto& v : ask) std::cin >> v;
    if (!std::cin) return 2;
    const SharedRows sh = plan_shared_rows(od.data(), od.size(), pos_nd);
    printf("table %llu %u %u\n", (unsigned long long)sh.table_rows, sh.zrow, sh.base);
    printf("deg");
    for (uint32_t v : sh.deg) printf(" %u", v);
    printf("\nrows");
    for (uint32_t v : od) printf(" %u", sh.row_of(v));
    printf("\nquery");
    for (uint32_t v : ask) printf(" %u", sh.row_of(v));
    printf("\n");
    return 0;
}
