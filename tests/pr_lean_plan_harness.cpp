// Drives the lean walk of the PageRank work planner (plan_lean_items in spaghettisearch_amd/csrc/pr_plan.hpp) from stdin;
// tests/test_pr_lean_plan_cpu.py compiles this with the host compiler alone, under AddressSanitizer and UBSan, and checks what it prints.
//   <gw> <sl_nd> <nblocks> <t_quad> <item_turns> <base>
//   <runs> <val start>... <rows>      non-dangling rows: in-degree runs, falling
//   <runs> <val start>... <rows>      dangling rows
// prints the dealt table ("dealt ..." per item, "woff ..."), the lean one ("lean ..." per item, "loff ...") and the modelled turns per
// wave of both walks: "load <full max> <full mean> <lean max> <lean mean>" (item_costs; the lean walk keeps the full deal).
#include "pr_plan.hpp"

#include <cstdio>
#include <iostream>

static ss::SortedDegrees read_degrees() {
    ss::SortedDegrees d;
    size_t runs = 0;
    std::cin >> runs;
    d.val.resize(runs);
    d.start.resize(runs + 1);
    for (size_t j = 0; j < runs; j++) std::cin >> d.val[j] >> d.start[j];
    std::cin >> d.start[runs];
    return d;
}

static void print_items(const char* tag, const std::vector<WorkItem>& items) {
    for (const WorkItem& w : items) printf("%s %u %u %u %u %u %u\n", tag, w.kind, w.row, w.count, w.nseg, w.sbase, w.tix);
}

int main() {
    int gw = 0;
    uint32_t sl_nd = 0, nblocks = 0, base = 0;
    PlanOptions opt;
    std::cin >> gw >> sl_nd >> nblocks >> opt.t_quad >> opt.item_turns >> base;
    const ss::SortedDegrees nd = read_degrees(), d = read_degrees();
    if (!std::cin || gw < 8 || !nblocks) return 2;
    Cut cut = cut_items(nd, d, sl_nd, gw, false, opt);
    const uint32_t nw = nblocks * WAVES;
    const std::vector<double>& cost = item_costs(cut, nd, d, sl_nd, gw, false);
    std::vector<uint32_t>& owner = deal_items(cut, cost, nw, false, opt);
    std::vector<double> full(nw, 0.0), lean(nw, 0.0);
    for (size_t i = 0; i < cut.items.size(); i++) {
        full[owner[i]] += cost[i];
        if (cut.items[i].row < sl_nd) lean[owner[i]] += cost[i];
    }
    const std::vector<uint32_t>& woff = place_items(cut, owner, nw);
    const LeanPlan lp = plan_lean_items(cut.items, woff, nw, sl_nd, base);
    print_items("dealt", cut.items);
    printf("woff");
    for (uint32_t v : woff) printf(" %u", v);
    printf("\n");
    print_items("lean", lp.items);
    printf("loff");
    for (uint32_t v : lp.woff) printf(" %u", v);
    printf("\n");
    double fmax = 0.0, fsum = 0.0, lmax = 0.0, lsum = 0.0;
    for (uint32_t w = 0; w < nw; w++) {
        fmax = std::max(fmax, full[w]); fsum += full[w];
        lmax = std::max(lmax, lean[w]); lsum += lean[w];
    }
    printf("load %.3f %.3f %.3f %.3f\n", fmax, fsum / nw, lmax, lsum / nw);
    return 0;
}
