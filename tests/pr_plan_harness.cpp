// Drives the PageRank work planner (spaghettisearch_amd/csrc/pr_plan.hpp) from stdin; tests/test_pr_plan_cpu.py compiles this with
// the host compiler alone — no device header on the include path — and checks what it prints.
//   plan <gw> <lane_rows> <sl_nd> <nblocks> <t_quad> <item_turns> <deal_snake (-1 = default)> <deal_global>
//        <runs> <val start>... <rows>      non-dangling rows: in-degree runs, falling
//        <runs> <val start>... <rows>      dangling rows
//   class_order <code> | n_order <code>
#include "pr_plan.hpp"

#include <cstdio>
#include <iostream>
#include <string>

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
    std::string cmd;
    std::cin >> cmd;
    int64_t code = 0;
    if (cmd == "class_order") { std::cin >> code; printf("%u\n", pack_class_order(code)); return 0; }
    if (cmd == "n_order") { std::cin >> code; printf("%u\n", pack_n_order(code)); return 0; }
    if (cmd != "plan") return 2;
    int gw = 0, lane_rows = 0;
    uint32_t sl_nd = 0, nblocks = 0;
    int64_t snake = -1;
    PlanOptions opt;
    std::cin >> gw >> lane_rows >> sl_nd >> nblocks >> opt.t_quad >> opt.item_turns >> snake >> opt.deal_global;
    if (snake >= 0) opt.deal_snake = snake;
    const ss::SortedDegrees nd = read_degrees(), d = read_degrees();
    if (!std::cin) return 2;
    Cut cut = cut_items(nd, d, sl_nd, gw, lane_rows != 0, opt);
    printf("cut %u %u %u %u %u\n", cut.nsegs, cut.nmulti, cut.seg_edges, cut.pos_nd, cut.pos_d);
    printf("vbeg");
    for (uint32_t v : cut.vbeg) printf(" %u", v);
    printf("\n");
    print_items("item", cut.items);
    if (gw < 8) return 0;                          // block items are walked round-robin: nothing is dealt
    const uint32_t nw = nblocks * WAVES;
    const std::vector<double>& cost = item_costs(cut, nd, d, sl_nd, gw, lane_rows != 0);
    std::vector<uint32_t>& owner = deal_items(cut, cost, nw, lane_rows != 0, opt);
    const std::vector<uint32_t>& woff = place_items(cut, owner, nw);
    print_items("dealt", cut.items);
    printf("woff");
    for (uint32_t v : woff) printf(" %u", v);
    printf("\n");
    return 0;
}
