// pr_plan.hpp — the work plan of a PageRank sweep: pure host arithmetic over the two run-length-encoded in-degree tables of a rank
// (sorted_degrees.hpp).  Rows are cut into work items (cut_items), the items of the wave-item kernels get a modelled cost
// (item_costs), are dealt to the grid's waves (deal_items) and laid out per (wave, class) (place_items).  No device header, no
// graph, no context: ss_pr_create (pagerank.hip) fills PlanOptions from the context's options and uploads what comes out;
// tests/pr_plan_harness.cpp compiles this file with the host compiler alone.
#pragma once
#include "sorted_degrees.hpp"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int CH = 16;               // edges per chunk of the GW=16 path
constexpr uint32_t SEGW = 2048;      // edges per V_SEG piece

enum : uint32_t { W_SEG = 0, W_WAVE = 1, W_GROUP = 2, W_ZERO = 3,   // GW < 8 (k_pr_step): block-owned items
                  // GW >= 8 (k_pr_sweep): every item belongs to ONE wave
                  V_SEG = 8,     // a <= SEGW-edge piece of a row with more than T_MULTI in-edges (partials + ticket)
                  V_ROWW = 9,    // a whole row, T_QUAD < in-edges <= T_MULTI
                  V_QUAD = 10,   // `count` rows, one per lane group and turn, each `nseg` (= chunks per row) 16-edge chunks long
                  V_DEG = 11,    // `count` rows of EXACTLY `nseg` (<= 8) in-edges: several rows per lane group and chunk
                  V_ZERO = 12 }; // `count` non-dangling rows without in-edges

struct WorkItem {
    uint32_t kind;
    uint32_t row;     // first local row
    uint32_t count;   // rows (WAVE/GROUP/ZERO) or segment index (SEG)
    uint32_t nseg;    // SEG: segments of this row
    uint32_t sbase;   // SEG: index of the row's first segment partial
    uint32_t tix;     // SEG: per-row ticket index
    uint32_t beg, end; // k_pr_sweep items: the item's in-edges are in_src[beg .. end)
};

constexpr uint32_t plan_div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// What the context's "pr.*" options say about the plan, defaults resolved (ss_pr_create: plan_options).  AUTO: the default depends on
// something only a later step knows (the item count, the occupancy query) and is resolved there.
struct PlanOptions {
    static constexpr int64_t AUTO = INT64_MIN;
    uint32_t t_quad = 128;          // "pr.t_quad": longest row of a V_QUAD item (k_pr_sweep_n keeps 256)
    // turns per V_DEG item (a V_QUAD item: twice that): small graphs want finer items — with ~20 turns per wave in all, an
    // item of 16 leaves the deal nothing to balance ("pr.item_turns", 1 .. 64; default from the graph's size)
    uint32_t item_turns = 4;
    size_t items_per_wave = 1;      // "pr.items_per_wave": k_pr_sweep_n's waves get at least that many items
    int64_t deal_snake = AUTO;      // "pr.deal_snake" (deal_items)
    int64_t deal_global = 2;        // "pr.deal_global": 0 = chunks in table order, 1 = one order over all classes, 2 = class by class
    int64_t blocks_per_cu = AUTO;   // "pr.blocks_per_cu" (default: what the occupancy query admits)
    int64_t class_order = 235401;   // "pr.class_order" (pack_class_order)
    int64_t n_class_order = 2310;   // "pr.n_class_order" (pack_n_order)
    int64_t stagger = 0;            // "pr.stagger"
};

// (scratch kept per thread across calls: freshly reserved vectors of a few MB cost more in page faults — 0.7 ms at 10M nodes — than
//  the items cost to make)
struct PlanScratch {
    std::vector<WorkItem> seg, rwg, wav, grp, zer;               // cut_items, gw < 8: per class
    std::vector<WorkItem> vseg, vroww, vquad, vdeg[3], vzero;    // cut_items, gw >= 8: wave-owned items of k_pr_sweep
    std::vector<WorkItem> items, dealt;
    std::vector<double> cost, load;
    std::vector<uint32_t> owner, by_load, idx, order, bucket, woff, cnt;
    std::vector<std::pair<double, uint32_t>> key;
    std::vector<WorkItem> lean_items;                            // plan_lean_items
    std::vector<uint32_t> lean_woff;
};
inline PlanScratch& plan_scratch() {
    static thread_local PlanScratch s;
    return s;
}

struct Cut {
    std::vector<WorkItem>& items;   // (the calling thread's scratch)
    uint32_t nsegs = 0, nmulti = 0; // segment partials / multi-segment rows (tickets)
    uint32_t seg_edges = 0;         // edges per W_SEG piece
    uint32_t pos_nd = 0, pos_d = 0; // rows WITH in-edges per class
    uint32_t vbeg[7] = {0};         // wave-item classes: class k's items are items[vbeg[k] .. vbeg[k + 1])
};

// The rows of a rank cut into work items.  `nd` / `d`: the sorted in-degrees of its non-dangling / dangling rows, the dangling ones
// start at local row `sl_nd`; `gw`: the lane-group width the items are cut for; lane_rows: for k_pr_sweep_n (a LANE per short row).
inline Cut cut_items(const ss::SortedDegrees& nd, const ss::SortedDegrees& d, uint32_t sl_nd, int gw, bool lane_rows, const PlanOptions& opt) {
    PlanScratch& s = plan_scratch();
    Cut cut{s.items};
    uint32_t& nsegs = cut.nsegs;
    uint32_t& nmulti = cut.nmulti;
    const uint32_t NSLOT = 64 / gw;
    // gw < 8: rows above T_SEG in-edges get block(s) of their own, then wave-per-row / group-per-row classes.
    // gw >= 8: emit_v below.
    const uint32_t T_SEG = 32 * NSLOT;
    const uint32_t T_WAVE = 2 * NSLOT;
    const uint32_t seg_edges = cut.seg_edges = 128 * NSLOT;
    auto &seg = s.seg, &rwg = s.rwg, &wav = s.wav, &grp = s.grp, &zer = s.zer;
    // gw >= 8: wave-owned items of k_pr_sweep.  deg is sorted descending.
    auto &vseg = s.vseg, &vroww = s.vroww, &vquad = s.vquad, &vzero = s.vzero;
    auto& vdeg = s.vdeg;
    for (auto* v : {&seg, &rwg, &wav, &grp, &zer, &vseg, &vroww, &vquad, &vdeg[0], &vdeg[1], &vdeg[2], &vzero}) v->clear();
    auto emit_v = [&](const ss::SortedDegrees& deg, uint32_t row0, bool non_dangling, uint32_t& n_pos) {
        const uint32_t cnt = (uint32_t)deg.size();
        const uint32_t T_MULTI = 4096, T_DEG = 8;
        const uint32_t T_QUAD = opt.t_quad;
        const uint32_t item_turns = opt.item_turns;
        // (rows and limits only move forward: two cursors over the degree runs instead of a bisection per item — the bisections were
        //  most of the 0.8 ms this took at config 4)
        size_t j_at = 0, j_lim = 0;
        const size_t n_run = deg.val.size();
        auto deg_at = [&](uint32_t r) -> uint32_t {              // in-degree of row r (r < cnt, never smaller than the last call's)
            while (deg.start[j_at + 1] <= r) j_at++;
            return deg.val[j_at];
        };
        auto end_above = [&](uint32_t lim) -> uint32_t {         // first row with in-degree <= lim (lim never larger than the last call's)
            while (j_lim < n_run && deg.val[j_lim] > lim) j_lim++;
            return deg.start[j_lim];
        };
        uint32_t r = 0;
        for (; r < cnt && deg_at(r) > T_MULTI; r++) {
            const uint32_t ns = (deg_at(r) + SEGW - 1) / SEGW;
            const uint32_t tix = nmulti++;
            for (uint32_t sg = 0; sg < ns; sg++) vseg.push_back({V_SEG, row0 + r, sg, ns, nsegs, tix});
            nsegs += ns;
        }
        {
            const uint32_t end = std::min(cnt, end_above(T_QUAD));
            for (; r < end; r++) vroww.push_back({V_ROWW, row0 + r, 0, 0, 0, 0});
        }
        // one row per lane group and turn; an item's rows all take nch = ceil(longest / 16) turns, at most gw row groups
        // and about 32 turns per item
        while (r < cnt && deg_at(r) > T_DEG) {
            const uint32_t nch = (deg_at(r) + CH - 1) / CH;
            const uint32_t max_groups = std::min<uint32_t>((uint32_t)gw, std::max<uint32_t>(1u, 2u * item_turns / nch));
            // rows of the same turn count nch: in-degree > (nch - 1) * CH (and > T_DEG)
            const uint32_t lim = std::max<uint32_t>(T_DEG, (nch - 1) * CH);
            const uint32_t end = end_above(lim);
            const uint32_t same = end > r ? end - r : 0u;
            const uint32_t rows = std::min<uint32_t>(same, max_groups * NSLOT);
            vquad.push_back({V_QUAD, row0 + r, rows, nch, 0, 0});
            r += rows;
        }
        // exact-degree runs
        while (r < cnt && deg_at(r) > 0) {
            const uint32_t D = deg_at(r);
            // deg is sorted descending and run-length encoded: the rows with exactly D in-edges end with r's run
            const uint32_t run = deg.start[j_at + 1] - r;
            const uint32_t R = D <= 2 ? 8 : D <= 4 ? 4 : 2;
            // (k_pr_sweep_n gives every LANE a row: whole waves of 64 rows per item there)
            const uint32_t per_item = lane_rows ? 64u * item_turns : NSLOT * R * item_turns;
            auto& out = vdeg[R == 2 ? 0 : R == 4 ? 1 : 2];
            for (uint32_t o = 0; o < run; o += per_item) out.push_back({V_DEG, row0 + r + o, std::min(per_item, run - o), D, 0, 0});
            r += run;
        }
        n_pos = r;
        const uint32_t ZERO_ROWS = 16 * NSLOT;
        if (non_dangling)
            for (uint32_t o = r; o < cnt; o += ZERO_ROWS) vzero.push_back({V_ZERO, row0 + o, std::min<uint32_t>(ZERO_ROWS, cnt - o), 0, 0, 0});
    };
    auto emit = [&](const ss::SortedDegrees& deg, uint32_t row0, bool non_dangling, uint32_t& n_pos) {
        if (gw >= 8) { emit_v(deg, row0, non_dangling, n_pos); return; }
        const uint32_t cnt = (uint32_t)deg.size();
        // deg is sorted descending: class boundaries
        const uint32_t a = deg.first_at_most(T_SEG);
        const uint32_t c = std::max(a, deg.first_at_most(0));
        for (uint32_t r = 0; r < a; r++) {
            const uint32_t ns = (deg[r] + seg_edges - 1) / seg_edges;
            const uint32_t tix = ns > 1 ? nmulti++ : 0;
            for (uint32_t sg = 0; sg < ns; sg++) seg.push_back({W_SEG, row0 + r, sg, ns, nsegs, tix});
            nsegs += ns;
        }
        {
            const uint32_t b = std::min(c, std::max(a, deg.first_at_most(T_WAVE)));
            for (uint32_t r = a; r < b; r += WAVES) wav.push_back({W_WAVE, row0 + r, std::min<uint32_t>(WAVES, b - r), 0, 0, 0});
            const uint32_t GROUP_ROWS = WAVES * NSLOT * 4;   // 4 rows per lane group per block
            for (uint32_t r = b; r < c; r += GROUP_ROWS) grp.push_back({W_GROUP, row0 + r, std::min<uint32_t>(GROUP_ROWS, c - r), 0, 0, 0});
        }
        n_pos = c;
        // rows without in-edges all share one rank (zero_row_rank): only the non-dangling ones have work
        // (their next contribution); 8 elements per thread
        const uint32_t ZERO_ROWS = (TPB * 8) / gw;
        if (non_dangling)
            for (uint32_t r = c; r < cnt; r += ZERO_ROWS) zer.push_back({W_ZERO, row0 + r, std::min<uint32_t>(ZERO_ROWS, cnt - r), 0, 0, 0});
    };
    emit(nd, 0, true, cut.pos_nd);
    const size_t vquad_split = vquad.size();            // the non-dangling rows' groups (falling length), then the dangling rows'
    emit(d, sl_nd, false, cut.pos_d);
    auto& items = cut.items;
    auto& vbeg = cut.vbeg;
    items.clear();
    items.reserve(seg.size() + rwg.size() + wav.size() + grp.size() + zer.size());
    // heavy work first
    items.insert(items.end(), seg.begin(), seg.end());
    items.insert(items.end(), rwg.begin(), rwg.end());
    items.insert(items.end(), wav.begin(), wav.end());
    items.insert(items.end(), grp.begin(), grp.end());
    items.insert(items.end(), zer.begin(), zer.end());
    // k_pr_sweep: longest first (pieces of the hubs, whole long rows, then the row groups by falling length)
    vbeg[0] = (uint32_t)items.size();
    items.insert(items.end(), vseg.begin(), vseg.end());
    items.insert(items.end(), vroww.begin(), vroww.end());
    vbeg[1] = (uint32_t)items.size();
    // row groups by falling length (the dangling class was appended after the non-dangling one)
    // (each of the two classes is in falling length already: one stable merge, not a sort)
    std::inplace_merge(vquad.begin(), vquad.begin() + (ptrdiff_t)vquad_split, vquad.end(),
                       [](const WorkItem& a, const WorkItem& b) { return a.nseg > b.nseg; });
    items.insert(items.end(), vquad.begin(), vquad.end());
    for (int k = 0; k < 3; k++) {
        vbeg[2 + k] = (uint32_t)items.size();
        items.insert(items.end(), vdeg[k].begin(), vdeg[k].end());
    }
    vbeg[5] = (uint32_t)items.size();
    items.insert(items.end(), vzero.begin(), vzero.end());
    vbeg[6] = (uint32_t)items.size();
    if (items.empty()) items.push_back({W_ZERO, 0, 0, 0, 0, 0});   // a graph without work: one empty item, so that nothing downstream is empty
    return cut;
}

// The wave items' modelled costs in turns (from the sorted in-degrees the graph keeps on the host).  `gw`, `lane_rows`: as cut_items.
inline const std::vector<double>& item_costs(const Cut& cut, const ss::SortedDegrees& nd, const ss::SortedDegrees& d, uint32_t sl_nd, int gw, bool lane_rows) {
    const std::vector<WorkItem>& items = cut.items;
    std::vector<double>& cost = plan_scratch().cost;
    const uint32_t NS = 64 / gw;
    // (rows rise inside a class's items: a cursor per degree table, a bisection only when a row steps back)
    struct DegCursor {
        const ss::SortedDegrees* d;
        size_t j = 0;
        uint32_t at(uint32_t r) {
            if (r >= d->size()) return 0u;
            if (d->start[j] > r) j = d->run_of(r);
            while (d->start[j + 1] <= r) j++;
            return d->val[j];
        }
    } cur_nd{&nd}, cur_d{&d};
    auto deg_of = [&](uint32_t lrow) -> uint32_t { return lrow < sl_nd ? cur_nd.at(lrow) : cur_d.at(lrow - sl_nd); };
    cost.assign(items.size(), 0.0);
    for (size_t i = 0; i < items.size(); i++) {
        const WorkItem& w = items[i];
        double turns = 1.0;
        switch (w.kind) {
            case V_ROWW: turns = plan_div_up(deg_of(w.row), NS * CH); break;
            case V_SEG: turns = plan_div_up(std::min<uint32_t>(SEGW, deg_of(w.row) - w.count * SEGW), NS * CH) + 2.0; break;
            case V_QUAD: turns = (double)plan_div_up(w.count, NS) * w.nseg; break;
            case V_DEG: {
                if (lane_rows) { turns = (double)plan_div_up(w.count, 64u) * (0.6 + 0.2 * (w.nseg <= 2 ? 2 : w.nseg <= 4 ? 4 : 8)); break; }   // a pass of 64 rows: 2, 4 or 8 gathers per lane + a row each
                const uint32_t R = w.nseg <= 2 ? 8 : w.nseg <= 4 ? 4 : 2;
                turns = (double)plan_div_up(w.count, NS * R) * (R == 8 ? 2.5 : R == 4 ? 1.7 : 1.3);   // a turn finishes R rows per lane group
                break;
            }
            default: turns = 0.5; break;
        }
        cost[i] = turns + 1.0;                                   // + the item's own overhead
    }
    return cost;
}

// Owner (wave 0 .. nw - 1) per item.
// Longest-processing-time deal: items in table order (classes by falling item length), each to the wave with the
// least work so far — every wave ends up with the same number of turns (+- one item), whatever the degree mix.
// The items come in falling cost inside each class.  Deal them nw at a time: the waves ordered by their load so far, the
// chunk's items in table order (costliest first inside a class) to the least loaded waves first — the longest-processing-
// time rule applied per chunk, one sort of nw loads per chunk instead of a heap operation per item (3 ms -> 0.4 ms at
// 60k items / 3072 waves, same balance: every wave ends within one item of the mean).
inline std::vector<uint32_t>& deal_items(const Cut& cut, const std::vector<double>& cost, uint32_t nw, bool lane_rows, const PlanOptions& opt) {
    PlanScratch& s = plan_scratch();
    const size_t n_items = cut.items.size();
    auto &owner = s.owner, &by_load = s.by_load, &idx = s.idx, &order = s.order, &bucket = s.bucket;
    auto& load = s.load;
    auto& key = s.key;
    owner.assign(n_items, 0u);
    load.assign(nw, 0.0);
    by_load.resize(nw);
    for (uint32_t w = 0; w < nw; w++) by_load[w] = w;
    // Many chunks (a large graph): the loads are not sorted between chunks, every other chunk is dealt in reverse — costs fall
    // smoothly inside a class, so the snake ends as level as the sorted deal (config 4: sweep 0.960 against 0.963 ms) and the
    // deal takes 0.3 ms of host time instead of 2.8.  Few chunks: least-loaded-first as before (config 2 on k_pr_sweep<8>: 0.075
    // against 0.077 ms); k_pr_sweep_n's finer items sweep the same either way and the update is 0.1 ms shorter with the snake.
    const bool snake = (opt.deal_snake == PlanOptions::AUTO ? (n_items >= (size_t)8 * nw || lane_rows ? 1 : 0) : opt.deal_snake) != 0;
    // All items by falling cost first ("pr.deal_global": 1 = one order over all classes, 2 = class by class in table order): a
    // counting sort on the cost in sixteenths of a turn, stable (table order inside a bucket), O(items).  The chunks below
    // then come sorted.  [Sorting each chunk took 0.2 of
    // config 2's 0.4 ms here: inside a class the costs fall, but every run of equal rows ends in a short item, so a chunk
    // is dozens of falling runs, not one.]
    // (`tools/pr_deal.py`, sweep ms at 10M / 50M: K = 16 chunks 0.959, global 0.963, class-major 0.955; K = 1 chunks 0.383, global
    //  0.379, class-major 0.389 — k_pr_sweep and k_pr_sweep_n<2> take class-major, k_pr_sweep_n<1> the one global order)
    // (K = 2 on k_pr_sweep_n at 10M / 50M: class-major 0.471, global 0.481, chunks 0.483)
    const int64_t deal_mode = opt.deal_global;
    const bool global_order = deal_mode != 0;
    if (global_order) {
        constexpr uint32_t NB = 1u << 14;
        // (mode 2: class-major — the table's class order kept, falling cost inside a class)
        const auto bkey = [&](size_t i) { return NB - 1 - (uint32_t)std::min<double>(cost[i] * 16.0, (double)(NB - 1)); };
        bucket.assign(NB + 1, 0u);
        order.resize(n_items);
        size_t c0 = 0;
        for (int kcls = 0; kcls < (deal_mode == 2 ? 6 : 1); kcls++) {
            const size_t c1 = deal_mode == 2 ? (kcls < 5 ? std::min<size_t>(cut.vbeg[kcls + 1], n_items) : n_items) : n_items;
            if (kcls) std::fill(bucket.begin(), bucket.end(), 0u);
            for (size_t i = c0; i < c1; i++) bucket[bkey(i) + 1]++;
            for (uint32_t b = 0; b < NB; b++) bucket[b + 1] += bucket[b];
            for (size_t i = c0; i < c1; i++) order[c0 + bucket[bkey(i)]++] = (uint32_t)i;
            c0 = c1;
        }
    }
    // (Equal modelled loads do not end together: the hardware issues oldest-first, so of a CU's four resident blocks the one
    //  that arrived first is out of items after 623 us at config 4 and the last one after 906 — -DSS_PR_WAVETIME,
    //  tools/pr_wavetime.py.  Shares weighted by those speeds were tried and dropped: the late blocks end where they ended
    //  before, the early ones later, the sweep 0.985-1.0 ms instead of 0.955 — the sweep is bound by the memory system's
    //  throughput, and who finishes first is the scheduler's business.)
    for (size_t i0 = 0; i0 < n_items; i0 += nw) {
        const size_t n_chunk = std::min<size_t>(nw, n_items - i0);
        if (i0 && snake) {
            std::reverse(by_load.begin(), by_load.end());
        } else if (i0) {
            // (load, wave) pairs sorted by value: several times faster than a comparator that reads load[] through the ids
            key.resize(nw);
            for (uint32_t w = 0; w < nw; w++) key[w] = {load[w], w};
            std::sort(key.begin(), key.end());
            for (uint32_t w = 0; w < nw; w++) by_load[w] = key[w].second;
        }
        // the chunk's costliest item to the least loaded wave: order the chunk by falling cost (it already is, except
        // where it crosses a class boundary)
        // (a few falling runs: merged pairwise, O(chunk) per boundary — a full stable_sort of the chunk through cost[] took
        //  0.15 ms a chunk, most of config 2's deal)
        idx.resize(n_chunk);
        for (size_t j = 0; j < n_chunk; j++) idx[j] = global_order ? order[i0 + j] : (uint32_t)(i0 + j);
        const auto falling = [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; };
        size_t run_end = 0, n_merge = 0;
        for (size_t j = 1; j <= n_chunk && !global_order; j++) {
            if (j < n_chunk && !(cost[i0 + j] > cost[i0 + j - 1])) continue;     // still falling (or level)
            if (run_end) {
                if (++n_merge > 8) { std::stable_sort(idx.begin(), idx.end(), falling); break; }
                std::inplace_merge(idx.begin(), idx.begin() + (ptrdiff_t)run_end, idx.begin() + (ptrdiff_t)j, falling);
            }
            run_end = j;
        }
        for (size_t j = 0; j < n_chunk; j++) {
            owner[idx[j]] = by_load[j];
            load[by_load[j]] += cost[idx[j]];
        }
    }
    return owner;
}

// The dealt table: cut.items becomes the items in (wave, class) order plus the two pad items the pipelines read ahead into; returns
// woff[8 * w + c], where wave w's items of class c begin (`owner` is used up).
// table order inside a wave's list = item order = class order: count per (wave, class), offsets, place
inline const std::vector<uint32_t>& place_items(Cut& cut, std::vector<uint32_t>& owner, uint32_t nw) {
    PlanScratch& s = plan_scratch();
    auto& items = cut.items;
    auto &woff = s.woff, &cnt = s.cnt;
    // (the items are in class order: owner[i] * 8 + class, computed once per class range)
    woff.assign((size_t)nw * 8, 0);
    cnt.assign((size_t)nw * 8, 0);
    for (int k = 0; k < 6; k++) {
        const size_t i1 = k < 5 ? std::min<size_t>(cut.vbeg[k + 1], items.size()) : items.size();
        for (size_t i = std::min<size_t>(cut.vbeg[k], i1); i < i1; i++) { owner[i] = owner[i] * 8 + (uint32_t)k; cnt[owner[i]]++; }
    }
    uint32_t run_off = 0;
    for (uint32_t w = 0; w < nw; w++) {
        for (int k = 0; k < 8; k++) {
            woff[(size_t)w * 8 + k] = run_off;
            run_off += cnt[(size_t)w * 8 + k];
            cnt[(size_t)w * 8 + k] = woff[(size_t)w * 8 + k];       // becomes the write cursor of (wave, class)
        }
    }
    s.dealt.resize(items.size());
    for (size_t i = 0; i < items.size(); i++) s.dealt[cnt[owner[i]]++] = items[i];
    s.dealt.push_back({V_ZERO, 0, 0, 0, 0, 0, 0, 0});              // the pipelines read two items ahead
    s.dealt.push_back({V_ZERO, 0, 0, 0, 0, 0, 0, 0});
    items.swap(s.dealt);
    return woff;
}

// ---- the lean sweep's walk ("pr.lean_sweeps") -------------------------------------------------------------------------------
// A lean sweep of k_pr_sweep (pr_sweep.hip) writes neither ranks nor an L1 change, so the items of dangling rows (local row >= sl_nd:
// no table row either) have nothing to produce in it.  The dealt table mixes the two row classes inside a (wave, class) range
// (hub pieces and whole long rows of both in class 0, the mid rows merged by length), and the full sweep's L1 change depends on
// that order — so the table stays as it is, and the lean sweep gets a second, shorter one: every (wave, class) range without its
// dangling items, the others in the order place_items gave them (the contribution sums of a wave are added in the same order in
// both sweeps), its own two pad items behind it and its own per-wave class offsets.  All pieces of a cut dangling row go together:
// no ticket of such a row is ever taken in a lean sweep.  The waves are NOT dealt again; what a wave's lean walk costs is whatever
// the full deal left it.
// `dealt`, `woff`: what place_items returned (the table with its two pad items); base: where in the work table the lean items will
// stand (the offsets count from there).
struct LeanPlan {
    const std::vector<WorkItem>& items;   // (the calling thread's scratch)
    const std::vector<uint32_t>& woff;    // [nw][8]
};
inline LeanPlan plan_lean_items(const std::vector<WorkItem>& dealt, const std::vector<uint32_t>& woff, uint32_t nw, uint32_t sl_nd, uint32_t base) {
    PlanScratch& s = plan_scratch();
    auto& items = s.lean_items;
    auto& loff = s.lean_woff;
    items.clear();
    loff.assign((size_t)nw * 8, base);
    const size_t n = dealt.size() >= 2 ? dealt.size() - 2 : 0;   // without the pad items
    for (size_t j = 0; j < (size_t)nw * 8 && j < woff.size(); j++) {
        loff[j] = base + (uint32_t)items.size();
        const size_t lo = std::min<size_t>(woff[j], n), hi = j + 1 < woff.size() ? std::min<size_t>(woff[j + 1], n) : n;
        for (size_t i = lo; i < hi; i++)
            if (dealt[i].row < sl_nd) items.push_back(dealt[i]);
    }
    items.push_back({V_ZERO, 0, 0, 0, 0, 0, 0, 0});              // the pipelines read two items ahead
    items.push_back({V_ZERO, 0, 0, 0, 0, 0, 0, 0});
    return {items, loff};
}

// "pr.class_order": six decimal digits, position by position (012345 = long rows, mid rows, the three short-row classes,
// edge-less rows), packed 3 bits per position; anything that is not a permutation of 0..5 falls back to that order
inline uint32_t pack_class_order(int64_t code) {
    uint32_t packed = 0, seen = 0;
    for (int pos = 5; pos >= 0; pos--) {
        const uint32_t c = (uint32_t)(code % 10);
        code /= 10;
        packed |= (c & 7u) << (3 * pos);
        if (c < 6) seen |= 1u << c;
    }
    return seen == 0x3Fu ? packed : (0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12 | 5u << 15);
}
// "pr.n_class_order": four digits for k_pr_sweep_n's phases (0 = long rows, 1 = mid rows, 2 = rows of <= 8 in-edges, 3 = edge-less rows),
// 2 bits per position
// (all 24 orders, round 5: 2^20 nodes / 5M edges 0.0472 ms for 2-3-1-0 against 0.0492 for 0-1-2-3, the worst; at 10M / 50M the
//  numbering order is within 0.2 % of the best and short-rows-first among the worst: 0.3796 against 0.379 / 0.389)
inline uint32_t pack_n_order(int64_t code) {
    uint32_t packed = 0, seen = 0;
    for (int pos = 3; pos >= 0; pos--) {
        const uint32_t c = (uint32_t)(code % 10);
        code /= 10;
        packed |= (c & 3u) << (2 * pos);
        if (c < 4) seen |= 1u << c;
    }
    return seen == 0xFu ? packed : (0u | 1u << 2 | 2u << 4 | 3u << 6);
}

// ---- shared table rows of the edge-less sources ("pr.share_zero_rows") ----------------------------------------------------------
// A non-dangling row without in-edges holds the one rank all such rows share, so its contribution d * xz / outdeg depends on its
// out-degree alone: the sweep's table keeps ONE row per distinct out-degree among them instead of one per row.  Layout of such a
// table: rows [0, pos_nd) as ever (the rows with in-edges), the all-zero row at pos_nd, the shared rows behind it in rising degree.
struct SharedRows {
    std::vector<uint32_t> deg;      // the distinct out-degrees, rising: shared row j belongs to deg[j]
    uint32_t zrow = 0;              // the all-zero row (= pos_nd)
    uint32_t base = 0;              // first shared row (= pos_nd + 1)
    uint64_t table_rows = 0;        // rows of one table buffer: pos_nd + 1 + deg.size()
    // the table row of a source with out-degree `od`; the zero row for a degree that is not in the map
    uint32_t row_of(uint32_t od) const {
        const auto it = std::lower_bound(deg.begin(), deg.end(), od);
        return it != deg.end() && *it == od ? base + (uint32_t)(it - deg.begin()) : zrow;
    }
};
// `od`: the out-degrees of the n non-dangling rows without in-edges (table rows pos_nd .. pos_nd + n).  Any number of distinct
// values: flags per value while the largest stays near n, a sort otherwise.
inline SharedRows plan_shared_rows(const uint32_t* od, size_t n, uint32_t pos_nd) {
    SharedRows sh;
    uint32_t hi = 0;
    for (size_t i = 0; i < n; i++) hi = std::max(hi, od[i]);
    if (n && (uint64_t)hi <= 4 * (uint64_t)n + 65536) {
        std::vector<unsigned char> seen((size_t)hi + 1, 0);
        for (size_t i = 0; i < n; i++) seen[od[i]] = 1;
        for (size_t v = 0; v <= hi; v++)
            if (seen[v]) sh.deg.push_back((uint32_t)v);
    } else if (n) {
        sh.deg.assign(od, od + n);
        std::sort(sh.deg.begin(), sh.deg.end());
        sh.deg.erase(std::unique(sh.deg.begin(), sh.deg.end()), sh.deg.end());
    }
    sh.zrow = pos_nd;
    sh.base = pos_nd + 1;
    sh.table_rows = (uint64_t)pos_nd + 1 + sh.deg.size();
    return sh;
}

}  // namespace
