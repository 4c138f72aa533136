// A stand-alone program around spaghettisearch_amd/csrc/vector_lists_plan.hpp (host-only: no HIP header on the include path).
// test_vector_lists_cpu.py compiles it with AddressSanitizer + UBSan and feeds it one case per line:
//   P dim n_q k n_probe opt_seg_rows opt_batch_q n_cu lds_limit n_runs (len count)...   the plan of a probed call; the list lengths are
//                                                                                      given as runs and sorted descending here
//   S opt n_rows n_lists n_cu                                                           seg_rows
//   A opt                                                                               assign_batch
// and reads one line of numbers per case, then "ok <cases> lines".
#include "vector_lists_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main() {
    namespace vl = ss::veclists;
    std::string line;
    unsigned long long n_lines = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'P') {
            unsigned long long dim, n_q, k, n_probe, n_cu, lds, n_runs;
            long long opt_seg, opt_batch;
            in >> dim >> n_q >> k >> n_probe >> opt_seg >> opt_batch >> n_cu >> lds >> n_runs;
            std::vector<uint32_t> len;
            unsigned long long n_rows = 0;
            for (unsigned long long r = 0; r < n_runs; r++) {
                unsigned long long l, c;
                in >> l >> c;
                len.insert(len.end(), (size_t)c, (uint32_t)l);
                n_rows += l * c;
            }
            if (!in) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            std::sort(len.begin(), len.end(), std::greater<uint32_t>());
            const vl::Plan p = vl::plan(len.data(), (uint32_t)len.size(), n_rows, (uint32_t)dim, n_q, (uint32_t)k, (uint32_t)n_probe, opt_seg, opt_batch,
                                        (uint32_t)n_cu, (uint32_t)lds);
            // the slot bound again, by the definition: the n_probe largest per-list segment counts
            unsigned long long slots = 0;
            if (p.seg_rows) {
                std::vector<unsigned long long> segs;
                for (uint32_t l : len) segs.push_back(vl::segs_of(l, p.seg_rows));
                std::sort(segs.begin(), segs.end(), std::greater<unsigned long long>());
                for (size_t i = 0; i < segs.size() && i < p.n_probe; i++) slots += segs[i];
            }
            std::printf("%d %d %u %llu %llu %llu %llu %llu %u %u %u %llu\n", (int)p.ok, (int)p.too_large, p.n_probe, (unsigned long long)p.seg_rows,
                        (unsigned long long)p.slots_per_q, (unsigned long long)p.q_batch, (unsigned long long)p.n_batches, (unsigned long long)p.part_keys,
                        p.q_block, p.cap, p.lds_bytes, slots);
        } else if (kind == 'S') {
            long long opt;
            unsigned long long n_rows, n_lists, n_cu;
            in >> opt >> n_rows >> n_lists >> n_cu;
            if (!in) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            std::printf("%llu\n", (unsigned long long)vl::seg_rows(opt, n_rows, (uint32_t)n_lists, (uint32_t)n_cu));
        } else if (kind == 'A') {
            long long opt;
            in >> opt;
            if (!in) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            std::printf("%llu\n", (unsigned long long)vl::assign_batch(opt));
        } else {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %llu lines\n", n_lines);
    return 0;
}
