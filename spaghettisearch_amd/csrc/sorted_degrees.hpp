// sorted_degrees.hpp — the in-degrees of a rank's rows as the host sees them (no device header: the PageRank work planner,
// pr_plan.hpp, is host-only and reads nothing else of the graph).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ss {

// The local in-degrees, sorted descending per class, as the HOST sees them for work-table building: run-length encoded on the
// device (a few thousand distinct values at 10M rows: a few KB over PCIe instead of 40 MB, and a table the host's searches
// find in its L1 instead of a 40 MB array they miss in).  val[j] = in-degree of rows [start[j], start[j + 1]).
struct SortedDegrees {
    std::vector<uint32_t> val, start;     // start has val.size() + 1 entries; start.back() = number of rows
    size_t size() const { return start.empty() ? 0 : start.back(); }
    size_t run_of(size_t i) const {        // the run that holds row i (i < size())
        size_t lo = 0, hi = val.size();
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) >> 1;
            if (start[mid] <= i) lo = mid; else hi = mid;
        }
        return lo;
    }
    uint32_t operator[](size_t i) const { return val[run_of(i)]; }
    // number of rows with in-degree > lim = index of the first row whose in-degree is <= lim
    uint32_t first_at_most(uint32_t lim) const {
        size_t lo = 0, hi = val.size();   // first run with val <= lim (val is strictly descending)
        while (lo < hi) {
            const size_t mid = (lo + hi) >> 1;
            if (val[mid] > lim) lo = mid + 1; else hi = mid;
        }
        return start.empty() ? 0u : start[lo];
    }
};

}  // namespace ss
