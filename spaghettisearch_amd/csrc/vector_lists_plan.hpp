// vector_lists_plan.hpp — the host-only part of ss_vector_topk_probed and ss_vector_assign_lists (vector_lists.hip): rows
// per segment of a list, segments per list, the bound on the partial slots of one query from the list lengths in descending order, the
// split of a call into query batches at the bound of the partial lists, and the batch of ss_vector_assign_lists.  No HIP call and no HIP
// header: tests/vector_lists_plan_harness.cpp compiles this file alone (with a sanitizer).
#pragma once

#include "vector_plan.hpp"

#include <cstddef>
#include <cstdint>

namespace ss {
namespace veclists {

constexpr uint32_t MAX_LISTS = 65536;
constexpr uint32_t MIN_SEG_ROWS = 4 * vec::TILE;             // the default never goes below one round of the workgroup
constexpr uint64_t MAX_SEG_ROWS = (uint64_t)1 << 31;
constexpr uint32_t ASSIGN_BATCH = vec::MAX_QBLOCKS * vec::Q_TILE;   // doc rows of one top-1 search: never more than 65535 query blocks

// rows of one segment, a multiple of the 64-row tile: the option rounded up, or twice the mean list (a list of ordinary length is one
// segment) but not below what cuts the whole table into four segments per compute unit (one list holding every doc still fills the
// device)
inline uint64_t seg_rows(int64_t opt, uint64_t n_rows, uint32_t n_lists, uint32_t n_cu) {
    uint64_t r;
    if (opt > 0) r = (uint64_t)opt;
    else {
        const uint64_t mean2 = n_lists ? 2 * (n_rows / n_lists) : 0;
        const uint64_t spread = n_rows / ((uint64_t)4 * (n_cu ? n_cu : 1));
        r = mean2 > spread ? mean2 : spread;
        if (r < MIN_SEG_ROWS) r = MIN_SEG_ROWS;
    }
    if (r > MAX_SEG_ROWS) r = MAX_SEG_ROWS;
    return (r + vec::TILE - 1) / vec::TILE * vec::TILE;
}

inline uint64_t segs_of(uint64_t len, uint64_t seg) { return (len + seg - 1) / seg; }

struct Plan {
    bool ok = false;             // false: as vec::Plan::ok
    bool too_large = false;      // one query's partial lists alone are more than 2^31 keys
    uint32_t n_probe = 0;        // min(n_probe, n_lists): lists one query probes
    uint64_t seg_rows = 0;
    uint64_t slots_per_q = 0;    // >= 1: the sum of the n_probe largest per-list segment counts, the partial lists one query can fill
    uint64_t q_batch = 0;        // queries of one batch, >= 1
    uint64_t n_batches = 0;      // ceil(n_q / q_batch)
    uint64_t part_keys = 0;      // min(n_q, q_batch) * slots_per_q * k
    uint32_t q_block = 0, cap = 0, row_stride = 0, lds_bytes = 0;   // the LDS image of one workgroup: vec::plan's, for one batch
};

// len_desc: the list lengths in descending order (the largest lists give the largest segment counts)
inline Plan plan(const uint32_t* len_desc, uint32_t n_lists, uint64_t n_rows, uint32_t dim, uint64_t n_q, uint32_t k, uint32_t n_probe,
                 int64_t opt_seg_rows, int64_t opt_batch_q, uint32_t n_cu = 256, uint32_t lds_limit = 160u << 10) {
    Plan p;
    if (n_lists < 1 || n_lists > MAX_LISTS || n_probe < 1) return p;
    p.n_probe = n_probe < n_lists ? n_probe : n_lists;
    p.seg_rows = seg_rows(opt_seg_rows, n_rows, n_lists, n_cu);
    uint64_t slots = 0;
    for (uint32_t i = 0; i < p.n_probe; i++) slots += segs_of(len_desc[i], p.seg_rows);
    p.slots_per_q = slots ? slots : 1;
    const uint64_t per_q = p.slots_per_q * k;                       // keys of one query: the merge counts them in 32 bits
    if (per_q > ((uint64_t)1 << 31)) { p.too_large = true; return p; }
    uint64_t qb = vec::PART_BYTES / (per_q * 8);
    if (qb < 1) qb = 1;
    const uint64_t pairs = (((uint64_t)1 << 32) - 1) / p.n_probe;   // a (query, probe rank) pair is one 32-bit word
    if (qb > pairs) qb = pairs;
    const uint64_t by_block = (uint64_t)vec::MAX_QBLOCKS * vec::Q_TILE;   // the probe step's query blocks
    if (qb > by_block) qb = by_block;
    if (opt_batch_q > 0 && (uint64_t)opt_batch_q < qb) qb = (uint64_t)opt_batch_q;
    p.q_batch = qb;
    p.n_batches = (n_q + qb - 1) / qb;
    const uint64_t in_batch = n_q < qb ? n_q : qb;
    p.part_keys = in_batch * per_q;
    const vec::Plan v = vec::plan(0, dim, in_batch, k, 0, n_cu, lds_limit);
    if (!v.ok) return p;
    p.q_block = v.q_block; p.cap = v.cap; p.row_stride = v.row_stride; p.lds_bytes = v.lds_bytes;
    p.ok = true;
    return p;
}

// doc rows of one batch of ss_vector_assign_lists: the option, at most ASSIGN_BATCH
inline uint64_t assign_batch(int64_t opt) {
    if (opt > 0 && (uint64_t)opt < ASSIGN_BATCH) return (uint64_t)opt;
    return ASSIGN_BATCH;
}

}  // namespace veclists
}  // namespace ss
