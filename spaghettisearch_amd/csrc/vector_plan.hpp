// vector_plan.hpp — the host-only part of ss_vector_topk (vector.hip): how the docs are cut into chunks and the queries
// into blocks, and the LDS image of one k_vec_topk workgroup, from n_docs, dim, n_q, k, the option "vec.chunk_docs" and two figures of
// the device (compute units, LDS bytes a workgroup may have).  No HIP call and no HIP header: tests/vector_plan_harness.cpp compiles
// this file alone (with a sanitizer).
#pragma once

#include <cstdint>

namespace ss {
namespace vec {

constexpr uint32_t TILE = 64;            // docs of one wave step: four 16-row A tiles of the 16x16x64 product; chunks are multiples of it
constexpr uint32_t WAVES = 4;            // waves of a k_vec_topk workgroup: one round of the workgroup is WAVES * TILE docs
constexpr uint32_t Q_TILE = 16;          // queries of one B tile
constexpr uint32_t ROW_PAD = 16;         // bytes between the query rows of the LDS image (rows of dim bytes would all start in bank 0)
constexpr uint32_t MAX_DIM = 1024, MAX_K = 1024;
constexpr uint32_t HOLES = MAX_K;        // 16-bit slots of the compaction's hole list
constexpr uint64_t PART_BYTES = (uint64_t)256 << 20;   // the default chunking keeps the partial lists below this
constexpr uint32_t MAX_QBLOCKS = 65535;  // grid.y

struct Plan {
    bool ok = false;             // false: the LDS cannot hold one block of 16 queries with k + TILE candidates each, or too many query blocks
    bool too_large = false;      // the partial lists do not fit 2^40 bytes: SS_ERR_OOM without asking the allocator
    uint32_t q_block = 0;        // queries of one workgroup: 16, 32 or 64
    uint32_t n_qblocks = 0;      // ceil(n_q / q_block): how often every doc byte is read from memory
    uint32_t chunk_docs = 0;     // docs of one chunk, a multiple of TILE
    uint32_t n_chunks = 0;       // ceil(n_docs / chunk_docs); 0 only when n_docs == 0
    uint32_t cap = 0;            // candidate keys one query holds in LDS, >= k + TILE
    uint32_t row_stride = 0;     // bytes from one query row of the LDS image to the next
    uint32_t lds_bytes = 0;      // dynamic LDS of the workgroup
    uint64_t part_keys = 0;      // n_q * n_chunks * k keys of 8 bytes
};

inline uint32_t lds_fixed(uint32_t qb) {         // thresholds, valid words per wave, counts, histogram, hole list, flags
    return qb * 8 + WAVES * qb * 8 + qb * 4 + 256 * 4 + HOLES * 2 + 64;
}
inline uint32_t lds_of(uint32_t qb, uint32_t row_stride, uint32_t cap) { return qb * row_stride + qb * cap * 8 + lds_fixed(qb); }

// the chunk [begin, end) of chunk c
inline uint64_t chunk_begin(const Plan& p, uint32_t c) { return (uint64_t)c * p.chunk_docs; }
inline uint64_t chunk_end(const Plan& p, uint32_t c, uint64_t n_docs) {
    const uint64_t e = ((uint64_t)c + 1) * p.chunk_docs;
    return e < n_docs ? e : n_docs;
}

inline Plan plan(uint64_t n_docs, uint32_t dim, uint64_t n_q, uint32_t k, int64_t opt_chunk_docs, uint32_t n_cu = 256,
                 uint32_t lds_limit = 160u << 10) {
    Plan p;
    if (dim < 64 || dim > MAX_DIM || dim % 64 || k < 1 || k > MAX_K || n_docs >> 32) return p;
    p.row_stride = dim + ROW_PAD;
    // ---- query block and candidate capacity: the widest block whose queries keep max(2k, k + 96) candidates each, first in half the
    // LDS (two workgroups per CU), then in all of it; failing that 16 queries with what fits, at least k + TILE
    const uint32_t want = 2 * k > k + 96 ? 2 * k : k + 96;
    const uint32_t budgets[2] = {lds_limit / 2, lds_limit};
    auto fit = [&](uint32_t qb, uint32_t budget) -> uint32_t {
        const uint32_t fixed = qb * p.row_stride + lds_fixed(qb);
        return budget > fixed ? (budget - fixed) / (qb * 8) : 0;
    };
    for (int b = 0; b < 2 && !p.q_block; b++)
        for (uint32_t qb = 64; qb >= 16 && !p.q_block; qb /= 2) {
            if (qb > 16 && n_q <= qb / 2) continue;                 // (a narrower block holds every query)
            const uint32_t c = fit(qb, budgets[b]);
            if (c >= want) { p.q_block = qb; p.cap = c; }
        }
    if (!p.q_block) {
        const uint32_t c = fit(16, lds_limit);
        if (c < k + TILE) return p;
        p.q_block = 16;
        p.cap = c;
    }
    if (p.cap > 4 * want) p.cap = 4 * want;                         // (more than that buys no fewer compactions worth the LDS)
    p.lds_bytes = lds_of(p.q_block, p.row_stride, p.cap);
    const uint64_t nqb = (n_q + p.q_block - 1) / p.q_block;
    if (nqb > MAX_QBLOCKS) return p;
    p.n_qblocks = (uint32_t)nqb;
    // ---- chunks
    uint64_t cd;
    if (opt_chunk_docs > 0) {
        cd = (uint64_t)opt_chunk_docs > ((uint64_t)1 << 31) ? (uint64_t)1 << 31 : (uint64_t)opt_chunk_docs;
        cd = (cd + TILE - 1) / TILE * TILE;
    } else {
        // four workgroups per compute unit over all query blocks, a chunk not below one round of the workgroup, the partial lists bounded
        uint64_t target = ((uint64_t)4 * (n_cu ? n_cu : 1) + (nqb ? nqb : 1) - 1) / (nqb ? nqb : 1);
        const uint64_t per_chunk = (n_q ? n_q : 1) * (uint64_t)k * 8;
        const uint64_t most = PART_BYTES / per_chunk ? PART_BYTES / per_chunk : 1;
        if (target > most) target = most;
        if (target < 1) target = 1;
        cd = (n_docs + target - 1) / target;
        cd = (cd + TILE - 1) / TILE * TILE;
        if (cd < WAVES * TILE) cd = WAVES * TILE;
    }
    p.chunk_docs = (uint32_t)cd;
    p.n_chunks = (uint32_t)((n_docs + cd - 1) / cd);
    const uint64_t per_q = (uint64_t)p.n_chunks * k;                // < 2^26 * 2^10
    if (n_q && per_q > ((uint64_t)1 << 37) / n_q) { p.too_large = true; return p; }
    p.part_keys = n_q * per_q;
    p.ok = true;
    return p;
}

}  // namespace vec
}  // namespace ss
