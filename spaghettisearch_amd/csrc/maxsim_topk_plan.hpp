// maxsim_topk_plan.hpp — the part of ss_maxsim_topk (maxsim_topk.hip) that needs no device: the cut table
// ss_scorer_set_doc_tokens keeps beside tok_ptr (the first doc at or behind every multiple of SLICE_TOKENS tokens), how many queries one
// workgroup of k_maxsim_topk holds and with how long a candidate list each, the LDS it asks for, and the chunks (runs of slices) a
// call's grid is made of, from what the host knows at registration time.  tests/maxsim_topk_plan_harness.cpp runs all of it on the host
// under ASan + UBSan.  Includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "maxsim_plan.hpp"

namespace ss {
namespace mtp {

constexpr uint32_t SLICE_TOKENS = 64;                     // tokens between two entries of the cut table; a chunk is a run of slices
constexpr uint32_t GROUP_DOCS = 64;                       // docs of one round of a workgroup: one ballot word, one 'nearly full' check
constexpr uint32_t INC = GROUP_DOCS;                      // keys one query can gain in one round
constexpr uint32_t MAX_QB = 16;                           // queries of one workgroup: 16, 8, 4, 2 or 1
constexpr uint32_t HOLES = 1024;                          // 16-bit slots of the compaction's hole list (vec::HOLES: k <= 1024)
constexpr uint32_t MAX_K = 1024;                          // SS_MAX_TOPK
constexpr uint64_t PART_BYTES = (uint64_t)256 << 20;      // the default chunking keeps the partial lists below this
constexpr uint32_t MAX_QBLOCKS = 65535;                   // grid.y
constexpr uint64_t MAX_CHUNKS = 0x7FFFFFFFull;            // grid.x
constexpr uint32_t MIN_CHUNK_SLICES = 4;                  // the default chunking goes no finer

// ---- the cut table ----------------------------------------------------------------------------------------------------------
// n_slices = ceil(tok_ptr[n_docs] / SLICE_TOKENS); cut[s], s < n_slices: the first doc d with tok_ptr[d] >= s * SLICE_TOKENS, so
// cut[0] = 0; cut[n_slices] = the last doc that has a token, + 1.  Slice s holds the docs [cut[s], cut[s + 1]): those whose first token
// lies in it and the token-less docs standing at such a place with them.  The token-less docs behind the table's last token lie in no
// slice: they are never candidates, and one workgroup per query block would walk all of them (9M of the benchmark's 10M docs).  A doc
// longer than a slice leaves the slices it runs through empty.  A table without a token has no slice (and no candidate).  tok_ptr:
// checked by msp::check_tok_ptr; n_docs < 2^32.
inline uint64_t n_slices_of(uint64_t total_tokens) { return (total_tokens + SLICE_TOKENS - 1) / SLICE_TOKENS; }
inline void build_cuts(const uint64_t* tok_ptr, uint64_t n_docs, std::vector<uint32_t>* cut) {
    const uint64_t n_slices = n_slices_of(tok_ptr[n_docs]);
    cut->assign(n_slices ? (size_t)n_slices + 1 : 0, 0u);
    if (!n_slices) return;
    uint64_t d = 0;
    for (uint64_t s = 0; s < n_slices; s++) {
        while (d < n_docs && tok_ptr[d] < s * SLICE_TOKENS) d++;   // (s * SLICE_TOKENS < tok_ptr[n_docs]: d stops below n_docs)
        (*cut)[(size_t)s] = (uint32_t)d;
    }
    uint64_t e = n_docs;                                                          // (a slice exists, so a doc has a token: e stops above 0)
    while (tok_ptr[e] == tok_ptr[e - 1]) e--;
    (*cut)[(size_t)n_slices] = (uint32_t)e;
}

// ---- one workgroup ----------------------------------------------------------------------------------------------------------
// LDS of k_maxsim_topk<qt> holding qb queries with cap candidate keys each: per query the token image (16 qt rows at msp::row_stride),
// the list, the slots' joined maxima of a doc the waves share, threshold, count, mask id and m_q; then the select's histogram and words,
// and the compaction's hole list.
constexpr uint32_t lds_per_query(uint32_t qt, uint32_t dim) { return 16 * qt * msp::row_stride(dim) + 16 * qt * 4 + 8 + 4 + 4 + 4; }
constexpr uint32_t lds_fixed() { return 256 * 4 + 16 * 4 + HOLES * 2; }
constexpr uint32_t lds_of(uint32_t qb, uint32_t qt, uint32_t dim, uint32_t cap) { return qb * (lds_per_query(qt, dim) + cap * 8) + lds_fixed(); }

struct Block {
    bool ok = false;             // false: not even one query with k + INC candidates fits lds_limit
    uint32_t qb = 0;             // queries of one workgroup
    uint32_t cap = 0;            // candidate keys one query holds, >= k + INC
    uint32_t lds_bytes = 0;
};
// The largest qb of 16 / 8 / 4 / 2 / 1 whose queries keep at least k + INC candidates each inside lds_limit (a qb of which half would
// hold every query is passed over); cap is what fits, at most max(2 k, k + 4 INC): more buys no fewer compactions worth the LDS.
inline Block block(uint32_t dim, uint32_t qt, uint32_t k, uint64_t n_q, uint32_t lds_limit) {
    Block b;
    if (!msp::dim_ok(dim) || (qt != 1 && qt != 2 && qt != 4) || k < 1 || k > MAX_K) return b;
    const uint32_t most = 2 * k > k + 4 * INC ? 2 * k : k + 4 * INC;
    for (uint32_t qb = MAX_QB; qb >= 1; qb /= 2) {
        if (qb > 1 && n_q <= qb / 2) continue;
        const uint64_t fixed = (uint64_t)qb * lds_per_query(qt, dim) + lds_fixed();
        if (lds_limit <= fixed) continue;
        uint32_t cap = (uint32_t)((lds_limit - fixed) / ((uint64_t)qb * 8));
        if (cap < k + INC) continue;
        if (cap > most) cap = most;
        b.qb = qb;
        b.cap = cap;
        b.lds_bytes = lds_of(qb, qt, dim, cap);
        b.ok = true;
        return b;
    }
    return b;
}

// ---- the chunks -------------------------------------------------------------------------------------------------------------
struct Chunks {
    bool ok = false;             // false: more query blocks or chunks than one launch holds
    bool too_large = false;      // the partial lists do not fit 2^40 bytes: SS_ERR_OOM without asking the allocator
    uint32_t n_qblocks = 0;      // ceil(n_q / qb): how often every token byte is read from memory
    uint64_t chunk_slices = 0;   // slices of one chunk, >= 1
    uint32_t n_chunks = 0;       // ceil(n_slices / chunk_slices); 0 only for a table without a token
    uint64_t part_keys = 0;      // n_q * n_chunks * k keys of 8 bytes
};
// Chunk c is the slices [c * chunk_slices, min((c + 1) * chunk_slices, n_slices)), i.e. the docs [cut[that begin], cut[that end]).
// opt_chunk_tokens > 0 forces the chunk (rounded up to whole slices); otherwise about four workgroups per compute unit over all query
// blocks, no chunk below MIN_CHUNK_SLICES, the partial lists bounded by PART_BYTES.
inline uint64_t chunk_first_slice(const Chunks& c, uint32_t i) { return (uint64_t)i * c.chunk_slices; }
inline uint64_t chunk_end_slice(const Chunks& c, uint32_t i, uint64_t n_slices) {
    const uint64_t e = ((uint64_t)i + 1) * c.chunk_slices;
    return e < n_slices ? e : n_slices;
}
inline Chunks chunks(uint64_t n_slices, uint64_t n_q, uint32_t qb, uint32_t k, int64_t opt_chunk_tokens, uint32_t n_cu) {
    Chunks c;
    if (!qb || !k) return c;
    const uint64_t nqb = (n_q + qb - 1) / qb;
    if (nqb > MAX_QBLOCKS) return c;
    c.n_qblocks = (uint32_t)nqb;
    uint64_t cs;
    if (opt_chunk_tokens > 0) {
        cs = ((uint64_t)opt_chunk_tokens + SLICE_TOKENS - 1) / SLICE_TOKENS;
    } else {
        uint64_t target = ((uint64_t)4 * (n_cu ? n_cu : 1) + (nqb ? nqb : 1) - 1) / (nqb ? nqb : 1);
        const uint64_t per_chunk = (n_q ? n_q : 1) * (uint64_t)k * 8;
        const uint64_t most = PART_BYTES / per_chunk ? PART_BYTES / per_chunk : 1;
        if (target > most) target = most;
        if (target < 1) target = 1;
        cs = (n_slices + target - 1) / target;
        if (cs < MIN_CHUNK_SLICES) cs = MIN_CHUNK_SLICES;
    }
    if (cs < 1) cs = 1;
    c.chunk_slices = cs;
    const uint64_t nc = (n_slices + cs - 1) / cs;
    if (nc > MAX_CHUNKS) return c;
    c.n_chunks = (uint32_t)nc;
    const uint64_t per_q = nc * k;                                  // < 2^31 * 2^10
    if (n_q && per_q > ((uint64_t)1 << 37) / n_q) { c.too_large = true; return c; }
    c.part_keys = n_q * per_q;
    c.ok = true;
    return c;
}

}  // namespace mtp
}  // namespace ss
