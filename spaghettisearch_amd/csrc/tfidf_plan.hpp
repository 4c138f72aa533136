// tfidf_plan.hpp — the host-only part of the TF-IDF build (tfidf.hip): the geometry constants its kernels and its partition share, the
// "tfidf.*" options, and the arithmetic that decides how a table of n_docs docs and n_post postings is summed — bucketed pass or one
// atomic per posting, the bucket shift and count, the block ranges, the head-list threshold, the buckets per owner thread, which
// k_scatter<W, BPT> instance runs and the two dynamic-LDS sizes.  No HIP call and no HIP header: tests/tfidf_plan_harness.cpp compiles
// this file alone (with a sanitizer) and tests/test_tfidf_plan_cpu.py holds it against tests/tfidf_cases.py's model.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ss {
namespace tfidf {

// ---- geometry (the SS_* macros are for variant builds: tools/build_variant.sh) -------------------------------------------------------
constexpr int CH = 4096;                       // postings per chunk of k_weight and k_weight_count (16 per thread of a 256-thread block)
constexpr int NB_MAX = 4096;                   // most buckets (LDS histogram of a k_weight_count block)
#ifndef SS_SC_TPB
#define SS_SC_TPB 1024
#endif
constexpr int SC_TPB = SS_SC_TPB;              // threads of a k_scatter block
#ifndef SS_SC_PT
#define SS_SC_PT (8192 / SS_SC_TPB)
#endif
constexpr int SC_PT = SS_SC_PT;                // records per thread
constexpr int SC_CH = SC_TPB * SC_PT;          // records per chunk (staged in LDS)
constexpr int SC_WIN = SC_CH;                  // term-window entries staged per chunk (a chunk spans at most SC_CH + 1 non-empty terms; beyond: global search)
constexpr int SC_PF = (1024 + SC_TPB - 1) / SC_TPB;   // entries of the next chunk's term window a thread prefetches (windows up to 1024 terms)
constexpr int SC_BPT_MAX = NB_MAX / SC_TPB;    // most buckets an owner thread of k_scatter keeps cursors for
#ifndef SS_HEAD_CAP
#define SS_HEAD_CAP 1024
#endif
constexpr int HEAD_CAP = SS_HEAD_CAP;          // most head lists (their run table sits in LDS beside the accumulators: 12 B each)
constexpr int HEAD_LEVELS = 24;                // doublings of the head threshold k_head_hist counts
#ifndef SS_HEAD_PIECE
#define SS_HEAD_PIECE 2048
#endif
constexpr int HEAD_PIECE = SS_HEAD_PIECE;      // head postings a wave of k_bucket_sum takes at a time
static_assert(SC_CH <= 65535, "staging positions are 16-bit");
static_assert(SC_CH % CH == 0 || CH % SC_CH == 0, "a range must be whole chunks of both passes");

// dynamic LDS of k_scatter (nbt = the bucket count rounded up to even; layout: see the kernel) and of k_bucket_sum
inline size_t scatter_lds_bytes(uint32_t nbt) { return (size_t)SC_CH * 8 + (size_t)nbt * 8 + 64; }
inline size_t bucket_lds_bytes(int shift) { return ((size_t)1 << shift) * 8 + (size_t)(3 * HEAD_CAP + 4) * 4; }

// ---- options ("tfidf.<name>" of ss_set_option; the driver fills this from the context) ------------------------------------------------
struct Options {
    int64_t blocks = 4096;                     // ranges the postings are cut into (at least 1)
    int64_t bucket_shift = 13;                 // 8192 docs per bucket = 64 KB of float64 LDS accumulators; clamped to 10 .. 14
    int64_t head_min_run = 64;                 // a head list averages at least this many postings per bucket; <= 0 switches the head path off
    int64_t bucket_min = (int64_t)1 << 22;     // (tests, A/B) smallest table that takes the bucketed pass; a huge value forces the atomics
};

struct Plan {
    bool bucketed = false;                     // bucketed magnitude pass (no global float64 atomics); otherwise one atomic per posting
    int shift = 13;                            // a bucket holds 2^shift consecutive docs
    bool shift_forced = false;                 // the option's shift would give NB_MAX buckets or more: 14 whatever it says
    uint32_t nb = 0;                           // buckets
    // ---- the rest: bucketed tables only (0 otherwise) ----
    uint64_t per = 0;                          // postings of a block's range: a multiple of both passes' chunk sizes
    uint32_t nblk = 0;                         // ranges = blocks of k_weight_count and k_scatter
    uint64_t head_thr = 0;                     // shortest list that takes the head path; 0 = no head path
    uint32_t bpt = 0, nbt = 0;                 // buckets per owner thread of k_scatter and the bucket count, both rounded up to even
    int bpt_inst = 0;                          // the k_scatter<W, BPT> instance: 2, 4 or SC_BPT_MAX
    size_t scatter_lds_bytes = 0, bucket_lds_bytes = 0;
    bool too_many_buckets = false;             // more buckets per owner thread than any instance keeps cursors for: the driver refuses
};

inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

inline Plan make_plan(uint64_t n_docs, uint64_t n_post, const Options& o) {
    Plan p;
    p.shift = (int)std::max<int64_t>(10, std::min<int64_t>(14, o.bucket_shift));
    p.shift_forced = (n_docs >> p.shift) >= (uint64_t)NB_MAX;
    if (p.shift_forced) p.shift = 14;
    const uint64_t nb64 = div_up(std::max<uint64_t>(n_docs, 1), (uint64_t)1 << p.shift);
    p.nb = (uint32_t)nb64;
    const uint64_t min_p = (uint64_t)o.bucket_min;                           // (unsigned: a negative value is a huge one)
    p.bucketed = n_post >= std::max<uint64_t>(min_p, 1) && n_post < ((uint64_t)1 << 32) && nb64 <= (uint64_t)NB_MAX;
    if (!p.bucketed) return p;
    // blocks own contiguous ranges whose length is a multiple of both passes' chunk sizes
    const uint64_t unit = std::max<uint64_t>(SC_CH, CH);
    const uint64_t target_blocks = (uint64_t)std::max<int64_t>(1, o.blocks);
    p.per = std::max<uint64_t>(unit, div_up(div_up(n_post, target_blocks), unit) * unit);
    p.nblk = (uint32_t)div_up(n_post, p.per);
    // head lists: an average run of at least head_min_run postings per bucket, and longer than two chunks of either pass (head_skip
    // relies on it)
    p.head_thr = o.head_min_run > 0 ? std::max<uint64_t>((uint64_t)o.head_min_run * p.nb, 2 * unit + 1) : 0;
    p.bpt = ((uint32_t)div_up(p.nb, (uint32_t)SC_TPB) + 1u) & ~1u;           // even: a thread's buckets are whole words of the packed counts
    p.nbt = (p.nb + 1u) & ~1u;
    p.too_many_buckets = p.bpt > (uint32_t)SC_BPT_MAX;
    // The owner threads' cursor registers are sized by the instance.  bpt > 4 takes more than 4 * SC_TPB buckets: with nb <= NB_MAX
    // that is a variant build of fewer than NB_MAX / 4 threads (SS_SC_TPB = 512: 6 or 8 buckets per thread above 2048 buckets, the
    // instance of 8).  At the product's 1024 threads bpt is 2 up to 2048 buckets and 4 beyond, and SC_BPT_MAX is 4: the third
    // instance is the second.
    p.bpt_inst = p.bpt <= 2 ? 2 : p.bpt <= 4 ? 4 : SC_BPT_MAX;
    p.scatter_lds_bytes = scatter_lds_bytes(p.nbt);
    p.bucket_lds_bytes = bucket_lds_bytes(p.shift);
    return p;
}

}  // namespace tfidf
}  // namespace ss
