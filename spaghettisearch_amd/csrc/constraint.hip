// constraint.hip — k_constraint_masks: the per-query allow-lists of ss_score_topk_constrained, built on the device from the
// posting lists of the queries' required and excluded terms (no reference counterpart).
//
// A set's words: allowed = mask(q) AND (every required term: T_t | B_t) AND NOT (any excluded term: T_t | B_t), bit (d & 31) of word
// d >> 5 = doc d, the layout of the registered masks (ss_scorer_set_doc_masks), so that the MASKED scoring kernels read a set
// unchanged.  Every posting list is strictly ascending by doc: the postings of a block's doc range are one contiguous run of each
// list, found by two binary searches per list and block.  A workgroup owns one block of words of one set; it ORs a term's runs into
// an LDS image of the block, combines the image into the words it keeps in registers, and writes every word exactly once with
// vector stores.  No global atomics, no order dependence: the words are a function of the lists alone.
#include "scorer.hpp"

namespace {

constexpr int CM_TPB = 256;                     // threads
constexpr int CM_WPT = 4;                       // words of a thread (one 16-byte store)
constexpr int CM_WORDS = CM_TPB * CM_WPT;       // words of a block: 32768 docs
constexpr int CM_LISTS = 2 * SS_MAX_CONSTRAINT_TERMS;

// lower bound: the first position in [b, e) whose doc is >= target
__device__ __forceinline__ uint64_t lower_doc(const uint32_t* __restrict__ doc, uint64_t b, uint64_t e, uint64_t target) {
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if ((uint64_t)doc[mid] < target) b = mid + 1;
        else e = mid;
    }
    return b;
}

__global__ __launch_bounds__(CM_TPB) void k_constraint_masks(ConstraintParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t img[CM_WORDS];   // one term's docs in this block (title | body)
    __shared__ uint64_t cur[CM_LISTS][2];                             // each list's run in this block: [first, end)
    const int tid = threadIdx.x;
    const uint32_t set = blockIdx.x / p.n_blocks, blk = blockIdx.x - set * p.n_blocks;
    const ConstraintSet cs = p.sets[set];
    const uint64_t w0 = (uint64_t)blk * CM_WORDS + (uint64_t)tid * CM_WPT;          // this thread's first word
    const uint64_t base = (uint64_t)blk * CM_WORDS * 32;                            // the block's first doc
    uint32_t acc[CM_WPT];
    const bool empty = cs.mask1 == CS_EMPTY;
#pragma unroll
    for (int i = 0; i < CM_WPT; i++) {
        const uint64_t w = w0 + i;
        acc[i] = empty ? 0u : cs.mask1 && w < p.n_words ? p.reg_masks[(uint64_t)(cs.mask1 - 1u) * p.reg_words + w] : ~0u;
    }
    const uint32_t n_terms = empty ? 0u : cs.n_req + cs.n_exc;
    if (n_terms) {
        const ConstraintTerm* const terms = p.terms + cs.t0;
        // the cursors: thread (term, field, end) searches one bound; at most 2 x 16 lists, 64 searches side by side
        if ((uint32_t)tid < 4 * n_terms) {
            const ConstraintTerm& ct = terms[tid >> 2];
            const int field = (tid >> 1) & 1, hi = tid & 1;
            const uint32_t* doc = field ? p.t_doc : p.b_doc;
            const uint64_t b = field ? ct.t_b : ct.b_b, e = field ? ct.t_e : ct.b_e;
            cur[tid >> 1][hi] = lower_doc(doc, b, e, base + (hi ? (uint64_t)CM_WORDS * 32 : 0));
        }
        for (uint32_t t = 0; t < n_terms; t++) {
            *reinterpret_cast<uint4*>(&img[tid * CM_WPT]) = make_uint4(0u, 0u, 0u, 0u);   // (only this thread reads these words)
            __syncthreads();
#pragma unroll
            for (int field = 0; field < 2; field++) {
                const uint32_t* doc = field ? p.t_doc : p.b_doc;
                const uint64_t e = cur[2 * t + field][1];
                for (uint64_t j = cur[2 * t + field][0] + tid; j < e; j += CM_TPB) {
                    const uint32_t d = (uint32_t)((uint64_t)doc[j] - base);
                    atomicOr(&img[d >> 5], 1u << (d & 31u));                              // LDS: the block's own image
                }
            }
            __syncthreads();
            const uint4 u = *reinterpret_cast<const uint4*>(&img[tid * CM_WPT]);
            const uint32_t uw[CM_WPT] = {u.x, u.y, u.z, u.w};
            const bool req = t < cs.n_req;
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < CM_WPT; i++) {
                acc[i] &= req ? uw[i] : ~uw[i];
                any |= acc[i];
            }
            if (!__syncthreads_or(any != 0)) break;     // nothing of the block left: the other terms cannot add a doc back
        }
    }
    uint32_t* const out = p.out + (uint64_t)set * p.stride;
    if (w0 + CM_WPT <= p.stride) {                      // (stride: a multiple of 4 words, so a set's start is 16-byte aligned)
        *reinterpret_cast<uint4*>(out + w0) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int i = 0; i < CM_WPT; i++)
            if (w0 + i < p.stride) out[w0 + i] = acc[i];
    }
}

}  // namespace

namespace ss {

uint32_t constraint_blocks(uint64_t n_words) { return (uint32_t)((n_words + CM_WORDS - 1) / CM_WORDS); }

void launch_constraint_masks(const void* params, uint32_t n_sets, hipStream_t st) {
    const ConstraintParams& p = *static_cast<const ConstraintParams*>(params);
    if (!n_sets || !p.n_blocks) return;
    hipLaunchKernelGGL(k_constraint_masks, dim3(n_sets * p.n_blocks), dim3(CM_TPB), 0, st, p);
}

}  // namespace ss
