// match_set.hpp — the HIP side of what ss_facet_counts (facet.hip), ss_field_topk (field_topk.hip), ss_top_groups (group_topk.hip) and
// ss_field_stats / ss_field_histogram (field_stats.hip) share; match_set_plan.hpp holds the pure host part.  DESIGN.md "K4s–u shared
// match-set code".
//
// M(q) = (the docs with a posting of any usable query term, title or body) AND (the allowed set ss_score_topk_filtered builds for the
// query's mask id, required / excluded terms and range clauses) AND d < n_docs.  These calls form it by this file alone: one host
// prologue (open_match_call: the list table and the allowed sets), one layout of the tables a kernel reads (stage_match_tables ->
// MatchSetArgs) and one device walk of a 32768-doc block (steps 1 to 3 below).  So they agree about M(q) by construction;
// test_agrees_with_facet_counts* check that it stays so.
//
//   host    build_match_lists, open_match_call, stage_match_tables, plan_code
//   device  lower_doc, lower_doc_from, wave_sum; runs_cold / runs_warm, or_image, and_allowed; BestK
//
// The block walk, by the THREADS threads of a workgroup over caller-owned LDS cur[MAX_LISTS][2] and img[BLOCK_WORDS]:
//   1. runs_cold (the first block of a workgroup) or runs_warm (the block behind the last one): cur[l] = list l's postings in the block.
//      No barrier inside.
//   2. or_image: a barrier (cur is written), then a vote.  No list reaches the block: false in every thread, img untouched.  Else img is
//      zeroed, a barrier, the runs are ORed in, a barrier: img is complete and cur is read no more, so the next runs_warm may follow
//      without another barrier.
//   3. and_allowed: a thread's own four words of img, ANDed with the allowed row and d < n_docs, into registers.  No barrier, and no
//      thread reads another's words: a caller may store its words back to its own slots of img without one.  The barrier at the head of
//      the next or_image stands between any such use of img and its zeroing.
// What a kernel does when or_image says false or when no thread has a bit left (return, continue) is the kernel's.
#pragma once
#include "hit_window.hpp"
#include "match_set_plan.hpp"
#include "scorer.hpp"

#include <algorithm>

namespace ss {

static_assert(mset::MAX_LISTS == 2 * SS_MAX_QUERY_TERMS && mset::MAX_K == SS_MAX_TOPK, "match_set_plan.hpp restates the ABI's limits");

struct __attribute__((aligned(16))) MatchList { uint64_t b; uint32_t len, field; };   // postings [b, b + len) of the title (field 1) or body (0) table
static_assert(sizeof(MatchList) == 16, "list table layout");

// what the block walk reads: the head of every match-set kernel's parameters
struct MatchSetArgs {
    const uint32_t* t_doc;            // the tables' post_doc (strictly ascending inside a term)
    const uint32_t* b_doc;
    const uint32_t* lptr;             // [n_active + 1] the active queries' lists in `lists`
    const int32_t* qset;              // [n_active] row of `allowed`, -1: every doc
    const MatchList* lists;
    const uint32_t* allowed;          // [..][allowed_stride]
    uint64_t allowed_stride;
    uint64_t n_docs;
};

// ---------------------------------------------------------------- host side
inline int32_t plan_code(int rc) { return rc == mset::INVALID ? SS_ERR_INVALID : rc == mset::UNSUPPORTED ? SS_ERR_UNSUPPORTED : SS_ERR_STATE; }

struct MatchLists {
    std::vector<uint32_t> aq;                   // the queries that have a list, ascending
    std::vector<uint32_t> lptr{0u};             // [aq.size() + 1] their lists in `lists`
    std::vector<MatchList> lists;
};

// qptr [nq + 1] and terms: host copies, already checked.  A repeated term counts once; ids >= n_terms have no list.  More than
// SS_MAX_QUERY_TERMS distinct usable terms in a query: SS_ERR_UNSUPPORTED under `entry`'s name, as the scoring calls refuse them.
inline int32_t build_match_lists(ss_scorer* s, const char* entry, const uint32_t* qptr, const uint32_t* terms, size_t nq, MatchLists* out) {
    const std::vector<uint64_t>& tp = s->title->h_term_ptr;
    const std::vector<uint64_t>& bp = s->body->h_term_ptr;
    std::vector<uint32_t> dterm;
    for (size_t q = 0; q < nq; q++) {
        dterm.clear();
        for (uint32_t i = qptr[q]; i < qptr[q + 1]; i++) {
            const uint32_t t = terms[i];
            if ((uint64_t)t >= s->n_terms || std::find(dterm.begin(), dterm.end(), t) != dterm.end()) continue;
            dterm.push_back(t);
        }
        if (dterm.size() > SS_MAX_QUERY_TERMS)
            return s->ctx->fail(SS_ERR_UNSUPPORTED, "%s: query %zu has more than %d distinct terms", entry, q, SS_MAX_QUERY_TERMS);
        const size_t before = out->lists.size();
        for (const uint32_t t : dterm)
            for (uint32_t field = 0; field < 2; field++) {
                const uint64_t* const pp = field ? tp.data() : bp.data();
                if (pp[t + 1] > pp[t]) out->lists.push_back(MatchList{pp[t], (uint32_t)(pp[t + 1] - pp[t]), field});   // (a list is shorter than 2^32: ss_index_create)
            }
        if (out->lists.size() > before) {
            out->aq.push_back((uint32_t)q);
            out->lptr.push_back((uint32_t)out->lists.size());
        }
    }
    return SS_OK;
}

// The part of a call that says what M(q) is: the list table and the allowed sets.
struct MatchCall {
    MatchLists ml;
    AllowedSets as;
};
// The last checks of a call, in this order: q_ptr fetched and checked, q_terms, the list table, then the mask ids, constraint arrays and
// range clauses by the scoring call's own checks, which takes a plan turn and puts the sets on the device.  Nothing is enqueued before
// the last check has passed; nothing behind this function refuses an argument.  The caller has set the device.
inline int32_t open_match_call(ss_scorer* s, const char* entry, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                               const QueryConstraints& cons, const QueryRanges& ranges, MatchCall* mc) {
    ss_ctx* ctx = s->ctx;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> qptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, entry, "q", q_ptr, nq, qptr.data()));
    const uint32_t n_tok = qptr[nq];
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "%s: q_terms is NULL", entry);
    std::vector<uint32_t> terms(n_tok);
    if (n_tok) SS_HIP(ctx, ss::copy_in(ctx->stream, terms.data(), q_terms, n_tok * sizeof(uint32_t)));
    SS_TRY(build_match_lists(s, entry, qptr.data(), terms.data(), nq, &mc->ml));
    return allowed_sets_into_turn(s, n_q, q_ptr, mask_id, &cons, &ranges, &mc->as);
}

// The call's tables on the device, through the pinned block of the call's turn: active queries | list offsets | sets | lists | extra
// (each 16-byte aligned; `extra`: extra_bytes the caller's kernel reads beside them, ss_facet_counts' BucketTable).  The caller records
// the turn's batch_ev behind the last kernel that reads them.
struct MatchTables {
    MatchSetArgs args;
    const uint32_t* aq = nullptr;               // device: [n_active] the queries that have a list
    const unsigned char* extra = nullptr;       // device
};
inline int32_t stage_match_tables(ss_scorer* s, const MatchCall& mc, const void* extra, size_t extra_bytes, MatchTables* out) {
    ss_ctx* ctx = s->ctx;
    Turn& turn = s->turn[mc.as.turn];
    const MatchLists& ml = mc.ml;
    const size_t n_active = ml.aq.size();
    std::vector<int32_t> qset(n_active);
    for (size_t i = 0; i < n_active; i++) qset[i] = mc.as.set_of[ml.aq[i]];
    const size_t o_lptr = align16(n_active * sizeof(uint32_t)), o_qset = align16(o_lptr + (n_active + 1) * sizeof(uint32_t)),
                 o_lists = align16(o_qset + n_active * sizeof(int32_t)), o_extra = align16(o_lists + ml.lists.size() * sizeof(MatchList)),
                 bytes = extra_bytes ? o_extra + extra_bytes : o_lists + ml.lists.size() * sizeof(MatchList);
    SS_HIP(ctx, turn.h_facet.ensure(bytes));
    SS_HIP(ctx, ensure(turn.d_facet, bytes));
    unsigned char* const h = turn.h_facet.p;
    std::memcpy(h, ml.aq.data(), n_active * sizeof(uint32_t));
    std::memcpy(h + o_lptr, ml.lptr.data(), (n_active + 1) * sizeof(uint32_t));
    std::memcpy(h + o_qset, qset.data(), n_active * sizeof(int32_t));
    std::memcpy(h + o_lists, ml.lists.data(), ml.lists.size() * sizeof(MatchList));
    if (extra_bytes) std::memcpy(h + o_extra, extra, extra_bytes);
    SS_HIP(ctx, hipMemcpyAsync(turn.d_facet.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    const unsigned char* const d = turn.d_facet.p;
    out->args.t_doc = s->title->post_doc.p;
    out->args.b_doc = s->body->post_doc.p;
    out->args.lptr = reinterpret_cast<const uint32_t*>(d + o_lptr);
    out->args.qset = reinterpret_cast<const int32_t*>(d + o_qset);
    out->args.lists = reinterpret_cast<const MatchList*>(d + o_lists);
    out->args.allowed = mc.as.words;
    out->args.allowed_stride = mc.as.stride;
    out->args.n_docs = s->n_docs;
    out->aq = reinterpret_cast<const uint32_t*>(d);
    out->extra = extra_bytes ? d + o_extra : nullptr;
    return SS_OK;
}

// ---------------------------------------------------------------- device side
namespace mset {

// lower bound: the first position in [b, e) whose doc is >= target
__device__ __forceinline__ uint64_t lower_doc(const uint32_t* __restrict__ doc, uint64_t b, uint64_t e, uint64_t target) {
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if ((uint64_t)doc[mid] < target) b = mid + 1;
        else e = mid;
    }
    return b;
}
// the same bound when it is expected near b: probe at growing steps from b, then search the bracket.  Reads doc[x] for x < e only.
__device__ __forceinline__ uint64_t lower_doc_from(const uint32_t* __restrict__ doc, uint64_t b, uint64_t e, uint64_t target, uint64_t step) {
    uint64_t hi = e - b > step ? b + step : e;
    while (hi < e && (uint64_t)doc[hi] < target) {  // every position <= hi lies below the target
        b = hi + 1;
        step <<= 1;
        hi = e - b > step ? b + step : e;
    }
    return lower_doc(doc, b, hi, target);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// ---- 1. the runs of the query's lists [l0, l0 + nl) (1 <= nl <= MAX_LISTS) in block `blk`.  Cold: thread (list, end) searches one bound.
__device__ __forceinline__ void runs_cold(const MatchSetArgs& p, uint32_t l0, uint32_t nl, uint32_t blk, uint64_t (*cur)[2]) {
    const uint32_t tid = threadIdx.x;
    if (tid < 2 * nl) {
        const MatchList fl = p.lists[l0 + (tid >> 1)];
        const uint32_t hi = tid & 1;
        cur[tid >> 1][hi] = lower_doc(fl.field ? p.t_doc : p.b_doc, fl.b, fl.b + fl.len, (uint64_t)blk * BLOCK_DOCS + (hi ? (uint64_t)BLOCK_DOCS : 0));
    }
}
// Warm: cur holds the runs in block blk - 1; a list's run starts at the last one's end, and its end is searched from there at the
// galloping step 2 x the last run's length + 64.
__device__ __forceinline__ void runs_warm(const MatchSetArgs& p, uint32_t l0, uint32_t nl, uint32_t blk, uint64_t (*cur)[2]) {
    const uint32_t tid = threadIdx.x;
    if (tid < nl) {
        const MatchList fl = p.lists[l0 + tid];
        const uint64_t lo = cur[tid][1], len = lo - cur[tid][0];
        cur[tid][0] = lo;
        cur[tid][1] = lower_doc_from(fl.field ? p.t_doc : p.b_doc, lo, fl.b + fl.len, (uint64_t)blk * BLOCK_DOCS + BLOCK_DOCS, 2 * len + 64);
    }
}
// ---- 2. the image: the block's docs with a posting of the query.  false (in every thread alike): no list reaches the block, which
// has then cost the search paths and nothing else.
__device__ __forceinline__ bool or_image(const MatchSetArgs& p, uint32_t l0, uint32_t nl, uint32_t blk, const uint64_t (*cur)[2], uint32_t* img) {
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blk * BLOCK_DOCS;                        // the block's first doc
    __syncthreads();
    if (!__syncthreads_or(tid < nl && cur[tid][0] < cur[tid][1])) return false;
    *reinterpret_cast<uint4*>(&img[tid * WORDS_PER_THREAD]) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t* const doc = p.lists[l0 + l].field ? p.t_doc : p.b_doc;
        const uint64_t e = cur[l][1];
        for (uint64_t j = cur[l][0] + tid; j < e; j += THREADS) {
            const uint32_t d = (uint32_t)((uint64_t)doc[j] - base);
            if (d < BLOCK_DOCS) atomicOr(&img[d >> 5], 1u << (d & 31u));     // (always, for an ascending list: the image is never left)
        }
    }
    __syncthreads();
    return true;
}
// ---- 3. this thread's words w0 .. w0 + 3 of the image (w0 = word_begin(blk): global word numbers) AND the allowed set of active
// query `a` AND d < n_docs.  Returns their bit count.
__device__ __forceinline__ uint64_t word_begin(uint32_t blk) { return (uint64_t)blk * BLOCK_WORDS + (uint64_t)threadIdx.x * WORDS_PER_THREAD; }
__device__ __forceinline__ uint32_t and_allowed(uint32_t (&m)[WORDS_PER_THREAD], const MatchSetArgs& p, uint32_t a, uint32_t blk, const uint32_t* img) {
    const uint64_t w0 = word_begin(blk);
    const uint4 u = *reinterpret_cast<const uint4*>(&img[threadIdx.x * WORDS_PER_THREAD]);
    m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w;
    const int32_t set = p.qset[a];
    if (set >= 0) {
        const uint32_t* const row = p.allowed + (uint64_t)set * p.allowed_stride;
        if ((p.allowed_stride & 3u) == 0 && w0 + WORDS_PER_THREAD <= p.allowed_stride) {   // (rows then start 16-byte aligned)
            const uint4 al = *reinterpret_cast<const uint4*>(row + w0);
            m[0] &= al.x; m[1] &= al.y; m[2] &= al.z; m[3] &= al.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < WORDS_PER_THREAD; i++) m[i] &= w0 + i < p.allowed_stride ? row[w0 + i] : 0u;
        }
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t i = 0; i < WORDS_PER_THREAD; i++) {
        m[i] &= word_valid(w0 + i, p.n_docs);
        cnt += __popc(m[i]);
    }
    return cnt;
}

// ---- The running best-K of a workgroup (match_set_plan.hpp: its size and order): `cap` entries in LDS, a key each and with WITH_DOC a
// doc id, head->cnt of them in use (it may run past cap while threads are refused), and the threshold: the K-th smallest entry once K
// are known, the pad entry before.  Without WITH_DOC there is no doc array: `doc` is never read.
struct BestHead { uint64_t thr_key; uint32_t thr_doc, cnt; };                // in LDS, one per workgroup (thr_doc: WITH_DOC only)
template <bool WITH_DOC>
struct BestK {
    BestHead* head;
    uint64_t* key;                    // [cap]
    uint32_t* doc;                    // [cap], WITH_DOC only
    uint32_t cap, K;

    // dyn: the workgroup's dynamic LDS, cap keys and then, WITH_DOC, cap doc ids.  A barrier must follow before the first drain.
    __device__ __forceinline__ BestK(BestHead* h, unsigned char* dyn, uint32_t cap_, uint32_t K_)
        : head(h), key(reinterpret_cast<uint64_t*>(dyn)), doc(WITH_DOC ? reinterpret_cast<uint32_t*>(dyn + (size_t)cap_ * sizeof(uint64_t)) : nullptr),
          cap(cap_), K(K_) {
        if (threadIdx.x == 0) {
            h->cnt = 0u;
            h->thr_key = PAD_KEY;
            if (WITH_DOC) h->thr_doc = PAD_DOC;
        }
    }
    // false: the buffer is full, the caller keeps the candidate until the next compaction
    __device__ __forceinline__ bool push(uint64_t k, uint32_t d) const {
        const uint32_t pos = atomicAdd(&head->cnt, 1u);
        if (pos >= cap) return false;
        key[pos] = k;
        if (WITH_DOC) doc[pos] = d;
        return true;
    }
    // By all threads, behind a barrier that ends the pushes: the entries sorted, the K smallest kept, the threshold lowered.  Ends behind
    // a barrier.
    __device__ void compact() const {
        const uint32_t n = min(head->cnt, cap);
        const uint32_t np = pow2_at_least(n);       // <= cap, a power of two
        __syncthreads();                            // (everyone has read the count)
        for (uint32_t i = n + threadIdx.x; i < np; i += THREADS) {
            key[i] = PAD_KEY;
            if (WITH_DOC) doc[i] = PAD_DOC;
        }
        __syncthreads();
        hitwin::bitonic_sort<(int)THREADS>(np, [&](uint32_t i, uint32_t o, bool up) {
            const uint64_t ki = key[i], ko = key[o];
            if (WITH_DOC) {
                const uint32_t di = doc[i], dd = doc[o];
                if (key_less(ko, dd, ki, di) == up) {
                    key[i] = ko; key[o] = ki;
                    doc[i] = dd; doc[o] = di;
                }
            } else if ((ko < ki) == up) {
                key[i] = ko;
                key[o] = ki;
            }
        });
        if (threadIdx.x == 0) {
            head->cnt = min(n, K);
            if (n >= K) {
                head->thr_key = key[K - 1];
                if (WITH_DOC) head->thr_doc = doc[K - 1];
            }
        }
        __syncthreads();
    }
    // By all threads: walk(offer) goes on from where this thread's walk stands and calls offer(k, d) for each candidate in turn (d is
    // ignored without WITH_DOC).  offer pushes a candidate that beats the threshold.  offer says false: the buffer is full; the walk
    // stays AT that candidate and returns true, and is called again behind the compaction, against the lowered threshold.  The walk
    // returns false when it has no candidate left.  Returns behind a barrier, every thread's candidates taken in.
    template <typename Walk>
    __device__ __forceinline__ void drain(Walk walk) const {
        uint64_t thr_key = head->thr_key;
        uint32_t thr_doc = WITH_DOC ? head->thr_doc : 0u;
        for (;;) {
            const bool pending = walk([&](uint64_t k, uint32_t d) { return !(WITH_DOC ? key_less(k, d, thr_key, thr_doc) : k < thr_key) || push(k, d); });
            if (!__syncthreads_or(pending)) break;
            compact();
            thr_key = head->thr_key;
            if (WITH_DOC) thr_doc = head->thr_doc;
        }
    }
};

}  // namespace mset
}  // namespace ss
