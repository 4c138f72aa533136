// group_topk.hip — ss_top_groups and ss_scorer_group_values: the m groups ("sites") of the doc -> group table that hold most of a
// query's matches, counted over ALL docs the query matches.  DESIGN.md K4u; no reference counterpart.
//
// The group ranks turn every 32-bit group value into an array index: gval = the table's distinct values != SS_NO_GROUP ascending (a
// rocprim sort of a copy of the table and a unique pass), grank[d] = the index of group[d] in gval (k_group_ranks, a binary search per
// doc).  They are built by the first call that needs them after ss_scorer_set_doc_groups, which waits once, and dropped with the table.
//
// M(q) is ss_facet_counts' match set.  k_group_count gives a workgroup a RUN of consecutive 32768-doc blocks of one query and forms the
// match words per block as k_field_select does (steps 1 to 3: a private copy, as that kernel's are of k_facet_counts').  For every set
// bit it gathers grank[d]; a thread walks its 128 docs in ascending order and merges consecutive equal ranks into one add.  The adds go
// to a histogram in LDS that joins the query's counter row at the end of the run (tables of at most "gtopk.lds_groups" values), or
// straight to the row by non-returning global atomics.  The row's two extra slots take the run's matches and its SS_NO_GROUP matches.
// k_group_select, one workgroup per query, streams the row, pushes key = (0xFFFFFFFF - cnt) << 32 | rank of every non-zero counter
// through a running best first + m (the threshold and the buffer compacted by an exact bitonic sort of field_topk.hip, here over keys
// alone: a private copy) and writes the page.  Integer atomics only, and a total order of the keys: no arrival order can show.
#include "group_topk_plan.hpp"
#include "hit_window.hpp"
#include "match_lists.hpp"

#include <rocprim/rocprim.hpp>

namespace gp = ss::gtopk;
namespace hw = ss::hitwin;

static_assert(gp::MAX_K == SS_MAX_TOPK && gp::NO_RANK == SS_NO_GROUP, "group_topk_plan.hpp restates the ABI's limits");
static_assert(sizeof(ss_group_count) == 8, "ss_group_count layout");

namespace {

constexpr int GT_TPB = (int)gp::THREADS;
constexpr int GT_WPT = 4;                           // words of a thread (one 16-byte LDS / global load)
constexpr int GT_WAVES = GT_TPB / 64;
constexpr uint32_t GT_MAX_LISTS = ss::ftopk::MAX_LISTS;
static_assert(GT_TPB * GT_WPT == (int)gp::BLOCK_WORDS && GT_TPB == 2 * (int)GT_MAX_LISTS, "block geometry");

using ss::MatchList;

struct CountParams {
    const uint32_t* t_doc;            // the tables' post_doc (strictly ascending inside a term)
    const uint32_t* b_doc;
    const uint32_t* lptr;             // [n_active + 1] the active queries' lists in `lists`
    const int32_t* qset;              // [n_active] row of `allowed`, -1: every doc
    const MatchList* lists;
    const uint32_t* allowed;          // [..][allowed_stride]
    uint64_t allowed_stride;
    const uint32_t* grank;            // [n_docs]
    uint64_t n_docs;
    uint32_t n_blocks, R, n_groups;
    uint32_t a0, n_group, run0;       // this launch: active queries [a0, a0 + n_group), runs from run0
    uint64_t stride;                  // words of a counter row
    uint32_t* rows;                   // [n_group][stride], zeroed
};

struct SelectParams {
    const uint32_t* aq;               // [n_active] the queries that have a list
    const uint32_t* rows;
    const uint32_t* gval;             // [n_groups]
    uint64_t stride;
    uint32_t n_groups, K, cap, first, m, a0;
    ss_group_count* groups_out;       // [n_q][m]
    int32_t* n_out;                   // [n_q]
    uint32_t* n_groups_out;           // [n_q], nullable
    uint32_t* n_ungrouped_out;        // [n_q], nullable
    uint32_t* n_match_out;            // [n_q], nullable
};

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

// grank[d] = the index of group[d] in gval [n_groups] (ascending, distinct; every value of the table != SS_NO_GROUP is in it)
__global__ __launch_bounds__(GT_TPB) void k_group_ranks(const uint32_t* __restrict__ group, const uint32_t* __restrict__ gval, uint32_t n_groups,
                                                        uint64_t n_docs, uint32_t* __restrict__ grank) {
    const uint64_t d = (uint64_t)blockIdx.x * GT_TPB + threadIdx.x;
    if (d >= n_docs) return;
    const uint32_t v = group[d];
    uint32_t lo = 0, hi = n_groups;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (gval[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    grank[d] = v != SS_NO_GROUP && lo < n_groups ? lo : gp::NO_RANK;
}

// Grid: blockIdx.x = (run - run0) * n_group + query — the queries of one run are neighbours, so the run's allowed words and ranks come
// from L2 for all but the first of them.  LDS: dynamic LDS holds the histogram, n_groups counters rounded up to four.
template <bool LDS>
__global__ __launch_bounds__(GT_TPB) void k_group_count(CountParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t gt_hist[];
    __shared__ uint64_t cur[GT_MAX_LISTS][2];                                // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[gp::BLOCK_WORDS];   // the block's docs with a posting of the query
    __shared__ uint32_t wsum[GT_WAVES][2];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.lptr[a], nl = p.lptr[a + 1] - l0;                  // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint32_t b0 = gp::run_begin(r, p.R, p.n_blocks), b1 = gp::run_begin(r + 1, p.R, p.n_blocks);
    uint32_t* const row = p.rows + (uint64_t)al * p.stride;
    if (LDS) {
        for (uint32_t i = tid; i < p.n_groups; i += GT_TPB) gt_hist[i] = 0u;   // (the barrier of step 1 stands before the first add)
    }
    uint32_t matches = 0, ungrouped = 0;                                     // of this thread's words, over the run
    for (uint32_t blk = b0; blk < b1; blk++) {
        const uint64_t base = (uint64_t)blk * gp::BLOCK_DOCS;                // the block's first doc
        // ---- 1. the runs: cold at the head of the run (thread (list, end) searches one bound), from the last block's end after it
        if (blk == b0) {
            if ((uint32_t)tid < 2 * nl) {
                const MatchList fl = p.lists[l0 + (tid >> 1)];
                const int hi = tid & 1;
                cur[tid >> 1][hi] = lower_doc(fl.field ? p.t_doc : p.b_doc, fl.b, fl.b + fl.len, base + (hi ? (uint64_t)gp::BLOCK_DOCS : 0));
            }
        } else if ((uint32_t)tid < nl) {
            const MatchList fl = p.lists[l0 + tid];
            const uint64_t lo = cur[tid][1], len = lo - cur[tid][0];
            cur[tid][0] = lo;
            cur[tid][1] = lower_doc_from(fl.field ? p.t_doc : p.b_doc, lo, fl.b + fl.len, base + gp::BLOCK_DOCS, 2 * len + 64);
        }
        __syncthreads();
        // a block no list reaches is left here: it has read the search paths and nothing else
        if (!__syncthreads_or((uint32_t)tid < nl && cur[tid][0] < cur[tid][1])) continue;
        // ---- 2. the image
        *reinterpret_cast<uint4*>(&img[tid * GT_WPT]) = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t* const doc = p.lists[l0 + l].field ? p.t_doc : p.b_doc;
            const uint64_t e = cur[l][1];
            for (uint64_t j = cur[l][0] + tid; j < e; j += GT_TPB) {
                const uint32_t d = (uint32_t)((uint64_t)doc[j] - base);
                if (d < gp::BLOCK_DOCS) atomicOr(&img[d >> 5], 1u << (d & 31u));   // (always, for an ascending list: the image is never left)
            }
        }
        __syncthreads();
        // ---- 3. AND the allowed set and d < n_docs (each thread reads its own words only)
        const uint64_t w0 = (uint64_t)blk * gp::BLOCK_WORDS + (uint64_t)tid * GT_WPT;   // this thread's first word
        const uint4 u = *reinterpret_cast<const uint4*>(&img[tid * GT_WPT]);
        uint32_t m[GT_WPT] = {u.x, u.y, u.z, u.w};
        const int32_t set = p.qset[a];
        if (set >= 0) {
            const uint32_t* const arow = p.allowed + (uint64_t)set * p.allowed_stride;
            if ((p.allowed_stride & 3u) == 0 && w0 + GT_WPT <= p.allowed_stride) {      // (rows then start 16-byte aligned)
                const uint4 al4 = *reinterpret_cast<const uint4*>(arow + w0);
                m[0] &= al4.x; m[1] &= al4.y; m[2] &= al4.z; m[3] &= al4.w;
            } else {
#pragma unroll
                for (int i = 0; i < GT_WPT; i++) m[i] &= w0 + i < p.allowed_stride ? arow[w0 + i] : 0u;
            }
        }
        // ---- 4. the ranks of the set bits, ascending by doc: consecutive equal ranks become one add
        uint32_t run_rank = gp::NO_RANK, run_len = 0;
#pragma unroll
        for (int i = 0; i < GT_WPT; i++) {
            uint32_t bits = m[i] & gp::word_valid(w0 + i, p.n_docs);
            matches += __popc(bits);
            while (bits) {
                const uint32_t d = (uint32_t)((w0 + i) * 32) + (uint32_t)(__ffs(bits) - 1);      // < n_docs < 2^32
                bits &= bits - 1;
                const uint32_t rk = p.grank[d];                                                  // < n_groups, or NO_RANK
                if (rk == run_rank) {
                    run_len++;
                    continue;
                }
                if (run_rank == gp::NO_RANK) ungrouped += run_len;
                else if (LDS) atomicAdd(&gt_hist[run_rank], run_len);
                else atomicAdd(&row[run_rank], run_len);
                run_rank = rk;
                run_len = 1;
            }
        }
        if (run_rank == gp::NO_RANK) ungrouped += run_len;
        else if (LDS) atomicAdd(&gt_hist[run_rank], run_len);
        else atomicAdd(&row[run_rank], run_len);
    }
    // ---- the run's histogram and its two totals join the row
    matches = wave_sum(matches);
    ungrouped = wave_sum(ungrouped);
    if ((tid & 63) == 0) {
        wsum[tid >> 6][0] = matches;
        wsum[tid >> 6][1] = ungrouped;
    }
    __syncthreads();
    if (LDS) {
        for (uint32_t i = tid; i < p.n_groups; i += GT_TPB) {
            const uint32_t c = gt_hist[i];
            if (c) atomicAdd(&row[i], c);
        }
    }
    if (tid < 2) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < GT_WAVES; w++) v += wsum[w][tid];
        if (v) atomicAdd(&row[p.n_groups + tid], v);                         // slot_match, slot_ungrouped
    }
}

// The running best-K of a workgroup over keys alone (field_topk.hip's Best without the doc word): `cap` keys in LDS, *cnt of them in use
// (it may run past cap while threads are refused), and the threshold: the K-th smallest key once K are known, the pad key before.
struct Best {
    uint64_t* key;
    uint32_t* cnt;
    uint64_t* thr;
    uint32_t cap, K;
};
// false: the buffer is full, the caller keeps the candidate until the next compaction
__device__ __forceinline__ bool best_push(const Best& b, uint64_t key) {
    const uint32_t pos = atomicAdd(b.cnt, 1u);
    if (pos >= b.cap) return false;
    b.key[pos] = key;
    return true;
}
// By all threads, behind a barrier that ends the pushes: the keys sorted, the K smallest kept, the threshold lowered.  Ends behind a
// barrier.
__device__ void best_compact(const Best& b) {
    const uint32_t n = min(*b.cnt, b.cap);
    const uint32_t np = gp::pow2_at_least(n);       // <= cap, a power of two
    __syncthreads();                                // (everyone has read the count)
    for (uint32_t i = n + threadIdx.x; i < np; i += GT_TPB) b.key[i] = gp::PAD_KEY;
    __syncthreads();
    hw::bitonic_sort<GT_TPB>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t ki = b.key[i], ko = b.key[o];
        if ((ko < ki) == up) {
            b.key[i] = ko;
            b.key[o] = ki;
        }
    });
    if (threadIdx.x == 0) {
        *b.cnt = min(n, b.K);
        if (n >= b.K) *b.thr = b.key[b.K - 1];
    }
    __syncthreads();
}

// Grid: one workgroup per active query of the group.  Dynamic LDS: cap keys.
__global__ __launch_bounds__(GT_TPB) void k_group_select(SelectParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gt_dyn[];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t wsum[GT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x, q = p.aq[p.a0 + al];
    const Best best{reinterpret_cast<uint64_t*>(gt_dyn), &s_cnt, &s_thr, p.cap, p.K};
    if (tid == 0) {
        s_cnt = 0u;
        s_thr = gp::PAD_KEY;
    }
    __syncthreads();
    const uint32_t* const row = p.rows + (uint64_t)al * p.stride;            // 16-byte aligned: the stride is a multiple of four words
    const uint4* const row4 = reinterpret_cast<const uint4*>(row);
    const uint64_t n4 = ((uint64_t)p.n_groups + 3) >> 2;                     // <= stride / 4
    uint64_t thr = gp::PAD_KEY;
    uint64_t x = (uint64_t)tid;
    uint32_t j = 0, nz = 0;
    for (;;) {
        bool pending = false;
        for (; x < n4; x += GT_TPB, j = 0) {
            const uint4 u = row4[x];
            const uint32_t c[4] = {u.x, u.y, u.z, u.w};
            for (; j < 4; j++) {
                const uint64_t idx = x * 4 + j;
                if (idx >= p.n_groups || !c[j]) continue;                    // (the two extra slots and the padding are no counters)
                const uint64_t key = gp::pack_key(c[j], (uint32_t)idx);
                if (key < thr && !best_push(best, key)) {
                    pending = true;
                    break;
                }
                nz++;
            }
            if (pending) break;
        }
        if (!__syncthreads_or(pending)) break;
        best_compact(best);
        thr = s_thr;
    }
    best_compact(best);
    const uint32_t n_page = hw::page_len(s_cnt, p.first, p.m);
    for (uint32_t i = tid; i < n_page; i += GT_TPB) {
        const uint64_t key = best.key[p.first + i];
        p.groups_out[(uint64_t)q * p.m + i] = ss_group_count{p.gval[gp::key_rank(key)], gp::key_count(key)};
    }
    nz = wave_sum(nz);
    if ((tid & 63) == 0) wsum[tid >> 6] = nz;
    __syncthreads();
    if (tid == 0) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < GT_WAVES; w++) v += wsum[w];
        p.n_out[q] = (int32_t)n_page;
        if (p.n_groups_out) p.n_groups_out[q] = v;
        if (p.n_ungrouped_out) p.n_ungrouped_out[q] = row[gp::slot_ungrouped(p.n_groups)];
        if (p.n_match_out) p.n_match_out[q] = row[gp::slot_match(p.n_groups)];
    }
}

int32_t plan_code(int rc) { return rc == gp::INVALID ? SS_ERR_INVALID : rc == gp::UNSUPPORTED ? SS_ERR_UNSUPPORTED : SS_ERR_STATE; }

// The group ranks of the registered table, built if they are missing (the caller holds the context's lock and has set the device).
// Waits for the context's stream once when it builds.
int32_t ensure_group_ranks(ss_scorer* s) {
    ss_ctx* ctx = s->ctx;
    if (s->has_group_ranks) return SS_OK;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)s->n_docs;
    uint32_t n_groups = 0;
    ss::DevBuf<uint32_t> gval, grank;
    if (n) {
        ss::DevBuf<uint32_t> sorted, uniq, n_uniq;
        ss::DevBuf<unsigned char> tmp;
        SS_HIP(ctx, sorted.alloc(n));
        SS_HIP(ctx, uniq.alloc(n));
        SS_HIP(ctx, n_uniq.alloc(2));
        size_t sort_bytes = 0, uniq_bytes = 0;
        SS_HIP(ctx, rocprim::radix_sort_keys(nullptr, sort_bytes, (const uint32_t*)s->groups.p, sorted.p, n, 0u, 32u, st));
        SS_HIP(ctx, rocprim::unique(nullptr, uniq_bytes, sorted.p, uniq.p, n_uniq.p, n, rocprim::equal_to<uint32_t>(), st));
        SS_HIP(ctx, tmp.alloc(std::max(sort_bytes, uniq_bytes)));
        SS_HIP(ctx, rocprim::radix_sort_keys(tmp.p, sort_bytes, (const uint32_t*)s->groups.p, sorted.p, n, 0u, 32u, st));
        SS_HIP(ctx, rocprim::unique(tmp.p, uniq_bytes, sorted.p, uniq.p, n_uniq.p, n, rocprim::equal_to<uint32_t>(), st));
        // the largest value of the table sorts last: SS_NO_GROUP, if any doc has it, is the last distinct value and is left out
        uint32_t h_uniq = 0, h_last = 0;
        SS_HIP(ctx, ss::fetch(ctx, st, &h_uniq, n_uniq.p, sizeof(uint32_t), &h_last, sorted.p + (n - 1), sizeof(uint32_t)));
        n_groups = h_last == SS_NO_GROUP ? h_uniq - 1 : h_uniq;
        SS_HIP(ctx, gval.alloc(n_groups));
        SS_HIP(ctx, grank.alloc(n));
        if (n_groups) SS_HIP(ctx, hipMemcpyAsync(gval.p, uniq.p, (size_t)n_groups * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_group_ranks, dim3(ss::div_up(n, GT_TPB)), dim3(GT_TPB), 0, st, (const uint32_t*)s->groups.p, (const uint32_t*)gval.p,
                           n_groups, (uint64_t)n, grank.p);
        SS_HIP(ctx, hipGetLastError());
        SS_HIP(ctx, hipStreamSynchronize(st));      // the temporaries go back to the pool behind their last reader
    }
    s->gval = std::move(gval);
    s->grank = std::move(grank);
    s->n_groups = n_groups;
    s->has_group_ranks = true;
    return SS_OK;
}

int32_t group_values_impl(ss_scorer* s, uint32_t* n_groups_out, uint32_t* values_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!s->has_groups) return ctx->fail(SS_ERR_STATE, "ss_scorer_group_values: no group table registered (ss_scorer_set_doc_groups)");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    SS_TRY(ensure_group_ranks(s));
    if (n_groups_out) *n_groups_out = s->n_groups;
    if (values_out && s->n_groups) {
        SS_HIP(ctx, hipMemcpyAsync(values_out, s->gval.p, (size_t)s->n_groups * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
        SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SS_OK;
}

int32_t top_groups_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id, const QueryConstraints& cons,
                        const QueryRanges& ranges, int32_t first, int32_t m, ss_group_count* groups_out, int32_t* n_out, uint32_t* n_groups_out,
                        uint32_t* n_ungrouped_out, uint32_t* n_match_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_top_groups";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = gp::check_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, groups_out != nullptr, n_out != nullptr, first, m, s->has_groups))
        return ctx->fail(plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> qptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, entry, "q", q_ptr, nq, qptr.data()));
    const uint32_t n_tok = qptr[nq];
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "%s: q_terms is NULL", entry);
    std::vector<uint32_t> terms(n_tok);
    if (n_tok) SS_HIP(ctx, ss::copy_in(ctx->stream, terms.data(), q_terms, n_tok * sizeof(uint32_t)));
    // the list table: ss_facet_counts' own (match_lists.hpp), so the calls mean the same M(q)
    ss::MatchLists ml;
    SS_TRY(ss::build_match_lists(s, entry, qptr.data(), terms.data(), nq, &ml));
    const std::vector<uint32_t>&aq = ml.aq, &lptr = ml.lptr;
    const std::vector<MatchList>& lists = ml.lists;
    // the mask ids, constraint arrays and range clauses: the scoring call's own checks, then its sets on the device
    ss::AllowedSets as;
    SS_TRY(ss::allowed_sets_into_turn(s, n_q, q_ptr, mask_id, &cons, &ranges, &as));
    // ---- nothing below refuses an argument
    SS_TRY(ensure_group_ranks(s));                  // (the first call after a registration builds them and waits once)
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[as.turn];
    const size_t n_rows = nq * (size_t)m;
    const bool dev_out = ss::on_device(groups_out) && ss::on_device(n_out) && (!n_groups_out || ss::on_device(n_groups_out)) &&
                         (!n_ungrouped_out || ss::on_device(n_ungrouped_out)) && (!n_match_out || ss::on_device(n_match_out));
    ss_group_count* d_rows = groups_out;
    int32_t* d_n = n_out;
    uint32_t *d_ng = n_groups_out, *d_ug = n_ungrouped_out, *d_match = n_match_out;
    const size_t o_n = n_rows * sizeof(ss_group_count), o_ng = o_n + nq * sizeof(int32_t), o_ug = o_ng + nq * sizeof(uint32_t),
                 o_match = o_ug + nq * sizeof(uint32_t), out_bytes = o_match + nq * sizeof(uint32_t);
    if (!dev_out) {                                 // the scorer's block: rows | n_out | n_groups | n_ungrouped | n_match
        SS_HIP(ctx, ensure(s->d_gtopk_out, out_bytes));
        unsigned char* const o = s->d_gtopk_out.p;
        d_rows = reinterpret_cast<ss_group_count*>(o);
        d_n = reinterpret_cast<int32_t*>(o + o_n);
        d_ng = reinterpret_cast<uint32_t*>(o + o_ng);
        d_ug = reinterpret_cast<uint32_t*>(o + o_ug);
        d_match = reinterpret_cast<uint32_t*>(o + o_match);
    }
    // a query without a list keeps these zeros; every other query's entries are written by its selection
    SS_HIP(ctx, hipMemsetAsync(d_n, 0, nq * sizeof(int32_t), st));
    if (d_ng) SS_HIP(ctx, hipMemsetAsync(d_ng, 0, nq * sizeof(uint32_t), st));
    if (d_ug) SS_HIP(ctx, hipMemsetAsync(d_ug, 0, nq * sizeof(uint32_t), st));
    if (d_match) SS_HIP(ctx, hipMemsetAsync(d_match, 0, nq * sizeof(uint32_t), st));
    const uint32_t n_active = (uint32_t)aq.size(), n_blocks = gp::blocks(s->n_docs), n_groups = s->n_groups;
    if (n_active && n_blocks) {
        const uint32_t K = (uint32_t)first + (uint32_t)m, cap = gp::buffer_entries(K), lds = gp::buffer_lds_bytes(K);
        const uint32_t R = gp::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("gtopk.runs", 0));
        const bool use_lds = gp::use_lds(n_groups, ctx->opt("gtopk.lds_groups", gp::DEFAULT_LDS_GROUPS));
        const uint64_t stride = gp::row_stride(n_groups);
        const uint32_t group = gp::group_queries(n_active, n_groups, gp::scratch_bytes_of(ctx->opt("gtopk.scratch_bytes", 0)));
        const size_t row_words = (size_t)group * stride;
        SS_HIP(ctx, ensure(s->d_gtopk_rows, row_words));
        // the call's tables through the turn's pinned block: active queries | list offsets | sets | lists
        std::vector<int32_t> qset(n_active);
        for (uint32_t i = 0; i < n_active; i++) qset[i] = as.set_of[aq[i]];
        const size_t o_lptr = align16(n_active * sizeof(uint32_t)), o_qset = align16(o_lptr + (n_active + 1) * sizeof(uint32_t)),
                     o_lists = align16(o_qset + n_active * sizeof(int32_t)), bytes = o_lists + lists.size() * sizeof(MatchList);
        SS_HIP(ctx, turn.h_facet.ensure(bytes));
        SS_HIP(ctx, ensure(turn.d_facet, bytes));
        unsigned char* const h = turn.h_facet.p;
        std::memcpy(h, aq.data(), n_active * sizeof(uint32_t));
        std::memcpy(h + o_lptr, lptr.data(), (n_active + 1) * sizeof(uint32_t));
        std::memcpy(h + o_qset, qset.data(), n_active * sizeof(int32_t));
        std::memcpy(h + o_lists, lists.data(), lists.size() * sizeof(MatchList));
        SS_HIP(ctx, hipMemcpyAsync(turn.d_facet.p, h, bytes, hipMemcpyHostToDevice, st));
        const unsigned char* const d = turn.d_facet.p;
        CountParams cp{};
        cp.t_doc = s->title->post_doc.p;
        cp.b_doc = s->body->post_doc.p;
        cp.lptr = reinterpret_cast<const uint32_t*>(d + o_lptr);
        cp.qset = reinterpret_cast<const int32_t*>(d + o_qset);
        cp.lists = reinterpret_cast<const MatchList*>(d + o_lists);
        cp.allowed = as.words;
        cp.allowed_stride = as.stride;
        cp.grank = s->grank.p;
        cp.n_docs = s->n_docs;
        cp.n_blocks = n_blocks;
        cp.R = R;
        cp.n_groups = n_groups;
        cp.stride = stride;
        cp.rows = s->d_gtopk_rows.p;
        SelectParams sp{};
        sp.aq = reinterpret_cast<const uint32_t*>(d);
        sp.rows = cp.rows;
        sp.gval = s->gval.p;
        sp.stride = stride;
        sp.n_groups = n_groups;
        sp.K = K;
        sp.cap = cap;
        sp.first = (uint32_t)first;
        sp.m = (uint32_t)m;
        sp.groups_out = d_rows;
        sp.n_out = d_n;
        sp.n_groups_out = d_ng;
        sp.n_ungrouped_out = d_ug;
        sp.n_match_out = d_match;
        const uint32_t hist = use_lds ? gp::hist_lds_bytes(n_groups) : 0u;
        for (const gp::Group& g : gp::groups(n_active, group)) {                // one group after another: they share the counter rows
            cp.a0 = sp.a0 = g.first;
            cp.n_group = g.count;
            SS_HIP(ctx, hipMemsetAsync(cp.rows, 0, (size_t)g.count * stride * sizeof(uint32_t), st));
            for (const gp::Launch& l : gp::launches(R, g.count)) {
                cp.run0 = l.first;
                if (use_lds) hipLaunchKernelGGL(k_group_count<true>, dim3(l.count * g.count), dim3(GT_TPB), hist, st, cp);
                else hipLaunchKernelGGL(k_group_count<false>, dim3(l.count * g.count), dim3(GT_TPB), 0, st, cp);
            }
            hipLaunchKernelGGL(k_group_select, dim3(g.count), dim3(GT_TPB), lds, st, sp);
        }
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, turn.batch_ev.record(st));          // until here the call reads the turn's sets and tables
    if (dev_out) return SS_OK;                      // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    // the block comes back whole; the caller's arrays get the counts whole and, of the rows, exactly the entries written
    std::vector<unsigned char> h_out(out_bytes);
    SS_HIP(ctx, hipMemcpyAsync(h_out.data(), s->d_gtopk_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    const int32_t* const h_n = reinterpret_cast<const int32_t*>(h_out.data() + o_n);
    // (a caller's array in device memory beside one in host memory: the same entries, by copies that wait)
    const auto give = [&](void* dst, size_t off, size_t stride, size_t elem, bool whole) -> hipError_t {
        if (!ss::on_device(dst)) {
            if (whole) std::memcpy(dst, h_out.data() + off, nq * elem);
            else hw::copy_written(dst, h_out.data() + off, nq, stride, elem, h_n);
            return hipSuccess;
        }
        if (whole) return hipMemcpy(dst, h_out.data() + off, nq * elem, hipMemcpyHostToDevice);
        for (size_t q = 0; q < nq; q++) {
            const size_t o = q * stride * elem;
            if (h_n[q] > 0)
                if (const hipError_t e = hipMemcpy(static_cast<unsigned char*>(dst) + o, h_out.data() + off + o, (size_t)h_n[q] * elem, hipMemcpyHostToDevice))
                    return e;
        }
        return hipSuccess;
    };
    SS_HIP(ctx, give(groups_out, 0, (size_t)m, sizeof(ss_group_count), false));
    SS_HIP(ctx, give(n_out, o_n, 1, sizeof(int32_t), true));
    if (n_groups_out) SS_HIP(ctx, give(n_groups_out, o_ng, 1, sizeof(uint32_t), true));
    if (n_ungrouped_out) SS_HIP(ctx, give(n_ungrouped_out, o_ug, 1, sizeof(uint32_t), true));
    if (n_match_out) SS_HIP(ctx, give(n_match_out, o_match, 1, sizeof(uint32_t), true));
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_scorer_group_values(ss_scorer* s, uint32_t* n_groups_out, uint32_t* values_out) {
    return hw::guarded(s, "ss_scorer_group_values", [&] { return group_values_impl(s, n_groups_out, values_out); });
}

int32_t ss_top_groups(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                      const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                      const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t first, int32_t m, ss_group_count* groups_out, int32_t* n_out,
                      uint32_t* n_groups_out, uint32_t* n_ungrouped_out, uint32_t* n_match_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return hw::guarded(s, "ss_top_groups", [&] {
        return top_groups_impl(s, n_q, q_ptr, q_terms, mask_id, cons, ranges, first, m, groups_out, n_out, n_groups_out, n_ungrouped_out, n_match_out);
    });
}

}  // extern "C"
