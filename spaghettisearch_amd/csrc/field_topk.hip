// field_topk.hip — ss_field_topk: the exact top-k of ALL docs a query matches, ordered by a doc field ("newest first" over every match,
// not over a relevance window).  DESIGN.md K4t; no reference counterpart.
//
// M(q) is ss_facet_counts' match set (facet.hip): the docs with a posting of any usable query term AND the allowed set of the scoring
// path (ss::allowed_sets_into_turn).  k_field_select gives a workgroup a RUN of consecutive 32768-doc blocks of one query.  Per block it
// forms the match words as k_facet_counts does (the lists' runs in the block, the OR image in LDS, AND with the allowed row and
// d < n_docs); the bounds of a block's runs are searched from the previous block's ends, not cold.  For every set bit it gathers
// value[field][d], forms the key (field_topk_plan.hpp) and, if the key beats the threshold, appends it to a candidate buffer in LDS.
// A thread that finds the buffer full keeps its candidate; the workgroup then compacts the buffer to its K = first + k smallest keys by
// a bitonic sort, lowers the threshold to the K-th and goes on: exact whatever the arrival order, at most one compaction per
// (buffer - K) appended keys.  The run's K smallest keys and its match count go to a partial list.  k_field_merge, one workgroup per
// query, pushes the R partial lists through the same buffer and writes the page, n_out and the summed match count.  No atomics on any
// output; the total order of the keys (value, then doc id) leaves nothing for an arrival order to decide.
//
// Steps 1 to 3 of the kernel are a private copy of k_facet_counts': step 1 differs (warm bounds along the run), the ANDed words go back
// to LDS for the resumable walk of step 4, and k_facet_counts stays the same instructions.  The host's list table is shared
// (match_lists.hpp).
#include "field_topk_plan.hpp"
#include "hit_window.hpp"
#include "match_lists.hpp"

namespace tp = ss::ftopk;
namespace hw = ss::hitwin;

static_assert(tp::MAX_K == SS_MAX_TOPK && tp::MAX_LISTS == 2 * SS_MAX_QUERY_TERMS, "field_topk_plan.hpp restates the ABI's limits");

namespace {

constexpr int FT_TPB = (int)tp::THREADS;
constexpr int FT_WPT = 4;                           // words of a thread (one 16-byte LDS / global load)
constexpr int FT_WAVES = FT_TPB / 64;
static_assert(FT_TPB * FT_WPT == (int)tp::BLOCK_WORDS && FT_TPB == 2 * (int)tp::MAX_LISTS, "block geometry");

using ss::MatchList;                            // postings [b, b + len) of the title (field 1) or body (0) table (match_lists.hpp)

struct SelectParams {
    const uint32_t* t_doc;            // the tables' post_doc (strictly ascending inside a term)
    const uint32_t* b_doc;
    const uint32_t* lptr;             // [n_active + 1] the active queries' lists in `lists`
    const int32_t* qset;              // [n_active] row of `allowed`, -1: every doc
    const MatchList* lists;
    const uint32_t* allowed;          // [..][allowed_stride]
    uint64_t allowed_stride;
    const int64_t* col;               // value[field]: [n_docs]
    uint64_t n_docs;
    uint32_t n_blocks, R, K, cap, desc;
    uint32_t a0, n_group, run0;       // this launch: active queries [a0, a0 + n_group), runs from run0
    uint64_t* part_key;               // [n_group][R][K]
    uint32_t* part_doc;               // [n_group][R][K]
    uint32_t* run_cnt;                // [n_group][R][2]: the run's matches, the length of its list
};

struct MergeParams {
    const uint32_t* aq;               // [n_active] the queries that have a list
    const uint64_t* part_key;
    const uint32_t* part_doc;
    const uint32_t* run_cnt;
    uint32_t R, K, cap, desc, first, k, a0;
    uint32_t* docs_out;               // [n_q][k]
    int32_t* n_out;                   // [n_q]
    int64_t* values_out;              // [n_q][k], nullable
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

// The running best-K of a workgroup: `cap` entries (key, doc) in LDS, *cnt of them in use (it may run past cap while threads are
// refused), and the threshold: the K-th smallest key once K are known, the pad key before.
struct Best {
    uint64_t* key;
    uint32_t* doc;
    uint32_t* cnt;
    uint64_t* thr_key;
    uint32_t* thr_doc;
    uint32_t cap, K;
};
// false: the buffer is full, the caller keeps the candidate until the next compaction
__device__ __forceinline__ bool best_push(const Best& b, uint64_t key, uint32_t doc) {
    const uint32_t pos = atomicAdd(b.cnt, 1u);
    if (pos >= b.cap) return false;
    b.key[pos] = key;
    b.doc[pos] = doc;
    return true;
}
// By all threads, behind a barrier that ends the pushes: the entries sorted, the K smallest kept, the threshold lowered.  Ends behind a
// barrier.
__device__ void best_compact(const Best& b) {
    const uint32_t n = min(*b.cnt, b.cap);
    const uint32_t np = tp::pow2_at_least(n);       // <= cap, a power of two
    __syncthreads();                                // (everyone has read the count)
    for (uint32_t i = n + threadIdx.x; i < np; i += FT_TPB) {
        b.key[i] = tp::PAD_KEY;
        b.doc[i] = tp::PAD_DOC;
    }
    __syncthreads();
    hw::bitonic_sort<FT_TPB>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t ki = b.key[i], ko = b.key[o];
        const uint32_t di = b.doc[i], dd = b.doc[o];
        if (tp::key_less(ko, dd, ki, di) == up) {
            b.key[i] = ko; b.key[o] = ki;
            b.doc[i] = dd; b.doc[o] = di;
        }
    });
    if (threadIdx.x == 0) {
        *b.cnt = min(n, b.K);
        if (n >= b.K) {
            *b.thr_key = b.key[b.K - 1];
            *b.thr_doc = b.doc[b.K - 1];
        }
    }
    __syncthreads();
}

// Grid: blockIdx.x = (run - run0) * n_group + query — the queries of one run are neighbours, so the run's allowed words and field
// values come from L2 for all but the first of them.  Dynamic LDS: cap keys, then cap doc ids.
__global__ __launch_bounds__(FT_TPB) void k_field_select(SelectParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ft_dyn[];
    __shared__ uint64_t cur[tp::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[tp::BLOCK_WORDS];   // the block's docs with a posting of the query, then its matches
    __shared__ uint64_t s_thr_key;
    __shared__ uint32_t s_thr_doc, s_cnt;
    __shared__ uint32_t wsum[FT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.lptr[a], nl = p.lptr[a + 1] - l0;                  // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint32_t b0 = tp::run_begin(r, p.R, p.n_blocks), b1 = tp::run_begin(r + 1, p.R, p.n_blocks);
    const Best best{reinterpret_cast<uint64_t*>(ft_dyn), reinterpret_cast<uint32_t*>(ft_dyn + (size_t)p.cap * sizeof(uint64_t)), &s_cnt,
                    &s_thr_key, &s_thr_doc, p.cap, p.K};
    const bool desc = p.desc != 0;
    if (tid == 0) {
        s_cnt = 0u;
        s_thr_key = tp::PAD_KEY;
        s_thr_doc = tp::PAD_DOC;
    }
    uint32_t matches = 0;                                                    // of this thread's words, over the run
    for (uint32_t blk = b0; blk < b1; blk++) {
        const uint64_t base = (uint64_t)blk * tp::BLOCK_DOCS;                // the block's first doc
        // ---- 1. the runs: cold at the head of the run (thread (list, end) searches one bound), from the last block's end after it
        if (blk == b0) {
            if ((uint32_t)tid < 2 * nl) {
                const MatchList fl = p.lists[l0 + (tid >> 1)];
                const int hi = tid & 1;
                cur[tid >> 1][hi] = lower_doc(fl.field ? p.t_doc : p.b_doc, fl.b, fl.b + fl.len, base + (hi ? (uint64_t)tp::BLOCK_DOCS : 0));
            }
        } else if ((uint32_t)tid < nl) {
            const MatchList fl = p.lists[l0 + tid];
            const uint64_t lo = cur[tid][1], len = lo - cur[tid][0];
            cur[tid][0] = lo;
            cur[tid][1] = lower_doc_from(fl.field ? p.t_doc : p.b_doc, lo, fl.b + fl.len, base + tp::BLOCK_DOCS, 2 * len + 64);
        }
        __syncthreads();
        // a block no list reaches is left here: it has read the search paths and nothing else
        if (!__syncthreads_or((uint32_t)tid < nl && cur[tid][0] < cur[tid][1])) continue;
        // ---- 2. the image
        *reinterpret_cast<uint4*>(&img[tid * FT_WPT]) = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t* const doc = p.lists[l0 + l].field ? p.t_doc : p.b_doc;
            const uint64_t e = cur[l][1];
            for (uint64_t j = cur[l][0] + tid; j < e; j += FT_TPB) {
                const uint32_t d = (uint32_t)((uint64_t)doc[j] - base);
                if (d < tp::BLOCK_DOCS) atomicOr(&img[d >> 5], 1u << (d & 31u));   // (always, for an ascending list: the image is never left)
            }
        }
        __syncthreads();
        // ---- 3. AND the allowed set and d < n_docs; the words go back to the image (each thread reads its own words only)
        const uint64_t w0 = (uint64_t)blk * tp::BLOCK_WORDS + (uint64_t)tid * FT_WPT;   // this thread's first word
        const uint4 u = *reinterpret_cast<const uint4*>(&img[tid * FT_WPT]);
        uint32_t m[FT_WPT] = {u.x, u.y, u.z, u.w};
        const int32_t set = p.qset[a];
        if (set >= 0) {
            const uint32_t* const row = p.allowed + (uint64_t)set * p.allowed_stride;
            if ((p.allowed_stride & 3u) == 0 && w0 + FT_WPT <= p.allowed_stride) {      // (rows then start 16-byte aligned)
                const uint4 al4 = *reinterpret_cast<const uint4*>(row + w0);
                m[0] &= al4.x; m[1] &= al4.y; m[2] &= al4.z; m[3] &= al4.w;
            } else {
#pragma unroll
                for (int i = 0; i < FT_WPT; i++) m[i] &= w0 + i < p.allowed_stride ? row[w0 + i] : 0u;
            }
        }
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < FT_WPT; i++) {
            m[i] &= tp::word_valid(w0 + i, p.n_docs);
            cnt += __popc(m[i]);
        }
        *reinterpret_cast<uint4*>(&img[tid * FT_WPT]) = make_uint4(m[0], m[1], m[2], m[3]);
        matches += cnt;
        if (!__syncthreads_or(cnt != 0)) continue;   // the allowed set left nothing of the block
        // ---- 4. the candidates: the key of every set bit against the threshold, into the buffer; a refused thread stands still until
        // the buffer is compacted
        uint64_t thr_key = s_thr_key;
        uint32_t thr_doc = s_thr_doc;
        uint32_t wi = 0, bits = m[0];
        for (;;) {
            bool pending = false;
            for (;;) {
                while (!bits && wi + 1 < FT_WPT) bits = img[tid * FT_WPT + ++wi];
                if (!bits) break;
                const uint32_t d = (uint32_t)((w0 + wi) * 32) + (uint32_t)(__ffs(bits) - 1);     // < n_docs < 2^32
                const uint64_t key = tp::value_key(p.col[d], desc);
                if (tp::key_less(key, d, thr_key, thr_doc) && !best_push(best, key, d)) {
                    pending = true;
                    break;
                }
                bits &= bits - 1;
            }
            if (!__syncthreads_or(pending)) break;
            best_compact(best);
            thr_key = s_thr_key;
            thr_doc = s_thr_doc;
        }
    }
    // ---- the run's list: its K smallest keys in order, and its counts
    __syncthreads();
    best_compact(best);
    const uint32_t n = s_cnt;
    const uint64_t slot = (uint64_t)al * p.R + r;
    for (uint32_t i = tid; i < n; i += FT_TPB) {
        p.part_key[slot * p.K + i] = best.key[i];
        p.part_doc[slot * p.K + i] = best.doc[i];
    }
    matches = wave_sum(matches);
    if ((tid & 63) == 0) wsum[tid >> 6] = matches;
    __syncthreads();
    if (tid == 0) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < FT_WAVES; w++) v += wsum[w];
        p.run_cnt[slot * 2] = v;
        p.run_cnt[slot * 2 + 1] = n;
    }
}

// Grid: one workgroup per active query of the group.  Dynamic LDS as k_field_select's.
__global__ __launch_bounds__(FT_TPB) void k_field_merge(MergeParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ft_dyn[];
    __shared__ uint64_t s_thr_key;
    __shared__ uint32_t s_thr_doc, s_cnt;
    __shared__ uint32_t wsum[FT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x, q = p.aq[p.a0 + al];
    const Best best{reinterpret_cast<uint64_t*>(ft_dyn), reinterpret_cast<uint32_t*>(ft_dyn + (size_t)p.cap * sizeof(uint64_t)), &s_cnt,
                    &s_thr_key, &s_thr_doc, p.cap, p.K};
    if (tid == 0) {
        s_cnt = 0u;
        s_thr_key = tp::PAD_KEY;
        s_thr_doc = tp::PAD_DOC;
    }
    const uint32_t* const rc = p.run_cnt + (uint64_t)al * p.R * 2;
    uint32_t total = 0;
    for (uint32_t r = tid; r < p.R; r += FT_TPB) total += rc[r * 2];
    total = wave_sum(total);
    if ((tid & 63) == 0) wsum[tid >> 6] = total;
    __syncthreads();
    uint64_t thr_key = tp::PAD_KEY;
    uint32_t thr_doc = tp::PAD_DOC;
    const uint64_t n_slots = (uint64_t)p.R * p.K, e0 = (uint64_t)al * n_slots;
    uint64_t x = (uint64_t)tid;
    for (;;) {
        bool pending = false;
        for (; x < n_slots; x += FT_TPB) {
            const uint32_t r = (uint32_t)(x / p.K), j = (uint32_t)(x - (uint64_t)r * p.K);
            if (j >= rc[r * 2 + 1]) continue;
            const uint64_t key = p.part_key[e0 + x];
            const uint32_t d = p.part_doc[e0 + x];
            if (tp::key_less(key, d, thr_key, thr_doc) && !best_push(best, key, d)) {
                pending = true;
                break;
            }
        }
        if (!__syncthreads_or(pending)) break;
        best_compact(best);
        thr_key = s_thr_key;
        thr_doc = s_thr_doc;
    }
    best_compact(best);
    const uint32_t n_page = hw::page_len(s_cnt, p.first, p.k);
    const bool desc = p.desc != 0;
    for (uint32_t i = tid; i < n_page; i += FT_TPB) {
        p.docs_out[(uint64_t)q * p.k + i] = best.doc[p.first + i];
        if (p.values_out) p.values_out[(uint64_t)q * p.k + i] = tp::key_value(best.key[p.first + i], desc);
    }
    if (tid == 0) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < FT_WAVES; w++) v += wsum[w];
        p.n_out[q] = (int32_t)n_page;
        if (p.n_match_out) p.n_match_out[q] = v;
    }
}

int32_t plan_code(int rc) { return rc == tp::INVALID ? SS_ERR_INVALID : rc == tp::UNSUPPORTED ? SS_ERR_UNSUPPORTED : SS_ERR_STATE; }

int32_t field_topk_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id, const QueryConstraints& cons,
                        const QueryRanges& ranges, int32_t field, int32_t descending, int32_t first, int32_t k, uint32_t* docs_out, int32_t* n_out,
                        int64_t* values_out, uint32_t* n_match_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_field_topk";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = tp::check_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, docs_out != nullptr, n_out != nullptr, field, first, k, s->n_fields))
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
    // the list table: ss_facet_counts' own (match_lists.hpp), so both calls mean the same M(q)
    ss::MatchLists ml;
    SS_TRY(ss::build_match_lists(s, entry, qptr.data(), terms.data(), nq, &ml));
    const std::vector<uint32_t>&aq = ml.aq, &lptr = ml.lptr;
    const std::vector<MatchList>& lists = ml.lists;
    // the mask ids, constraint arrays and range clauses: the scoring call's own checks, then its sets on the device
    ss::AllowedSets as;
    SS_TRY(ss::allowed_sets_into_turn(s, n_q, q_ptr, mask_id, &cons, &ranges, &as));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[as.turn];
    const size_t n_rows = nq * (size_t)k;
    const bool dev_out = ss::on_device(docs_out) && ss::on_device(n_out) && (!values_out || ss::on_device(values_out)) &&
                         (!n_match_out || ss::on_device(n_match_out));
    uint32_t *d_docs = docs_out, *d_match = n_match_out;
    int32_t* d_n = n_out;
    int64_t* d_val = values_out;
    const size_t o_docs = n_rows * sizeof(int64_t), o_n = o_docs + n_rows * sizeof(uint32_t), o_match = o_n + nq * sizeof(int32_t),
                 out_bytes = o_match + nq * sizeof(uint32_t);
    if (!dev_out) {                                 // the scorer's block: values | docs | n_out | n_match
        SS_HIP(ctx, ensure(s->d_ftopk_out, out_bytes));
        unsigned char* const o = s->d_ftopk_out.p;
        d_val = values_out ? reinterpret_cast<int64_t*>(o) : nullptr;
        d_docs = reinterpret_cast<uint32_t*>(o + o_docs);
        d_n = reinterpret_cast<int32_t*>(o + o_n);
        d_match = reinterpret_cast<uint32_t*>(o + o_match);
    }
    // a query without a list keeps these zeros; every other query's entries are written by its merge
    SS_HIP(ctx, hipMemsetAsync(d_n, 0, nq * sizeof(int32_t), st));
    if (d_match) SS_HIP(ctx, hipMemsetAsync(d_match, 0, nq * sizeof(uint32_t), st));
    const uint32_t n_active = (uint32_t)aq.size(), n_blocks = tp::blocks(s->n_docs);
    if (n_active && n_blocks) {
        const uint32_t K = (uint32_t)first + (uint32_t)k, cap = tp::buffer_entries(K), lds = tp::buffer_lds_bytes(K);
        const uint32_t R = tp::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("ftopk.runs", 0));
        const uint32_t group = tp::group_queries(n_active, R, K, tp::scratch_bytes_of(ctx->opt("ftopk.scratch_bytes", 0)));
        // the partial lists of one group: keys | doc ids | run counts
        const size_t slots = (size_t)group * R, o_pdoc = slots * K * sizeof(uint64_t), o_rc = o_pdoc + slots * K * sizeof(uint32_t),
                     part_bytes = o_rc + slots * 2 * sizeof(uint32_t);
        SS_HIP(ctx, ensure(s->d_ftopk_part, part_bytes));
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
        unsigned char* const part = s->d_ftopk_part.p;
        SelectParams sp{};
        sp.t_doc = s->title->post_doc.p;
        sp.b_doc = s->body->post_doc.p;
        sp.lptr = reinterpret_cast<const uint32_t*>(d + o_lptr);
        sp.qset = reinterpret_cast<const int32_t*>(d + o_qset);
        sp.lists = reinterpret_cast<const MatchList*>(d + o_lists);
        sp.allowed = as.words;
        sp.allowed_stride = as.stride;
        sp.col = s->fields.p + (size_t)field * s->n_docs;
        sp.n_docs = s->n_docs;
        sp.n_blocks = n_blocks;
        sp.R = R;
        sp.K = K;
        sp.cap = cap;
        sp.desc = descending != 0;
        sp.part_key = reinterpret_cast<uint64_t*>(part);
        sp.part_doc = reinterpret_cast<uint32_t*>(part + o_pdoc);
        sp.run_cnt = reinterpret_cast<uint32_t*>(part + o_rc);
        MergeParams mp{};
        mp.aq = reinterpret_cast<const uint32_t*>(d);
        mp.part_key = sp.part_key;
        mp.part_doc = sp.part_doc;
        mp.run_cnt = sp.run_cnt;
        mp.R = R;
        mp.K = K;
        mp.cap = cap;
        mp.desc = sp.desc;
        mp.first = (uint32_t)first;
        mp.k = (uint32_t)k;
        mp.docs_out = d_docs;
        mp.n_out = d_n;
        mp.values_out = d_val;
        mp.n_match_out = d_match;
        for (const tp::Group& g : tp::groups(n_active, group)) {                // one group after another: they share the partial lists
            sp.a0 = mp.a0 = g.first;
            sp.n_group = g.count;
            for (const tp::Launch& l : tp::launches(R, g.count)) {
                sp.run0 = l.first;
                hipLaunchKernelGGL(k_field_select, dim3(l.count * g.count), dim3(FT_TPB), lds, st, sp);
            }
            hipLaunchKernelGGL(k_field_merge, dim3(g.count), dim3(FT_TPB), lds, st, mp);
        }
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, turn.batch_ev.record(st));          // until here the call reads the turn's sets and tables
    if (dev_out) return SS_OK;                      // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    // the block comes back whole; the caller's arrays get the counts whole and, of docs and values, exactly the entries written
    const size_t from = values_out ? 0 : o_docs;
    std::vector<unsigned char> h_out(out_bytes);
    SS_HIP(ctx, hipMemcpyAsync(h_out.data() + from, s->d_ftopk_out.p + from, out_bytes - from, hipMemcpyDeviceToHost, st));
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
    SS_HIP(ctx, give(docs_out, o_docs, (size_t)k, sizeof(uint32_t), false));
    if (values_out) SS_HIP(ctx, give(values_out, 0, (size_t)k, sizeof(int64_t), false));
    SS_HIP(ctx, give(n_out, o_n, 1, sizeof(int32_t), true));
    if (n_match_out) SS_HIP(ctx, give(n_match_out, o_match, 1, sizeof(uint32_t), true));
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_field_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                      const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                      const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t field, int32_t descending, int32_t first, int32_t k,
                      uint32_t* docs_out, int32_t* n_out, int64_t* values_out, uint32_t* n_match_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return hw::guarded(s, "ss_field_topk", [&] {
        return field_topk_impl(s, n_q, q_ptr, q_terms, mask_id, cons, ranges, field, descending, first, k, docs_out, n_out, values_out, n_match_out);
    });
}

}  // extern "C"
