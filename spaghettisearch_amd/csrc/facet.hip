// facet.hip — ss_facet_counts: how many docs a query matches, in all, per registered allow-list and per value bucket of a doc field
// (no reference counterpart).
//
// M(q) = (the docs with a posting of any usable query term, title or body) AND (the allowed set ss_score_topk_filtered builds for the
// query's mask id, required / excluded terms and range clauses): the docs that call ranks.  k_facet_counts never writes M(q) out.  A
// workgroup owns one block of 32768 docs of one query: it finds the run of every list of the query in the block by two binary
// searches (posting lists ascend strictly by doc), ORs the runs into an LDS image, ANDs the image with the allowed set's words and
// with d < n_docs, and reduces it: one popcount for the total, one popcount of image & mask_m per registered mask, and for the
// buckets one gather of value[field][d] per SET bit and field, placed by one binary search among the elementary intervals of the
// buckets' bounds (facet_plan.hpp) into an LDS histogram.  The block's partial counts join the outputs by integer atomicAdd behind
// a zeroing memset: exact and independent of the order.  The allowed sets come from the scoring path (ss::allowed_sets_into_turn).
#include "facet_plan.hpp"
#include "hit_window.hpp"
#include "match_lists.hpp"

namespace fp = ss::facetp;
namespace hw = ss::hitwin;

static_assert(fp::MAX_BUCKETS == SS_MAX_FACET_BUCKETS && fp::MAX_FIELDS == SS_MAX_DOC_FIELDS && fp::MAX_LISTS == 2 * SS_MAX_QUERY_TERMS,
              "facet_plan.hpp restates the ABI's limits");
static_assert(sizeof(fp::Range) == sizeof(ss_doc_range) && offsetof(fp::Range, field) == offsetof(ss_doc_range, field) &&
                  offsetof(fp::Range, lo) == offsetof(ss_doc_range, lo) && offsetof(fp::Range, hi) == offsetof(ss_doc_range, hi),
              "facet_plan.hpp restates ss_doc_range");

namespace {

constexpr int FC_TPB = 256;                         // threads: one bound of one list each in the search phase (2 x MAX_LISTS)
constexpr int FC_WPT = 4;                           // words of a thread (one 16-byte LDS / global load)
constexpr int FC_WAVES = FC_TPB / 64;
constexpr int FC_CHUNK = 64;                        // counters (total, masks) that share one pass through the waves' partial sums
static_assert(FC_TPB * FC_WPT == (int)fp::BLOCK_WORDS && FC_TPB == 2 * (int)fp::MAX_LISTS, "block geometry");

using FacetList = ss::MatchList;               // postings [b, b + len) of the title (field 1) or body (0) table (match_lists.hpp)

struct FacetParams {
    const uint32_t* t_doc;            // the tables' post_doc (strictly ascending inside a term)
    const uint32_t* b_doc;
    const uint32_t* aq;               // [n_active] the queries that have a list
    const uint32_t* lptr;             // [n_active + 1] their lists in `lists`
    const int32_t* qset;              // [n_active] row of `allowed`, -1: every doc
    const FacetList* lists;
    const uint32_t* allowed;          // [..][allowed_stride]
    uint64_t allowed_stride;
    const uint32_t* masks;            // the registered allow-lists [n_masks][mask_words]; n_masks 0: no mask counts
    uint64_t mask_words;
    uint32_t n_masks;
    uint32_t n_buckets;
    const int64_t* values;            // the field table [n_fields][n_docs]
    const fp::BucketTable* btab;
    uint64_t n_docs;
    uint32_t n_active, blk0;          // this launch: doc blocks from blk0
    uint32_t* n_match;                // [n_q]
    uint32_t* mask_counts;            // [n_q][n_masks]
    uint32_t* bucket_counts;          // [n_q][n_buckets]
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

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// Grid: blockIdx.x = block * n_active + query — the queries of one doc block are neighbours, so the block's mask words and field
// values come from L2 for all but the first of them.
__global__ __launch_bounds__(FC_TPB) void k_facet_counts(FacetParams p) {
    __shared__ uint64_t cur[fp::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[fp::BLOCK_WORDS];   // the block's docs with a posting of the query
    __shared__ uint32_t wsum[FC_CHUNK][FC_WAVES];                            // the waves' partial sums of up to FC_CHUNK counters
    __shared__ int64_t cuts[fp::MAX_CUTS];                                   // the buckets' elementary intervals and their histogram
    __shared__ uint32_t hist[fp::MAX_CUTS];
    const int tid = threadIdx.x;
    const uint32_t a = blockIdx.x % p.n_active, blk = p.blk0 + blockIdx.x / p.n_active;
    const uint32_t l0 = p.lptr[a], nl = p.lptr[a + 1] - l0;                  // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint64_t base = (uint64_t)blk * fp::BLOCK_DOCS;                    // the block's first doc
    // ---- 1. the runs: thread (list, end) searches one bound
    if ((uint32_t)tid < 2 * nl) {
        const FacetList fl = p.lists[l0 + (tid >> 1)];
        const int hi = tid & 1;
        cur[tid >> 1][hi] = lower_doc(fl.field ? p.t_doc : p.b_doc, fl.b, fl.b + fl.len, base + (hi ? (uint64_t)fp::BLOCK_DOCS : 0));
    }
    __syncthreads();
    // a block no list reaches leaves here: it has read 2 x nl search paths and nothing else
    if (!__syncthreads_or((uint32_t)tid < nl && cur[tid][0] < cur[tid][1])) return;
    // ---- 2. the image
    *reinterpret_cast<uint4*>(&img[tid * FC_WPT]) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t* const doc = p.lists[l0 + l].field ? p.t_doc : p.b_doc;
        const uint64_t e = cur[l][1];
        for (uint64_t j = cur[l][0] + tid; j < e; j += FC_TPB) {
            const uint32_t d = (uint32_t)((uint64_t)doc[j] - base);
            if (d < fp::BLOCK_DOCS) atomicOr(&img[d >> 5], 1u << (d & 31u));   // (always, for an ascending list: the image is never left)
        }
    }
    __syncthreads();
    // ---- 3. AND the allowed set and d < n_docs
    const uint64_t w0 = (uint64_t)blk * fp::BLOCK_WORDS + (uint64_t)tid * FC_WPT;   // this thread's first word
    const uint4 u = *reinterpret_cast<const uint4*>(&img[tid * FC_WPT]);
    uint32_t m[FC_WPT] = {u.x, u.y, u.z, u.w};
    const int32_t set = p.qset[a];
    if (set >= 0) {
        const uint32_t* const row = p.allowed + (uint64_t)set * p.allowed_stride;
        if ((p.allowed_stride & 3u) == 0 && w0 + FC_WPT <= p.allowed_stride) {      // (rows then start 16-byte aligned)
            const uint4 al = *reinterpret_cast<const uint4*>(row + w0);
            m[0] &= al.x; m[1] &= al.y; m[2] &= al.z; m[3] &= al.w;
        } else {
#pragma unroll
            for (int i = 0; i < FC_WPT; i++) m[i] &= w0 + i < p.allowed_stride ? row[w0 + i] : 0u;
        }
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < FC_WPT; i++) {
        m[i] &= fp::word_valid(w0 + i, p.n_docs);
        cnt += __popc(m[i]);
    }
    if (!__syncthreads_or(cnt != 0)) return;        // the allowed set left nothing of the block
    // ---- 4a. the total and the masks: counter 0 = |M|, counter 1 + i = |M & mask_i|, FC_CHUNK counters per pass
    const uint32_t q = p.aq[a];
    const uint32_t n_cnt = 1 + p.n_masks;
    const int wave = tid >> 6, lane = tid & 63;
    for (uint32_t c0 = 0; c0 < n_cnt; c0 += FC_CHUNK) {
        const uint32_t n_c = min((uint32_t)FC_CHUNK, n_cnt - c0);
        for (uint32_t c = 0; c < n_c; c++) {
            uint32_t v = cnt;
            if (c0 + c) {
                const uint32_t* const mrow = p.masks + (uint64_t)(c0 + c - 1) * p.mask_words;
                v = 0;
#pragma unroll
                for (int i = 0; i < FC_WPT; i++)
                    if (m[i] && w0 + i < p.mask_words) v += __popc(m[i] & mrow[w0 + i]);     // (only words with a match are read)
            }
            v = wave_sum(v);
            if (lane == 0) wsum[c][wave] = v;
        }
        __syncthreads();
        if ((uint32_t)tid < n_c) {
            uint32_t v = 0;
#pragma unroll
            for (int w = 0; w < FC_WAVES; w++) v += wsum[tid][w];
            const uint32_t c = c0 + tid;
            if (v) atomicAdd(c ? &p.mask_counts[(uint64_t)q * p.n_masks + (c - 1)] : &p.n_match[q], v);
        }
        __syncthreads();
    }
    // ---- 4b. the buckets: the value of every SET bit, once per field that has a bucket
    if (p.n_buckets == 0) return;
    const fp::BucketTable& bt = *p.btab;
    const uint32_t n_cuts = bt.n_cuts;
    if ((uint32_t)tid < n_cuts) {
        cuts[tid] = bt.cuts[tid];
        hist[tid] = 0u;
    }
    __syncthreads();
    const uint32_t field_mask = bt.field_mask;
    for (uint32_t f = 0; f < fp::MAX_FIELDS; f++) {
        if (!(field_mask >> f & 1u)) continue;
        const uint32_t cb = bt.field_begin[f], ce = bt.field_begin[f + 1];
        const int64_t* const col = p.values + (uint64_t)f * p.n_docs;
#pragma unroll
        for (int i = 0; i < FC_WPT; i++) {
            uint32_t bits = m[i];
            while (bits) {
                const uint32_t bit = __ffs(bits) - 1;
                bits &= bits - 1;
                const uint32_t iv = fp::interval_of(cuts, cb, ce, col[(w0 + i) * 32 + bit]);
                if (iv != fp::NO_INTERVAL) atomicAdd(&hist[iv], 1u);                         // LDS
            }
        }
    }
    __syncthreads();
    if ((uint32_t)tid < p.n_buckets) {
        uint32_t v = 0;
        for (uint32_t i = bt.lo_idx[tid]; i < bt.hi_end[tid]; i++) v += hist[i];
        if (v) atomicAdd(&p.bucket_counts[(uint64_t)q * p.n_buckets + tid], v);
    }
}

int32_t plan_code(int rc) { return rc == fp::INVALID ? SS_ERR_INVALID : rc == fp::UNSUPPORTED ? SS_ERR_UNSUPPORTED : SS_ERR_STATE; }

int32_t facet_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id, const QueryConstraints& cons,
                   const QueryRanges& ranges, int32_t n_buckets, const ss_doc_range* buckets, uint32_t* n_match_out, uint32_t* mask_counts_out,
                   uint32_t* bucket_counts_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_facet_counts";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = fp::check_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, n_match_out != nullptr, n_buckets, buckets != nullptr,
                                      bucket_counts_out != nullptr, s->n_fields))
        return ctx->fail(plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    std::vector<ss_doc_range> bk((size_t)n_buckets);
    if (n_buckets) SS_HIP(ctx, ss::copy_in(ctx->stream, bk.data(), buckets, bk.size() * sizeof(ss_doc_range)));
    if (const int rc = fp::check_buckets(msg, sizeof(msg), entry, reinterpret_cast<const fp::Range*>(bk.data()), n_buckets, s->n_fields))
        return ctx->fail(plan_code(rc), "%s", msg);
    std::vector<uint32_t> qptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, entry, "q", q_ptr, nq, qptr.data()));
    const uint32_t n_tok = qptr[nq];
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "%s: q_terms is NULL", entry);
    std::vector<uint32_t> terms(n_tok);
    if (n_tok) SS_HIP(ctx, ss::copy_in(ctx->stream, terms.data(), q_terms, n_tok * sizeof(uint32_t)));
    // the list table: per query its distinct usable terms' non-empty lists (match_lists.hpp, shared with ss_field_topk)
    ss::MatchLists ml;
    SS_TRY(ss::build_match_lists(s, entry, qptr.data(), terms.data(), nq, &ml));
    const std::vector<uint32_t>&aq = ml.aq, &lptr = ml.lptr;
    const std::vector<FacetList>& lists = ml.lists;
    // the mask ids, constraint arrays and range clauses: the scoring call's own checks, then its sets on the device
    ss::AllowedSets as;
    SS_TRY(ss::allowed_sets_into_turn(s, n_q, q_ptr, mask_id, &cons, &ranges, &as));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[as.turn];
    const uint32_t n_masks = mask_counts_out ? (uint32_t)s->n_masks : 0u;
    const size_t n_mc = nq * n_masks, n_bc = nq * (size_t)n_buckets;
    const bool dev_out = ss::on_device(n_match_out) && (!n_mc || ss::on_device(mask_counts_out)) && (!n_bc || ss::on_device(bucket_counts_out));
    uint32_t *d_match = n_match_out, *d_mc = mask_counts_out, *d_bc = bucket_counts_out;
    if (!dev_out) {
        SS_HIP(ctx, ensure(s->d_facet_out, nq + n_mc + n_bc));
        d_match = s->d_facet_out.p;
        d_mc = d_match + nq;
        d_bc = d_mc + n_mc;
        SS_HIP(ctx, hipMemsetAsync(d_match, 0, (nq + n_mc + n_bc) * sizeof(uint32_t), st));
    } else {
        SS_HIP(ctx, hipMemsetAsync(d_match, 0, nq * sizeof(uint32_t), st));
        if (n_mc) SS_HIP(ctx, hipMemsetAsync(d_mc, 0, n_mc * sizeof(uint32_t), st));
        if (n_bc) SS_HIP(ctx, hipMemsetAsync(d_bc, 0, n_bc * sizeof(uint32_t), st));
    }
    const uint32_t n_active = (uint32_t)aq.size();
    const std::vector<fp::Launch> launches = fp::launches(fp::blocks(s->n_docs), n_active);
    if (!launches.empty()) {
        // the call's tables through the turn's pinned block: active queries | list offsets | sets | lists | bucket table
        std::vector<int32_t> qset(n_active);
        for (uint32_t i = 0; i < n_active; i++) qset[i] = as.set_of[aq[i]];
        const size_t o_lptr = align16(n_active * sizeof(uint32_t)), o_qset = align16(o_lptr + (n_active + 1) * sizeof(uint32_t)),
                     o_lists = align16(o_qset + n_active * sizeof(int32_t)), o_bt = align16(o_lists + lists.size() * sizeof(FacetList)),
                     bytes = o_bt + sizeof(fp::BucketTable);
        SS_HIP(ctx, turn.h_facet.ensure(bytes));
        SS_HIP(ctx, ensure(turn.d_facet, bytes));
        unsigned char* const h = turn.h_facet.p;
        std::memcpy(h, aq.data(), n_active * sizeof(uint32_t));
        std::memcpy(h + o_lptr, lptr.data(), (n_active + 1) * sizeof(uint32_t));
        std::memcpy(h + o_qset, qset.data(), n_active * sizeof(int32_t));
        std::memcpy(h + o_lists, lists.data(), lists.size() * sizeof(FacetList));
        fp::build_bucket_table(reinterpret_cast<const fp::Range*>(bk.data()), n_buckets, *reinterpret_cast<fp::BucketTable*>(h + o_bt));
        SS_HIP(ctx, hipMemcpyAsync(turn.d_facet.p, h, bytes, hipMemcpyHostToDevice, st));
        const unsigned char* const d = turn.d_facet.p;
        FacetParams p{};
        p.t_doc = s->title->post_doc.p;
        p.b_doc = s->body->post_doc.p;
        p.aq = reinterpret_cast<const uint32_t*>(d);
        p.lptr = reinterpret_cast<const uint32_t*>(d + o_lptr);
        p.qset = reinterpret_cast<const int32_t*>(d + o_qset);
        p.lists = reinterpret_cast<const FacetList*>(d + o_lists);
        p.allowed = as.words;
        p.allowed_stride = as.stride;
        p.masks = s->masks.p;
        p.mask_words = s->mask_words;
        p.n_masks = n_masks;
        p.n_buckets = (uint32_t)n_buckets;
        p.values = s->fields.p;
        p.btab = reinterpret_cast<const fp::BucketTable*>(d + o_bt);
        p.n_docs = s->n_docs;
        p.n_active = n_active;
        p.n_match = d_match;
        p.mask_counts = d_mc;
        p.bucket_counts = d_bc;
        for (const fp::Launch& l : launches) {
            p.blk0 = l.first;
            hipLaunchKernelGGL(k_facet_counts, dim3(l.count * n_active), dim3(FC_TPB), 0, st, p);
        }
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, turn.batch_ev.record(st));          // until here the call reads the turn's sets and tables
    if (dev_out) return SS_OK;                      // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    SS_HIP(ctx, hipMemcpyAsync(n_match_out, d_match, nq * sizeof(uint32_t), hipMemcpyDefault, st));
    if (n_mc) SS_HIP(ctx, hipMemcpyAsync(mask_counts_out, d_mc, n_mc * sizeof(uint32_t), hipMemcpyDefault, st));
    if (n_bc) SS_HIP(ctx, hipMemcpyAsync(bucket_counts_out, d_bc, n_bc * sizeof(uint32_t), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_facet_counts(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                        const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                        const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t n_buckets, const ss_doc_range* buckets,
                        uint32_t* n_match_out, uint32_t* mask_counts_out, uint32_t* bucket_counts_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return hw::guarded(s, "ss_facet_counts", [&] {
        return facet_impl(s, n_q, q_ptr, q_terms, mask_id, cons, ranges, n_buckets, buckets, n_match_out, mask_counts_out, bucket_counts_out);
    });
}

}  // extern "C"
