// facet.hip — ss_facet_counts: how many docs a query matches, in all, per registered allow-list and per value bucket of a doc field
// (no reference counterpart).
//
// M(q) is formed by match_set.hpp, which the call shares with ss_field_topk and ss_top_groups: the docs with a posting of any usable
// query term AND the allowed set of the scoring path AND d < n_docs.  k_facet_counts never writes M(q) out.  A workgroup owns one block
// of 32768 docs of one query: it forms the block's match words (match_set.hpp, steps 1 to 3, the runs searched cold) and reduces them:
// one popcount for the total, one popcount of image & mask_m per registered mask, and for the buckets one gather of value[field][d]
// per SET bit and field, placed by one binary search among the elementary intervals of the buckets' bounds (facet_plan.hpp) into an
// LDS histogram.  The block's partial counts join the outputs by integer atomicAdd behind a zeroing memset: exact and independent of
// the order.
#include "facet_plan.hpp"
#include "match_set.hpp"

namespace fp = ss::facetp;
namespace hw = ss::hitwin;
namespace ms = ss::mset;

static_assert(fp::MAX_BUCKETS == SS_MAX_FACET_BUCKETS && fp::MAX_FIELDS == SS_MAX_DOC_FIELDS, "facet_plan.hpp restates the ABI's limits");
static_assert(sizeof(fp::Range) == sizeof(ss_doc_range) && offsetof(fp::Range, field) == offsetof(ss_doc_range, field) &&
                  offsetof(fp::Range, lo) == offsetof(ss_doc_range, lo) && offsetof(fp::Range, hi) == offsetof(ss_doc_range, hi),
              "facet_plan.hpp restates ss_doc_range");

namespace {

constexpr int FC_TPB = (int)ms::THREADS;
constexpr int FC_WPT = (int)ms::WORDS_PER_THREAD;
constexpr int FC_WAVES = FC_TPB / 64;
constexpr int FC_CHUNK = 64;                        // counters (total, masks) that share one pass through the waves' partial sums

struct FacetParams {
    ss::MatchSetArgs match;
    const uint32_t* aq;               // [n_active] the queries that have a list
    const uint32_t* masks;            // the registered allow-lists [n_masks][mask_words]; n_masks 0: no mask counts
    uint64_t mask_words;
    uint32_t n_masks;
    uint32_t n_buckets;
    const int64_t* values;            // the field table [n_fields][n_docs]
    const fp::BucketTable* btab;
    uint32_t n_active, blk0;          // this launch: doc blocks from blk0
    uint32_t* n_match;                // [n_q]
    uint32_t* mask_counts;            // [n_q][n_masks]
    uint32_t* bucket_counts;          // [n_q][n_buckets]
};

// Grid: blockIdx.x = block * n_active + query — the queries of one doc block are neighbours, so the block's mask words and field
// values come from L2 for all but the first of them.
__global__ __launch_bounds__(FC_TPB) void k_facet_counts(FacetParams p) {
    __shared__ uint64_t cur[ms::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[ms::BLOCK_WORDS];   // the block's docs with a posting of the query
    __shared__ uint32_t wsum[FC_CHUNK][FC_WAVES];                            // the waves' partial sums of up to FC_CHUNK counters
    __shared__ int64_t cuts[fp::MAX_CUTS];                                   // the buckets' elementary intervals and their histogram
    __shared__ uint32_t hist[fp::MAX_CUTS];
    const int tid = threadIdx.x;
    const uint32_t a = blockIdx.x % p.n_active, blk = p.blk0 + blockIdx.x / p.n_active;
    const uint32_t l0 = p.match.lptr[a], nl = p.match.lptr[a + 1] - l0;            // 1 .. MAX_LISTS (the host leaves out a query without lists)
    // ---- 1 to 3. the block's match words (match_set.hpp)
    ms::runs_cold(p.match, l0, nl, blk, cur);
    if (!ms::or_image(p.match, l0, nl, blk, cur, img)) return;                  // no list reaches the block
    const uint64_t w0 = ms::word_begin(blk);                                 // this thread's first word
    uint32_t m[FC_WPT];
    const uint32_t cnt = ms::and_allowed(m, p.match, a, blk, img);
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
            v = ms::wave_sum(v);
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
        const int64_t* const col = p.values + (uint64_t)f * p.match.n_docs;
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
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    std::vector<ss_doc_range> bk((size_t)n_buckets);
    if (n_buckets) SS_HIP(ctx, ss::copy_in(ctx->stream, bk.data(), buckets, bk.size() * sizeof(ss_doc_range)));
    if (const int rc = fp::check_buckets(msg, sizeof(msg), entry, reinterpret_cast<const fp::Range*>(bk.data()), n_buckets, s->n_fields))
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    ss::MatchCall mc;
    SS_TRY(ss::open_match_call(s, entry, n_q, q_ptr, q_terms, mask_id, cons, ranges, &mc));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[mc.as.turn];
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
    const uint32_t n_active = (uint32_t)mc.ml.aq.size();
    const std::vector<ms::Launch> launches = ms::launches(ms::blocks(s->n_docs), n_active);
    if (!launches.empty()) {
        fp::BucketTable bt;
        fp::build_bucket_table(reinterpret_cast<const fp::Range*>(bk.data()), n_buckets, bt);
        ss::MatchTables mt;
        SS_TRY(ss::stage_match_tables(s, mc, &bt, sizeof(bt), &mt));
        FacetParams p{};
        p.match = mt.args;
        p.aq = mt.aq;
        p.masks = s->masks.p;
        p.mask_words = s->mask_words;
        p.n_masks = n_masks;
        p.n_buckets = (uint32_t)n_buckets;
        p.values = s->fields.p;
        p.btab = reinterpret_cast<const fp::BucketTable*>(mt.extra);
        p.n_active = n_active;
        p.n_match = d_match;
        p.mask_counts = d_mc;
        p.bucket_counts = d_bc;
        for (const ms::Launch& l : launches) {
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
