// group_topk.hip — ss_top_groups and ss_scorer_group_values: the m groups ("sites") of the doc -> group table that hold most of a
// query's matches, counted over ALL docs the query matches.  DESIGN.md K4u; no reference counterpart.
//
// The group ranks turn every 32-bit group value into an array index: gval = the table's distinct values != SS_NO_GROUP ascending (a
// rocprim sort of a copy of the table and a unique pass), grank[d] = the index of group[d] in gval (k_group_ranks, a binary search per
// doc).  They are built by the first call that needs them after ss_scorer_set_doc_groups, which waits once, and dropped with the table.
//
// M(q) is ss_facet_counts' match set, formed by the code that call uses (match_set.hpp).  k_group_count gives a workgroup a RUN of
// consecutive 32768-doc blocks of one query and forms the match words per block (match_set.hpp, steps 1 to 3, warm bounds along the run).
// For every set bit it gathers grank[d]; a thread walks its 128 docs in ascending order and merges consecutive equal ranks into one
// add.  The adds go to a histogram in LDS that joins the query's counter row at the end of the run (tables of at most
// "gtopk.lds_groups" values), or straight to the row by non-returning global atomics.  The row's two extra slots take the run's matches
// and its SS_NO_GROUP matches.  k_group_select, one workgroup per query, streams the row and offers key = (0xFFFFFFFF - cnt) << 32 | rank
// of every non-zero counter to a running best first + m (match_set.hpp's BestK over keys alone) and writes the page.  Integer atomics
// only, and a total order of the keys: no arrival order can show.
#include "group_topk_plan.hpp"
#include "match_set.hpp"

#include <rocprim/rocprim.hpp>

namespace gp = ss::gtopk;
namespace hw = ss::hitwin;
namespace ms = ss::mset;

static_assert(gp::NO_RANK == SS_NO_GROUP, "group_topk_plan.hpp restates the ABI's limits");
static_assert(sizeof(ss_group_count) == 8, "ss_group_count layout");

namespace {

constexpr int GT_TPB = (int)ms::THREADS;
constexpr int GT_WPT = (int)ms::WORDS_PER_THREAD;
constexpr int GT_WAVES = GT_TPB / 64;

struct CountParams {
    ss::MatchSetArgs match;
    const uint32_t* grank;            // [n_docs]
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
    __shared__ uint64_t cur[ms::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[ms::BLOCK_WORDS];   // the block's docs with a posting of the query
    __shared__ uint32_t wsum[GT_WAVES][2];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.match.lptr[a], nl = p.match.lptr[a + 1] - l0;      // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint32_t b0 = ms::run_begin(r, p.R, p.n_blocks), b1 = ms::run_begin(r + 1, p.R, p.n_blocks);
    uint32_t* const row = p.rows + (uint64_t)al * p.stride;
    if (LDS) {
        for (uint32_t i = tid; i < p.n_groups; i += GT_TPB) gt_hist[i] = 0u;   // (the barrier of step 2 stands before the first add)
    }
    uint32_t matches = 0, ungrouped = 0;                                     // of this thread's words, over the run
    for (uint32_t blk = b0; blk < b1; blk++) {
        // ---- 1 to 3. the block's match words (match_set.hpp)
        if (blk == b0) ms::runs_cold(p.match, l0, nl, blk, cur);
        else ms::runs_warm(p.match, l0, nl, blk, cur);
        if (!ms::or_image(p.match, l0, nl, blk, cur, img)) continue;         // no list reaches the block
        const uint64_t w0 = ms::word_begin(blk);                             // this thread's first word
        uint32_t m[GT_WPT];
        matches += ms::and_allowed(m, p.match, a, blk, img);
        // ---- 4. the ranks of the set bits, ascending by doc: consecutive equal ranks become one add
        uint32_t run_rank = gp::NO_RANK, run_len = 0;
#pragma unroll
        for (int i = 0; i < GT_WPT; i++) {
            uint32_t bits = m[i];
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
    matches = ms::wave_sum(matches);
    ungrouped = ms::wave_sum(ungrouped);
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

// Grid: one workgroup per active query of the group.  Dynamic LDS: cap keys.
__global__ __launch_bounds__(GT_TPB) void k_group_select(SelectParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gt_dyn[];
    __shared__ ms::BestHead head;
    __shared__ uint32_t wsum[GT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x, q = p.aq[p.a0 + al];
    const ms::BestK<false> best(&head, gt_dyn, p.cap, p.K);
    __syncthreads();
    const uint32_t* const row = p.rows + (uint64_t)al * p.stride;            // 16-byte aligned: the stride is a multiple of four words
    const uint4* const row4 = reinterpret_cast<const uint4*>(row);
    const uint64_t n4 = ((uint64_t)p.n_groups + 3) >> 2;                     // <= stride / 4
    uint64_t x = (uint64_t)tid;
    uint32_t j = 0, nz = 0;
    best.drain([&](auto offer) {                    // the row's non-zero counters
        for (; x < n4; x += GT_TPB, j = 0) {
            const uint4 u = row4[x];
            const uint32_t c[4] = {u.x, u.y, u.z, u.w};
            for (; j < 4; j++) {
                const uint64_t idx = x * 4 + j;
                if (idx >= p.n_groups || !c[j]) continue;                    // (the two extra slots and the padding are no counters)
                if (!offer(gp::pack_key(c[j], (uint32_t)idx), 0u)) return true;
                nz++;
            }
        }
        return false;
    });
    best.compact();
    const uint32_t n_page = hw::page_len(head.cnt, p.first, p.m);
    for (uint32_t i = tid; i < n_page; i += GT_TPB) {
        const uint64_t key = best.key[p.first + i];
        p.groups_out[(uint64_t)q * p.m + i] = ss_group_count{p.gval[gp::key_rank(key)], gp::key_count(key)};
    }
    nz = ms::wave_sum(nz);
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
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    ss::MatchCall mc;
    SS_TRY(ss::open_match_call(s, entry, n_q, q_ptr, q_terms, mask_id, cons, ranges, &mc));
    // ---- nothing below refuses an argument
    SS_TRY(ensure_group_ranks(s));                  // (the first call after a registration builds them and waits once)
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[mc.as.turn];
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
    const uint32_t n_active = (uint32_t)mc.ml.aq.size(), n_blocks = ms::blocks(s->n_docs), n_groups = s->n_groups;
    if (n_active && n_blocks) {
        const uint32_t K = (uint32_t)first + (uint32_t)m, cap = ms::buffer_entries(K), lds = gp::buffer_lds_bytes(K);
        const uint32_t R = ms::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("gtopk.runs", 0));
        const bool use_lds = gp::use_lds(n_groups, ctx->opt("gtopk.lds_groups", gp::DEFAULT_LDS_GROUPS));
        const uint64_t stride = gp::row_stride(n_groups);
        const uint32_t group = gp::group_queries(n_active, n_groups, gp::scratch_bytes_of(ctx->opt("gtopk.scratch_bytes", 0)));
        const size_t row_words = (size_t)group * stride;
        SS_HIP(ctx, ensure(s->d_gtopk_rows, row_words));
        ss::MatchTables mt;
        SS_TRY(ss::stage_match_tables(s, mc, nullptr, 0, &mt));
        CountParams cp{};
        cp.match = mt.args;
        cp.grank = s->grank.p;
        cp.n_blocks = n_blocks;
        cp.R = R;
        cp.n_groups = n_groups;
        cp.stride = stride;
        cp.rows = s->d_gtopk_rows.p;
        SelectParams sp{};
        sp.aq = mt.aq;
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
        for (const ms::Group& g : ms::groups(n_active, group)) {                // one group after another: they share the counter rows
            cp.a0 = sp.a0 = g.first;
            cp.n_group = g.count;
            SS_HIP(ctx, hipMemsetAsync(cp.rows, 0, (size_t)g.count * stride * sizeof(uint32_t), st));
            for (const ms::Launch& l : ms::launches(R, g.count)) {
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
    SS_HIP(ctx, hw::give_rows(groups_out, h_out.data(), nq, (size_t)m, sizeof(ss_group_count), h_n));
    SS_HIP(ctx, hw::give_rows(n_out, h_out.data() + o_n, nq, 1, sizeof(int32_t), nullptr));
    if (n_groups_out) SS_HIP(ctx, hw::give_rows(n_groups_out, h_out.data() + o_ng, nq, 1, sizeof(uint32_t), nullptr));
    if (n_ungrouped_out) SS_HIP(ctx, hw::give_rows(n_ungrouped_out, h_out.data() + o_ug, nq, 1, sizeof(uint32_t), nullptr));
    if (n_match_out) SS_HIP(ctx, hw::give_rows(n_match_out, h_out.data() + o_match, nq, 1, sizeof(uint32_t), nullptr));
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
