// field_topk.hip — ss_field_topk: the exact top-k of ALL docs a query matches, ordered by a doc field ("newest first" over every match,
// not over a relevance window).  DESIGN.md K4t; no reference counterpart.
//
// M(q) is ss_facet_counts' match set, formed by the code that call uses (match_set.hpp).  k_field_select gives a workgroup a RUN of
// consecutive 32768-doc blocks of one query.  Per block it forms the match words (match_set.hpp, steps 1 to 3; the bounds of a block's
// runs are searched from the previous block's ends, not cold) and puts them back into the LDS image for the resumable walk of step 4:
// for every set bit it gathers value[field][d], forms the key (field_topk_plan.hpp) and offers it to the workgroup's running best-K
// (match_set.hpp's BestK over (key, doc): a candidate buffer in LDS, compacted to its K = first + k smallest entries by a bitonic sort
// whenever it is full, and a threshold: exact whatever the arrival order).  The run's K smallest keys and its match count go to a
// partial list.  k_field_merge, one workgroup per query, pushes the R partial lists through the same best-K and writes the page, n_out
// and the summed match count.  No atomics on any output; the total order of the keys (value, then doc id) leaves nothing for an
// arrival order to decide.
#include "field_topk_plan.hpp"
#include "match_set.hpp"

namespace tp = ss::ftopk;
namespace hw = ss::hitwin;
namespace ms = ss::mset;

namespace {

constexpr int FT_TPB = (int)ms::THREADS;
constexpr int FT_WPT = (int)ms::WORDS_PER_THREAD;
constexpr int FT_WAVES = FT_TPB / 64;
using Best = ms::BestK<true>;                       // entries (key, doc)

struct SelectParams {
    ss::MatchSetArgs match;
    const int64_t* col;               // value[field]: [n_docs]
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

// Grid: blockIdx.x = (run - run0) * n_group + query — the queries of one run are neighbours, so the run's allowed words and field
// values come from L2 for all but the first of them.  Dynamic LDS: cap keys, then cap doc ids.
__global__ __launch_bounds__(FT_TPB) void k_field_select(SelectParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ft_dyn[];
    __shared__ uint64_t cur[ms::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[ms::BLOCK_WORDS];   // the block's docs with a posting of the query, then its matches
    __shared__ ms::BestHead head;
    __shared__ uint32_t wsum[FT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.match.lptr[a], nl = p.match.lptr[a + 1] - l0;      // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint32_t b0 = ms::run_begin(r, p.R, p.n_blocks), b1 = ms::run_begin(r + 1, p.R, p.n_blocks);
    const Best best(&head, ft_dyn, p.cap, p.K);                              // (the barrier of step 2 stands before the first drain)
    const bool desc = p.desc != 0;
    uint32_t matches = 0;                                                    // of this thread's words, over the run
    for (uint32_t blk = b0; blk < b1; blk++) {
        // ---- 1 to 3. the block's match words (match_set.hpp); they go back to the image (each thread reads its own words only)
        if (blk == b0) ms::runs_cold(p.match, l0, nl, blk, cur);
        else ms::runs_warm(p.match, l0, nl, blk, cur);
        if (!ms::or_image(p.match, l0, nl, blk, cur, img)) continue;         // no list reaches the block
        const uint64_t w0 = ms::word_begin(blk);                             // this thread's first word
        uint32_t m[FT_WPT];
        const uint32_t cnt = ms::and_allowed(m, p.match, a, blk, img);
        *reinterpret_cast<uint4*>(&img[tid * FT_WPT]) = make_uint4(m[0], m[1], m[2], m[3]);
        matches += cnt;
        if (!__syncthreads_or(cnt != 0)) continue;   // the allowed set left nothing of the block
        // ---- 4. the candidates: the key of every set bit
        uint32_t wi = 0, bits = m[0];
        best.drain([&](auto offer) {
            for (;;) {
                while (!bits && wi + 1 < FT_WPT) bits = img[tid * FT_WPT + ++wi];
                if (!bits) return false;
                const uint32_t d = (uint32_t)((w0 + wi) * 32) + (uint32_t)(__ffs(bits) - 1);     // < n_docs < 2^32
                if (!offer(tp::value_key(p.col[d], desc), d)) return true;
                bits &= bits - 1;
            }
        });
    }
    // ---- the run's list: its K smallest keys in order, and its counts
    __syncthreads();
    best.compact();
    const uint32_t n = head.cnt;
    const uint64_t slot = (uint64_t)al * p.R + r;
    for (uint32_t i = tid; i < n; i += FT_TPB) {
        p.part_key[slot * p.K + i] = best.key[i];
        p.part_doc[slot * p.K + i] = best.doc[i];
    }
    matches = ms::wave_sum(matches);
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
    __shared__ ms::BestHead head;
    __shared__ uint32_t wsum[FT_WAVES];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x, q = p.aq[p.a0 + al];
    const Best best(&head, ft_dyn, p.cap, p.K);
    const uint32_t* const rc = p.run_cnt + (uint64_t)al * p.R * 2;
    uint32_t total = 0;
    for (uint32_t r = tid; r < p.R; r += FT_TPB) total += rc[r * 2];
    total = ms::wave_sum(total);
    if ((tid & 63) == 0) wsum[tid >> 6] = total;
    __syncthreads();
    const uint64_t n_slots = (uint64_t)p.R * p.K, e0 = (uint64_t)al * n_slots;
    uint64_t x = (uint64_t)tid;
    best.drain([&](auto offer) {                    // the entries of the R partial lists
        for (; x < n_slots; x += FT_TPB) {
            const uint32_t r = (uint32_t)(x / p.K), j = (uint32_t)(x - (uint64_t)r * p.K);
            if (j < rc[r * 2 + 1] && !offer(p.part_key[e0 + x], p.part_doc[e0 + x])) return true;
        }
        return false;
    });
    best.compact();
    const uint32_t n_page = hw::page_len(head.cnt, p.first, p.k);
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

int32_t field_topk_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id, const QueryConstraints& cons,
                        const QueryRanges& ranges, int32_t field, int32_t descending, int32_t first, int32_t k, uint32_t* docs_out, int32_t* n_out,
                        int64_t* values_out, uint32_t* n_match_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_field_topk";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = tp::check_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, docs_out != nullptr, n_out != nullptr, field, first, k, s->n_fields))
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    ss::MatchCall mc;
    SS_TRY(ss::open_match_call(s, entry, n_q, q_ptr, q_terms, mask_id, cons, ranges, &mc));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[mc.as.turn];
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
    const uint32_t n_active = (uint32_t)mc.ml.aq.size(), n_blocks = ms::blocks(s->n_docs);
    if (n_active && n_blocks) {
        const uint32_t K = (uint32_t)first + (uint32_t)k, cap = ms::buffer_entries(K), lds = tp::buffer_lds_bytes(K);
        const uint32_t R = ms::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("ftopk.runs", 0));
        const uint32_t group = tp::group_queries(n_active, R, K, tp::scratch_bytes_of(ctx->opt("ftopk.scratch_bytes", 0)));
        // the partial lists of one group: keys | doc ids | run counts
        const size_t slots = (size_t)group * R, o_pdoc = slots * K * sizeof(uint64_t), o_rc = o_pdoc + slots * K * sizeof(uint32_t),
                     part_bytes = o_rc + slots * 2 * sizeof(uint32_t);
        SS_HIP(ctx, ensure(s->d_ftopk_part, part_bytes));
        ss::MatchTables mt;
        SS_TRY(ss::stage_match_tables(s, mc, nullptr, 0, &mt));
        unsigned char* const part = s->d_ftopk_part.p;
        SelectParams sp{};
        sp.match = mt.args;
        sp.col = s->fields.p + (size_t)field * s->n_docs;
        sp.n_blocks = n_blocks;
        sp.R = R;
        sp.K = K;
        sp.cap = cap;
        sp.desc = descending != 0;
        sp.part_key = reinterpret_cast<uint64_t*>(part);
        sp.part_doc = reinterpret_cast<uint32_t*>(part + o_pdoc);
        sp.run_cnt = reinterpret_cast<uint32_t*>(part + o_rc);
        MergeParams mp{};
        mp.aq = mt.aq;
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
        for (const ms::Group& g : ms::groups(n_active, group)) {                // one group after another: they share the partial lists
            sp.a0 = mp.a0 = g.first;
            sp.n_group = g.count;
            for (const ms::Launch& l : ms::launches(R, g.count)) {
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
    SS_HIP(ctx, hw::give_rows(docs_out, h_out.data() + o_docs, nq, (size_t)k, sizeof(uint32_t), h_n));
    if (values_out) SS_HIP(ctx, hw::give_rows(values_out, h_out.data(), nq, (size_t)k, sizeof(int64_t), h_n));
    SS_HIP(ctx, hw::give_rows(n_out, h_out.data() + o_n, nq, 1, sizeof(int32_t), nullptr));
    if (n_match_out) SS_HIP(ctx, hw::give_rows(n_match_out, h_out.data() + o_match, nq, 1, sizeof(uint32_t), nullptr));
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
