// similar.hip — ss_similar_topk: "similar pages" (DESIGN.md K4f).  The heaviest body terms of a seed doc become a query; the
// answer is that query's ranking without the seed itself.  A step file beside score_call.hip: it puts one kernel in front of the
// scoring call (k_doc_top_terms, doc_view.hip) and one behind it (k_drop_seed, here) and edits no scoring kernel.
//
//   checks                     k, m, the body view, the seeds, the mask ids, the prior — all before anything is enqueued
//   k_doc_top_terms            on the context's stream: terms [n_q][m] and their counts
//   one blocking copy          the terms come to the host (n_q * m * 4 bytes + the counts): the slice plan is made on the CPU
//   ss::score_into_turn        the fetch, plan, stage and enqueue steps of ss_score_topk_masked with k + 1; the rows stay in the
//                              block of the plan turn the call took
//   k_drop_seed                on the context's stream: an ordered copy of every row that skips the seed, cut to k; writes hits_out
//                              and n_hits_out (zero rows behind the last hit, as the scoring kernels leave them) and is the turn's
//                              last reader, so the turn's batch_ev is recorded again behind it
#include "scorer.hpp"

namespace {

constexpr int DS_WAVES = 4;                     // waves (= queries) per workgroup

// out row q = the first min(k, n - [seed in row]) hits of `rows` row q (k + 1 wide, n = n_rows[q] of them valid) without the hit
// whose doc is seeds[q]; a row holds a doc once.  Rows are copied as 8-byte words.
__global__ __launch_bounds__(DS_WAVES * 64) void k_drop_seed(const ss_hit* __restrict__ rows, const int32_t* __restrict__ n_rows,
                                                             const uint32_t* __restrict__ seeds, int32_t n_q, int32_t k,
                                                             ss_hit* __restrict__ hits_out, int32_t* __restrict__ n_hits_out) {
    static_assert(sizeof(ss_hit) == 40, "ss_hit rows are copied as 8-byte words");
    const int32_t q = (int32_t)(blockIdx.x * DS_WAVES + (threadIdx.x >> 6));
    if (q >= n_q) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k1 = (uint32_t)k + 1u;
    const ss_hit* __restrict__ src = rows + (size_t)q * k1;
    int32_t nr = n_rows[q];
    const uint32_t n = nr < 0 ? 0u : (uint32_t)nr > k1 ? k1 : (uint32_t)nr;
    const uint32_t seed = seeds[q];
    uint32_t pos = n;                           // the seed's place in the row, n = not there
    for (uint32_t j = lane; j < n; j += 64)
        if (src[j].doc == seed) pos = j;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(pos, off, 64);
        pos = o < pos ? o : pos;
    }
    const uint32_t left = n - (pos < n ? 1u : 0u);
    const uint32_t n_out = left < (uint32_t)k ? left : (uint32_t)k;
    const uint64_t* __restrict__ s8 = reinterpret_cast<const uint64_t*>(src);
    uint64_t* __restrict__ d8 = reinterpret_cast<uint64_t*>(hits_out + (size_t)q * (uint32_t)k);
    for (uint32_t e = lane; e < (uint32_t)k * 5u; e += 64) {
        const uint32_t j = e / 5u, f = e - j * 5u;
        d8[e] = j < n_out ? s8[(j + (j >= pos ? 1u : 0u)) * 5u + f] : 0ull;
    }
    if (lane == 0) n_hits_out[q] = (int32_t)n_out;
}

int32_t similar_impl(ss_scorer* s, int32_t n_q, const uint32_t* seeds, int32_t m, const double* topic_probs, const int32_t* mask_id, int32_t k,
                     ss_hit* hits_out, int32_t* n_hits_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- every check, before anything is enqueued
    if (n_q < 0 || (n_q && !seeds) || !hits_out || !n_hits_out) return ctx->fail(SS_ERR_INVALID, "ss_similar_topk: NULL argument or n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_similar_topk: k < 1");
    if (k > SS_MAX_TOPK - 1) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_similar_topk: k %d > SS_MAX_TOPK - 1 = %d (the seed's own row is scored too)", k, SS_MAX_TOPK - 1);
    if (m < 1 || m > SS_MAX_QUERY_TERMS) return ctx->fail(SS_ERR_INVALID, "ss_similar_topk: m = %d outside 1 .. %d", m, SS_MAX_QUERY_TERMS);
    if (!s->body->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_similar_topk: the body table has no doc view (ss_index_build_doc_view)");
    if (topic_probs && s->k_topics == 0) return ctx->fail(SS_ERR_STATE, "ss_similar_topk: topic_probs given but no prior set (ss_scorer_set_prior)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q, n_terms_max = nq * (size_t)m;
    std::vector<uint32_t> h_seeds(nq);
    SS_HIP(ctx, ss::copy_in(st, h_seeds.data(), seeds, nq * sizeof(uint32_t)));
    for (size_t q = 0; q < nq; q++)
        if ((uint64_t)h_seeds[q] >= s->body->n_docs)
            return ctx->fail(SS_ERR_INVALID, "ss_similar_topk: seed %zu is doc %u, the index has %llu docs", q, h_seeds[q], (unsigned long long)s->body->n_docs);
    std::vector<int32_t> h_mask;
    if (mask_id) {
        h_mask.resize(nq);
        SS_HIP(ctx, ss::copy_in(st, h_mask.data(), mask_id, nq * sizeof(int32_t)));
        for (size_t q = 0; q < nq; q++)
            if (h_mask[q] < -1 || h_mask[q] >= s->n_masks)
                return ctx->fail(SS_ERR_INVALID, "ss_similar_topk: query %zu has mask id %d (the scorer has %d masks)", q, h_mask[q], s->n_masks);
    }
    // ---- the seeds' terms
    // pinned block: terms [n_q][m] | counts [n_q] | seeds [n_q]
    const size_t cnt_off = align16(n_terms_max * sizeof(uint32_t)), seed_off = align16(cnt_off + nq * sizeof(int32_t));
    const size_t h_bytes = seed_off + nq * sizeof(uint32_t);
    SS_HIP(ctx, s->h_sim.ensure(h_bytes));
    unsigned char* const h_sim = s->h_sim.p;
    SS_HIP(ctx, ensure(s->d_sim_seeds, nq));
    SS_HIP(ctx, ensure(s->d_sim_terms, n_terms_max));
    SS_HIP(ctx, ensure(s->d_sim_cnt, nq));
    // (the seeds go up through the pinned block: an asynchronous copy; the wait for the terms below covers it)
    std::memcpy(h_sim + seed_off, h_seeds.data(), nq * sizeof(uint32_t));
    SS_HIP(ctx, hipMemcpyAsync(s->d_sim_seeds.p, h_sim + seed_off, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ss::launch_doc_top_terms(s->body, s->d_sim_seeds.p, (uint64_t)nq, m, s->d_sim_terms.p, nullptr, s->d_sim_cnt.p, st);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, hipMemcpyAsync(h_sim, s->d_sim_terms.p, n_terms_max * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipMemcpyAsync(h_sim + cnt_off, s->d_sim_cnt.p, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t* const h_terms = reinterpret_cast<const uint32_t*>(h_sim);
    const int32_t* const h_cnt = reinterpret_cast<const int32_t*>(h_sim + cnt_off);
    std::vector<uint32_t> q_ptr(nq + 1, 0), q_terms;
    q_terms.reserve(n_terms_max);
    for (size_t q = 0; q < nq; q++) {
        q_terms.insert(q_terms.end(), h_terms + q * (size_t)m, h_terms + q * (size_t)m + h_cnt[q]);
        q_ptr[q + 1] = (uint32_t)q_terms.size();
    }
    // ---- the scoring call with k + 1, rows in the turn's block
    TurnRows tr;
    if (const int32_t rc = ss::score_into_turn(s, n_q, q_ptr.data(), q_terms.data(), topic_probs, mask_id ? h_mask.data() : nullptr, k + 1, &tr)) {
        const std::string why = ctx->last_error;          // (the shared steps name ss_score_topk; nothing has touched the outputs)
        return ctx->fail(rc, "ss_similar_topk: scoring the seeds' terms at k + 1 failed: %s", why.c_str());
    }
    if (tr.turn < 0) return ctx->fail(SS_ERR_STATE, "ss_similar_topk: internal: the scoring call took no turn");
    // ---- drop the seed
    const bool dev_out = ss::on_device(hits_out) && ss::on_device(n_hits_out);
    if (!dev_out) {
        SS_HIP(ctx, ensure(s->d_hits, nq * (size_t)k));
        SS_HIP(ctx, ensure(s->d_nhits, nq));
    }
    ss_hit* const d_hits = dev_out ? hits_out : s->d_hits.p;
    int32_t* const d_n = dev_out ? n_hits_out : s->d_nhits.p;
    hipLaunchKernelGGL(k_drop_seed, dim3(ss::div_up(nq, DS_WAVES)), dim3(DS_WAVES * 64), 0, st, (const ss_hit*)tr.hits, (const int32_t*)tr.n_hits,
                       (const uint32_t*)s->d_sim_seeds.p, n_q, k, d_hits, d_n);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, s->turn[tr.turn].batch_ev.record(st));        // the turn's rows are read until here
    if (dev_out) return SS_OK;                          // ordered on the ctx stream, as ss_score_topk's device outputs
    SS_HIP(ctx, hipMemcpyAsync(hits_out, d_hits, nq * (size_t)k * sizeof(ss_hit), hipMemcpyDefault, st));
    SS_HIP(ctx, hipMemcpyAsync(n_hits_out, d_n, nq * sizeof(int32_t), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_similar_topk(ss_scorer* s, int32_t n_q, const uint32_t* seeds, int32_t m, const double* topic_probs, const int32_t* mask_id,
                        int32_t k, ss_hit* hits_out, int32_t* n_hits_out) {
    if (!s) return SS_ERR_INVALID;
    try {
        return similar_impl(s, n_q, seeds, m, topic_probs, mask_id, k, hits_out, n_hits_out);
    } catch (const std::bad_alloc&) {
        return s->ctx->fail(SS_ERR_OOM, "ss_similar_topk: host allocation failed");
    }
}

}  // extern "C"
