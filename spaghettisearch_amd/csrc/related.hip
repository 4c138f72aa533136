// related.hip — ss_related_terms: "related terms" of a query.  The heaviest body terms of a query's best pages,
// summed per term over the pages, without the words the user typed: the pseudo-relevance-feedback step, on the device from the
// hits to the selection.  A step file beside similar.hip: it puts three kernels behind the scoring call and edits no scoring kernel.
//
//   checks                     k_fb, m_doc, m, the body view, q_ptr — here; the mask ids, the prior and the queries themselves by the
//                              scoring call's own first steps: all before anything is enqueued
//   ss::score_into_turn        the fetch, plan, stage and enqueue steps of ss_score_topk_masked with k_fb; the rows stay in the
//                              block of the plan turn the call took
//   k_hit_docs                 docs [n_q][k_fb] of the rows (slots behind the last hit: doc 0, ignored downstream by their index)
//   k_doc_top_terms            (doc_view.hip, as it stands) terms, weights and counts [n_q * k_fb][m_doc]
//   k_related_terms            one workgroup per query: the entries (term, w, e = j * m_doc + i) sorted by (term, e) in LDS, every
//                              term's weights summed in float64 in ascending e (= ascending rank j, from 0.0), then m rounds of a
//                              workgroup-wide maximum over (ordered score, ~term) strictly below the previous winner; writes
//                              terms_out, score_out and n_out and is the turn's last reader, so the turn's batch_ev is recorded again
//                              behind it
// Everything runs on the context's stream and nothing comes back to the host: with device outputs the call never waits.  The
// queries' own terms go up through a pinned block of the turn (rewritten only after the wait for the turn's batch_ev).
#include "scorer.hpp"

#include <algorithm>

namespace {

constexpr int HD_TPB = 256;

// docs[q][j] = doc of hit j of row q (k_fb wide, n_rows[q] of them valid), 0 behind the last hit
__global__ __launch_bounds__(HD_TPB) void k_hit_docs(const ss_hit* __restrict__ rows, const int32_t* __restrict__ n_rows, uint32_t n_q,
                                                     uint32_t k_fb, uint32_t* __restrict__ docs) {
    const uint64_t i = (uint64_t)blockIdx.x * HD_TPB + threadIdx.x;
    if (i >= (uint64_t)n_q * k_fb) return;
    const uint32_t q = (uint32_t)(i / k_fb), j = (uint32_t)(i - (uint64_t)q * k_fb);
    const int32_t nr = n_rows[q];
    docs[i] = (nr > 0 && j < (uint32_t)nr) ? rows[i].doc : 0u;
}

// score descending as float64 values (-0 = +0), NaN below everything: larger key = earlier (doc_view.hip's ordered_weight, one width up)
__device__ __forceinline__ uint64_t ordered_score(double x) {
    if (x != x) return 0ull;
    if (x == 0.0) return 0x8000000000000000ull;           // both zeros: the key of +0
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);   // (~b = 0 only for a NaN's bits)
}

// selection keys are pairs (ordered score, ~term), compared score first
__device__ __forceinline__ bool key_less(uint64_t ah, uint32_t al, uint64_t bh, uint32_t bl) { return ah < bh || (ah == bh && al < bl); }

constexpr int RT_PER = 4;                                 // sorted positions per thread
constexpr uint64_t RT_DEAD = ~0ull;                       // the key of a slot that holds nothing: sorts behind every live key

// One workgroup of BLOCK threads per query; np = the power of two the query's k_fb * m_doc slots are padded to, np <= RT_PER * BLOCK.
// d_terms / d_w / d_cnt: k_doc_top_terms' rows of docs[q][0 .. k_fb).  qt_ptr [n_q + 1] into qt: the query's own (distinct) terms.
// Row q of the outputs = the first n_out[q] = min(m, candidates) candidates, score descending as float64 values, then ascending
// term id, NaN last; score_out (nullable) holds the sums' bits; entries past n_out[q] are not written.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_related_terms(const int32_t* __restrict__ n_rows, const uint32_t* __restrict__ d_terms,
                                                         const float* __restrict__ d_w, const int32_t* __restrict__ d_cnt,
                                                         const uint32_t* __restrict__ qt_ptr, const uint32_t* __restrict__ qt, uint32_t k_fb,
                                                         uint32_t m_doc, uint32_t m, uint32_t np, uint32_t* __restrict__ terms_out,
                                                         double* __restrict__ score_out, int32_t* __restrict__ n_out) {
    constexpr uint32_t CAP = RT_PER * BLOCK, WAVES = BLOCK / 64;
    __shared__ uint64_t s_key[CAP];                       // term << 32 | e
    __shared__ float s_w[CAP];                            // by e
    __shared__ uint32_t s_qt[SS_MAX_QUERY_TERMS];
    __shared__ uint64_t s_red_h[2][WAVES];
    __shared__ uint32_t s_red_l[2][WAVES];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n_slots = k_fb * m_doc;                // <= np <= CAP: checked by the launcher
    const int32_t nr = n_rows[q];
    const uint32_t n_hits = nr < 0 ? 0u : (uint32_t)nr > k_fb ? k_fb : (uint32_t)nr;
    const uint32_t qb = qt_ptr[q];
    uint32_t n_qt = qt_ptr[q + 1] - qb;
    n_qt = n_qt > (uint32_t)SS_MAX_QUERY_TERMS ? (uint32_t)SS_MAX_QUERY_TERMS : n_qt;
    if (tid < n_qt) s_qt[tid] = qt[qb + tid];
    __syncthreads();
    // ---- the slots: live ones get (term, e), the rest the key that sorts last
    const size_t row0 = (size_t)q * n_slots;
    for (uint32_t e = tid; e < np; e += BLOCK) {
        uint64_t key = RT_DEAD;
        if (e < n_slots) {
            const uint32_t j = e / m_doc, i = e - j * m_doc;
            if (j < n_hits) {
                const int32_t c = d_cnt[(size_t)q * k_fb + j];
                if (c > 0 && i < (uint32_t)c) {
                    const uint32_t t = d_terms[row0 + e];
                    bool typed = false;
                    for (uint32_t x = 0; x < n_qt; x++) typed = typed || s_qt[x] == t;
                    if (!typed) {
                        key = (uint64_t)t << 32 | e;
                        s_w[e] = d_w[row0 + e];
                    }
                }
            }
        }
        s_key[e] = key;
    }
    __syncthreads();
    // ---- bitonic sort of the keys, ascending: a term's entries end up side by side in ascending e
    for (uint32_t k2 = 2; k2 <= np; k2 <<= 1) {
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = tid; i < np; i += BLOCK) {
                const uint32_t o = i ^ j2;
                if (o > i) {
                    const uint64_t a = s_key[i], b = s_key[o];
                    if ((a > b) == ((i & k2) == 0)) {
                        s_key[i] = b;
                        s_key[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- the first entry of every term sums the term's weights in key order: ascending rank, one addend at a time from 0.0
    uint64_t c_h[RT_PER];                                 // this thread's candidates as selection keys; (0, 0) = none
    uint32_t c_l[RT_PER];
    double c_sum[RT_PER];
#pragma unroll
    for (int c = 0; c < RT_PER; c++) {
        const uint32_t p = tid + (uint32_t)c * BLOCK;
        c_h[c] = 0;
        c_l[c] = 0;
        c_sum[c] = 0.0;
        if (p >= np) continue;
        const uint64_t key = s_key[p];
        if (key == RT_DEAD) continue;
        const uint32_t t = (uint32_t)(key >> 32);
        if (p > 0 && (uint32_t)(s_key[p - 1] >> 32) == t) continue;
        double sum = 0.0;
        for (uint32_t pp = p; pp < np; pp++) {
            const uint64_t kk = s_key[pp];
            if (kk == RT_DEAD || (uint32_t)(kk >> 32) != t) break;
            sum += (double)s_w[(uint32_t)kk];
        }
        c_sum[c] = sum;
        c_h[c] = ordered_score(sum);
        c_l[c] = ~t;                                      // (never 0: no term has the id of SS_UNKNOWN_TERM)
    }
    // ---- m rounds of the workgroup-wide maximum strictly below the previous winner.  Candidates are distinct terms, so keys are
    // distinct and exactly one thread holds a round's winner.
    uint64_t prev_h = ~0ull;                              // no key reaches it (its score part would be a NaN's bits)
    uint32_t prev_l = ~0u;
    uint32_t n_sel = 0;
    for (uint32_t r = 0; r < m; r++) {
        uint64_t best_h = 0;
        uint32_t best_l = 0;
        double best_sum = 0.0;
#pragma unroll
        for (int c = 0; c < RT_PER; c++)
            if (key_less(c_h[c], c_l[c], prev_h, prev_l) && key_less(best_h, best_l, c_h[c], c_l[c])) {
                best_h = c_h[c];
                best_l = c_l[c];
                best_sum = c_sum[c];
            }
        uint64_t win_h = best_h;
        uint32_t win_l = best_l;
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t oh = __shfl_xor(win_h, off, 64);
            const uint32_t ol = __shfl_xor(win_l, off, 64);
            if (key_less(win_h, win_l, oh, ol)) {
                win_h = oh;
                win_l = ol;
            }
        }
        // (two sets of slots, taken in turn: a wave that runs ahead into round r + 1 writes the other set, and cannot reach round
        //  r + 2 before every wave has passed round r + 1's barrier, i.e. has read this round's set)
        if (lane == 0) {
            s_red_h[r & 1u][wave] = win_h;
            s_red_l[r & 1u][wave] = win_l;
        }
        __syncthreads();
        win_h = s_red_h[r & 1u][0];
        win_l = s_red_l[r & 1u][0];
#pragma unroll
        for (uint32_t v = 1; v < WAVES; v++) {
            const uint64_t oh = s_red_h[r & 1u][v];
            const uint32_t ol = s_red_l[r & 1u][v];
            if (key_less(win_h, win_l, oh, ol)) {
                win_h = oh;
                win_l = ol;
            }
        }
        if (win_h == 0 && win_l == 0) break;              // no candidate left (the same value in every thread)
        if (best_h == win_h && best_l == win_l) {
            terms_out[(size_t)q * m + r] = ~best_l;
            if (score_out) score_out[(size_t)q * m + r] = best_sum;
        }
        prev_h = win_h;
        prev_l = win_l;
        n_sel++;
    }
    if (tid == 0) n_out[q] = (int32_t)n_sel;
}

constexpr int RT_SMALL = 256, RT_LARGE = 1024;            // threads per query: up to 1024 slots, and up to 4096
static_assert(RT_PER * RT_LARGE >= SS_MAX_FEEDBACK_DOCS * SS_MAX_QUERY_TERMS, "k_related_terms holds k_fb * m_doc slots in LDS");

int32_t related_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                     const double* topic_probs, const int32_t* mask_id, int32_t k_fb, int32_t m_doc, int32_t m, uint32_t* terms_out,
                     double* score_out, int32_t* n_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks of this call; the scoring call below makes its own (mask ids, the prior, the queries) before it enqueues anything
    if (n_q < 0 || !q_ptr || !terms_out || !n_out) return ctx->fail(SS_ERR_INVALID, "ss_related_terms: NULL argument or n_q < 0");
    if (k_fb < 1 || k_fb > SS_MAX_FEEDBACK_DOCS) return ctx->fail(SS_ERR_INVALID, "ss_related_terms: k_fb = %d outside 1 .. %d", k_fb, SS_MAX_FEEDBACK_DOCS);
    if (m_doc < 1 || m_doc > SS_MAX_QUERY_TERMS) return ctx->fail(SS_ERR_INVALID, "ss_related_terms: m_doc = %d outside 1 .. %d", m_doc, SS_MAX_QUERY_TERMS);
    if (m < 1 || m > SS_MAX_QUERY_TERMS) return ctx->fail(SS_ERR_INVALID, "ss_related_terms: m = %d outside 1 .. %d", m, SS_MAX_QUERY_TERMS);
    if (!s->body->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_related_terms: the body table has no doc view (ss_index_build_doc_view)");
    if (topic_probs && s->k_topics == 0) return ctx->fail(SS_ERR_STATE, "ss_related_terms: topic_probs given but no prior set (ss_scorer_set_prior)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, "ss_related_terms", "q", q_ptr, nq, h_ptr.data()));
    const size_t n_tok = h_ptr[nq];
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "ss_related_terms: q_terms is NULL");
    std::vector<uint32_t> h_terms(n_tok);
    SS_HIP(ctx, ss::copy_in(st, h_terms.data(), q_terms, n_tok * sizeof(uint32_t)));
    // ---- the scoring call with k_fb, rows in the turn's block
    TurnRows tr;
    if (const int32_t rc = ss::score_into_turn(s, n_q, h_ptr.data(), h_terms.data(), topic_probs, mask_id, k_fb, &tr, query_len)) {
        const std::string why = ctx->last_error;          // (the shared steps name ss_score_topk; nothing has touched the outputs)
        return ctx->fail(rc, "ss_related_terms: scoring the queries at k_fb failed: %s", why.c_str());
    }
    if (tr.turn < 0) return ctx->fail(SS_ERR_STATE, "ss_related_terms: internal: the scoring call took no turn");
    // From here on the turn is taken: whatever happens, the turn's batch_ev stays recorded behind the scoring kernels (enqueue did that),
    // and is recorded again behind k_related_terms, the last reader of the turn's rows and of the turn's pinned block.
    // ---- the queries' own terms, each once (the scoring call has accepted them: at most SS_MAX_QUERY_TERMS distinct per query)
    // pinned block of the turn and its device copy: ptr [n_q + 1] | terms
    Turn& turn = s->turn[tr.turn];
    const size_t q_words = nq + 1 + n_tok;
    SS_HIP(ctx, turn.h_rel.ensure(q_words * sizeof(uint32_t)));
    uint32_t* const hq = turn.h_rel.as<uint32_t>();
    uint32_t* const hq_terms = hq + nq + 1;
    uint32_t n_own = 0;
    for (size_t q = 0; q < nq; q++) {
        hq[q] = n_own;
        for (uint32_t x = h_ptr[q]; x < h_ptr[q + 1]; x++)
            if (std::find(hq_terms + hq[q], hq_terms + n_own, h_terms[x]) == hq_terms + n_own) hq_terms[n_own++] = h_terms[x];
    }
    hq[nq] = n_own;
    const size_t n_docs_fb = nq * (size_t)k_fb, n_slots = n_docs_fb * (size_t)m_doc, n_rows_out = nq * (size_t)m;
    SS_HIP(ctx, ensure(s->d_rel_q, q_words));
    SS_HIP(ctx, ensure(s->d_rel_docs, n_docs_fb));
    SS_HIP(ctx, ensure(s->d_rel_cnt, n_docs_fb));
    SS_HIP(ctx, ensure(s->d_rel_terms, n_slots));
    SS_HIP(ctx, ensure(s->d_rel_w, n_slots));
    // outputs in device memory are written by the kernel itself; an output in host memory gets a device block and only the entries
    // the kernel wrote are copied out (entries past n_out[q] stay as the caller left them)
    const bool dev_t = ss::on_device(terms_out), dev_s = score_out && ss::on_device(score_out), dev_n = ss::on_device(n_out);
    if (!dev_t) SS_HIP(ctx, ensure(s->d_rel_out_terms, n_rows_out));
    if (score_out && !dev_s) SS_HIP(ctx, ensure(s->d_rel_out_score, n_rows_out));
    if (!dev_n) SS_HIP(ctx, ensure(s->d_nhits, nq));
    uint32_t* const o_terms = dev_t ? terms_out : s->d_rel_out_terms.p;
    double* const o_score = !score_out ? nullptr : dev_s ? score_out : s->d_rel_out_score.p;
    int32_t* const o_n = dev_n ? n_out : s->d_nhits.p;
    // ---- the pipeline
    SS_HIP(ctx, hipMemcpyAsync(s->d_rel_q.p, hq, (nq + 1 + n_own) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hit_docs, dim3(ss::div_up(n_docs_fb, HD_TPB)), dim3(HD_TPB), 0, st, (const ss_hit*)tr.hits, (const int32_t*)tr.n_hits,
                       (uint32_t)n_q, (uint32_t)k_fb, s->d_rel_docs.p);
    ss::launch_doc_top_terms(s->body, s->d_rel_docs.p, (uint64_t)n_docs_fb, m_doc, s->d_rel_terms.p, s->d_rel_w.p, s->d_rel_cnt.p, st);
    uint32_t np = 2;
    while (np < (uint32_t)k_fb * (uint32_t)m_doc) np <<= 1;
    const uint32_t* const d_qptr = s->d_rel_q.p;
    const uint32_t* const d_qt = s->d_rel_q.p + nq + 1;
    if (np <= (uint32_t)(RT_PER * RT_SMALL))
        hipLaunchKernelGGL(k_related_terms<RT_SMALL>, dim3((unsigned)n_q), dim3(RT_SMALL), 0, st, (const int32_t*)tr.n_hits,
                           (const uint32_t*)s->d_rel_terms.p, (const float*)s->d_rel_w.p, (const int32_t*)s->d_rel_cnt.p, d_qptr, d_qt,
                           (uint32_t)k_fb, (uint32_t)m_doc, (uint32_t)m, np, o_terms, o_score, o_n);
    else
        hipLaunchKernelGGL(k_related_terms<RT_LARGE>, dim3((unsigned)n_q), dim3(RT_LARGE), 0, st, (const int32_t*)tr.n_hits,
                           (const uint32_t*)s->d_rel_terms.p, (const float*)s->d_rel_w.p, (const int32_t*)s->d_rel_cnt.p, d_qptr, d_qt,
                           (uint32_t)k_fb, (uint32_t)m_doc, (uint32_t)m, np, o_terms, o_score, o_n);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.batch_ev.record(st));                // the turn's rows and pinned block are read until here
    if (dev_t && dev_n && (!score_out || dev_s)) return SS_OK;   // ordered on the ctx stream; nothing comes back, nothing is waited for
    // ---- host outputs
    const bool host_rows = !dev_t || (score_out && !dev_s);
    std::vector<int32_t> h_n(nq);
    std::vector<uint32_t> h_out_terms;
    std::vector<double> h_out_score;
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), o_n, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_t) {
        h_out_terms.resize(n_rows_out);
        SS_HIP(ctx, hipMemcpyAsync(h_out_terms.data(), o_terms, n_rows_out * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (score_out && !dev_s) {
        h_out_score.resize(n_rows_out);
        SS_HIP(ctx, hipMemcpyAsync(h_out_score.data(), o_score, n_rows_out * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_out, h_n.data(), nq * sizeof(int32_t));
    for (size_t q = 0; q < nq && host_rows; q++) {
        const size_t cnt = (size_t)h_n[q], o = q * (size_t)m;
        if (!dev_t) std::memcpy(terms_out + o, h_out_terms.data() + o, cnt * sizeof(uint32_t));
        if (score_out && !dev_s) std::memcpy(score_out + o, h_out_score.data() + o, cnt * sizeof(double));
    }
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_related_terms(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                         const double* topic_probs, const int32_t* mask_id, int32_t k_fb, int32_t m_doc, int32_t m, uint32_t* terms_out,
                         double* score_out, int32_t* n_out) {
    if (!s) return SS_ERR_INVALID;
    try {
        return related_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, mask_id, k_fb, m_doc, m, terms_out, score_out, n_out);
    } catch (const std::bad_alloc&) {
        return s->ctx->fail(SS_ERR_OOM, "ss_related_terms: host allocation failed");
    }
}

}  // extern "C"
