// explain.hip — ss_explain_hits: which query tokens matched each result row, and where.  For every (hit, token) of a
// batch: the stored weight of the (term, doc) posting in the title and in the body table, whether it exists, and the earliest
// non-negative body position.  A step file beside related.hip: one kernel behind whatever scoring call made the rows, no scoring
// kernel edited.
//
//   checks                     arguments, q_ptr, t_stride, host n_hits — all before anything is enqueued
//   the queries' table         ptr [n_q + 1] | tokens, through one of the TURNS explain turns (hit_window.hpp: query_table_fill)
//   k_explain_hits             one lane per entry (query q, hit j, token i).  Inside a query the lanes run over j fastest, so the 64
//                              lanes of a wave search the SAME two lists (one token, title and body) for 64 docs: the probes of the
//                              upper levels fall into shared cache lines and every lane runs the same number of steps.  A lane runs its
//                              title and its body search side by side (two independent loads in flight per step), then reads the two
//                              weights.  Position lists of up to EX_OWN values are read by their own lane; longer ones are taken one
//                              at a time by the whole wave, 64 values per step, and reduced with shuffles.  Every entry is written by
//                              exactly one lane; nothing else is written.
// The window in and the way back of a host `out`: hit_window.hpp.
#include "hit_window.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

constexpr int EX_TPB = 256;
constexpr uint32_t EX_OWN = 16;                           // position lists up to this length are read by their own lane
constexpr uint32_t EX_NONE = 0xFFFFFFFFu;                 // position key of "no value >= 0" (keys are bits of non-NaN floats >= 0)

struct ExplainParams {
    const uint64_t *t_ptr, *b_ptr;                        // term_ptr of the title / body table
    const uint32_t *t_doc, *b_doc;
    const float *t_w, *b_w;
    const uint64_t* b_pos_ptr;                            // NULL: the body table has no positional postings
    const float* b_pos;
    uint64_t t_terms, b_terms, n_docs;
    const uint32_t *q_ptr, *q_terms;                      // the call's table: [n_q + 1] offsets into the tokens
    const ss_hit* hits;                                   // [n_q][k]
    const int32_t* n_hits;                                // [n_q]
    ss_term_match* out;                                   // [n_q][k][t_stride]
    uint32_t n_q, k, t_stride, blocks_per_q;
};

// key of a position for the minimum over values >= 0: the float's bits (ascending with the value for v >= 0), both zeros -> 0;
// EX_NONE for a negative value or a NaN (both compare false against 0)
__device__ __forceinline__ uint32_t pos_key(float v) {
    return v >= 0.0f ? (v == 0.0f ? 0u : __float_as_uint(v)) : EX_NONE;
}

__global__ __launch_bounds__(EX_TPB) void k_explain_hits(ExplainParams p) {
    const uint32_t q = blockIdx.x / p.blocks_per_q;
    const uint32_t e = (blockIdx.x - q * p.blocks_per_q) * EX_TPB + threadIdx.x;   // the entry inside the query: token-major, hit fastest
    const uint32_t n_hits = hw::window_len(p.n_hits[q], p.k);
    const uint32_t q0 = p.q_ptr[q];
    uint32_t n_tok = p.q_ptr[q + 1] - q0;
    n_tok = n_tok > p.t_stride ? p.t_stride : n_tok;      // (the host has refused longer queries; the table is the call's own)
    const bool live = n_hits && e < n_hits * n_tok;       // (n_hits * n_tok <= k * t_stride < 2^31)
    uint32_t i = 0, j = 0;
    ss_term_match m;
    m.title_w = 0.0f;
    m.body_w = 0.0f;
    m.flags = 0u;
    m.body_pos = 0.0f;
    uint64_t pb = 0, pe = 0;                              // the body posting's position list [pb, pe)
    if (live) {
        i = e / n_hits;
        j = e - i * n_hits;
        const uint32_t term = p.q_terms[q0 + i];
        const uint32_t d = p.hits[(size_t)q * p.k + j].doc;
        if ((uint64_t)d < p.n_docs) {
            // [lo, hi) of both searches; an unknown term searches nothing
            uint64_t tlo = 0, thi = 0, blo = 0, bhi = 0;
            if ((uint64_t)term < p.t_terms) { tlo = p.t_ptr[term]; thi = p.t_ptr[term + 1]; }
            if ((uint64_t)term < p.b_terms) { blo = p.b_ptr[term]; bhi = p.b_ptr[term + 1]; }
            const uint64_t tend = thi, bend = bhi;
            // lower bound of d in both lists, one step of each per round: the two loads are independent
            while (tlo < thi || blo < bhi) {
                const bool ts = tlo < thi, bs = blo < bhi;
                const uint64_t tm = tlo + ((thi - tlo) >> 1), bm = blo + ((bhi - blo) >> 1);
                const uint32_t td = ts ? p.t_doc[tm] : 0u;
                const uint32_t bd = bs ? p.b_doc[bm] : 0u;
                if (ts) { if (td < d) tlo = tm + 1; else thi = tm; }
                if (bs) { if (bd < d) blo = bm + 1; else bhi = bm; }
            }
            if (tlo < tend && p.t_doc[tlo] == d) {
                m.title_w = p.t_w[tlo];
                m.flags |= 1u;
            }
            if (blo < bend && p.b_doc[blo] == d) {
                m.body_w = p.b_w[blo];
                m.flags |= 2u;
                if (p.b_pos_ptr) {
                    pb = p.b_pos_ptr[blo];
                    pe = p.b_pos_ptr[blo + 1];
                }
            }
        }
    }
    // ---- the earliest position: short lists by their lane, long ones by the wave (every lane of the wave gets here)
    uint32_t key = EX_NONE;
    const bool long_list = pe - pb > EX_OWN;
    if (!long_list)
        for (uint64_t x = pb; x < pe; x++) key = min(key, pos_key(p.b_pos[x]));
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(long_list);
    while (todo) {
        const int owner = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t ob = __shfl(pb, owner, 64), oe = __shfl(pe, owner, 64);
        uint32_t kk = EX_NONE;
        for (uint64_t x = ob + lane; x < oe; x += 64) kk = min(kk, pos_key(p.b_pos[x]));
        for (int off = 32; off > 0; off >>= 1) kk = min(kk, (uint32_t)__shfl_xor(kk, off, 64));
        if ((int)lane == owner) key = kk;
    }
    if (!live) return;
    if (key != EX_NONE) {
        m.body_pos = __uint_as_float(key);
        m.flags |= 4u;
    }
    static_assert(sizeof(ss_term_match) == 16, "an entry is 16 bytes");
    p.out[((size_t)q * p.k + j) * p.t_stride + i] = m;    // (a caller's array need only be aligned as the struct is: 4 bytes)
}

int32_t explain_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                     const int32_t* n_hits, int32_t t_stride, ss_term_match* out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and `out` is not touched before the last of them has passed
    if (!out || n_q < 0 || !q_ptr) return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: NULL argument or n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: k = %d, must be >= 1", k);
    if (t_stride < 1) return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: t_stride = %d, must be >= 1", t_stride);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_explain_hits: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
    if (t_stride > SS_MAX_QUERY_TERMS)
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_explain_hits: t_stride = %d exceeds SS_MAX_QUERY_TERMS = %d", t_stride, SS_MAX_QUERY_TERMS);
    if ((uint64_t)n_q * (uint64_t)k * (uint64_t)t_stride >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_explain_hits: n_q * k * t_stride = %llu entries, must be below 2^31",
                         (unsigned long long)((uint64_t)n_q * (uint64_t)k * (uint64_t)t_stride));
    if (n_q == 0) return SS_OK;
    if (!hits || !n_hits) return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: hits or n_hits is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, "ss_explain_hits", "q", q_ptr, nq, h_ptr.data()));
    for (size_t q = 0; q < nq; q++)
        if (h_ptr[q + 1] - h_ptr[q] > (uint32_t)t_stride)
            return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: query %zu has %u tokens, t_stride = %d", q, h_ptr[q + 1] - h_ptr[q], t_stride);
    const size_t tok0 = h_ptr[0], n_tok = h_ptr[nq] - tok0;
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "ss_explain_hits: q_terms is NULL");
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_explain_hits", "k", n_q, k, hits, n_hits, &w));
    // ---- the queries' table in the pinned block of the next explain turn, the blocks of host arrays; then the pipeline
    QueryTurn& turn = s->exp[s->exp_turn];
    hw::QueryTable tab;
    SS_TRY(hw::query_table_fill(ctx, turn, h_ptr, q_terms, 1, &tab));
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, out, nq * (size_t)k * (size_t)t_stride * sizeof(ss_term_match), &o));
    SS_TRY(hw::window_stage(s, &w));
    s->exp_turn = (s->exp_turn + 1) % ss_scorer::TURNS;
    SS_HIP(ctx, hw::query_table_upload(ctx, turn, tab));
    ExplainParams p{};
    p.t_ptr = s->title->term_ptr.p; p.t_doc = s->title->post_doc.p; p.t_w = s->title->post_w.p; p.t_terms = s->title->n_terms;
    p.b_ptr = s->body->term_ptr.p; p.b_doc = s->body->post_doc.p; p.b_w = s->body->post_w.p; p.b_terms = s->body->n_terms;
    p.b_pos_ptr = s->body->pos_ptr.p;
    p.b_pos = s->body->pos.p;
    p.n_docs = s->n_docs;
    p.q_ptr = turn.d_q.p;
    p.q_terms = turn.d_q.p + nq + 1;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.out = static_cast<ss_term_match*>(o.dev);
    p.n_q = (uint32_t)n_q; p.k = (uint32_t)k; p.t_stride = (uint32_t)t_stride;
    p.blocks_per_q = ss::div_up((uint64_t)k * (uint64_t)t_stride, EX_TPB);
    hipLaunchKernelGGL(k_explain_hits, dim3(p.n_q * p.blocks_per_q), dim3(EX_TPB), 0, st, p);   // (< 2^31 / 256 * 2 blocks)
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    // every array in device memory: nothing is waited for.  A host `out`: of every row the query's own tokens, the table's ptr
    return hw::entries_out_finish(s, o, w, sizeof(ss_term_match), (size_t)t_stride, tab.h);
}

}  // namespace

extern "C" {

int32_t ss_explain_hits(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                        const int32_t* n_hits, int32_t t_stride, ss_term_match* out) {
    return hw::guarded(s, "ss_explain_hits", [&] { return explain_impl(s, n_q, q_ptr, q_terms, k, hits, n_hits, t_stride, out); });
}

}  // extern "C"
