// collapse.hip — ss_scorer_set_doc_groups, ss_collapse_hits and ss_score_topk_collapsed: at most g rows per group ("site") in a
// result window, with paging.  A step file beside explain.hip and related.hip: one kernel behind whatever scoring call
// made the rows, no scoring kernel edited.
//
//   checks                     arguments, the group table, host n_hits — all before anything is enqueued
//   ss::score_into_turn        (ss_score_topk_collapsed only) the steps of ss_score_topk_masked at k_window; the rows stay in the block
//                              of the plan turn the call took
//   k_collapse_hits            one workgroup per query.  Row j of the window gets the 64-bit key (group key << 10 | j): the table's
//                              value, or — for a row of its own — bit 32 of the group key set beside j, which no table value reaches and
//                              no other row shares.  The keys are sorted in LDS over the next power of two >= the window's length; a
//                              group's rows then lie side by side in window order, so a row's rank inside its group is its sorted
//                              position minus the group's first, found by two binary searches, which also give the group's size
//                              (`same`).  keep = rank < g goes back to window order, a workgroup prefix sum of it numbers the kept rows,
//                              and the rows numbered [first, first + k) are copied out, five lanes to a row (8 bytes each), so that a
//                              wave's stores are one contiguous run.  Only .doc of a row is read to decide anything.
// The window in, the paging checks and the outputs' way back: hit_window.hpp.
#include "hit_window.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

constexpr uint64_t CL_DEAD = ~0ull;                       // the key of a slot behind the window: sorts behind every live key
constexpr uint32_t CL_J_BITS = 10;                        // j < SS_MAX_TOPK = 2^10
constexpr uint32_t CL_KEEP = 0x80000000u;                 // s_ks[j] = same | (kept ? CL_KEEP : 0)
constexpr uint32_t CL_NONE = 0xFFFFFFFFu;                 // s_pos[j] of a row that is not kept
static_assert(SS_MAX_TOPK == (1 << CL_J_BITS), "a window index takes CL_J_BITS bits of a key");

struct CollapseParams {
    const uint32_t* group;                                // [n_docs]
    uint64_t n_docs;
    const ss_hit* hits;                                   // [n_q][k_in]
    const int32_t* n_hits;                                // [n_q]
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;                                  // [n_q]
    uint32_t* same_out;                                   // [n_q][k], nullable
    int32_t* n_kept_out;                                  // [n_q], nullable
    uint32_t k_in, g, first, k;
};

// the first position in s_key[0 .. np) whose key is >= target (np a power of two or 0; the keys ascending)
__device__ __forceinline__ uint32_t lower_key(const uint64_t* s_key, uint32_t np, uint64_t target) {
    uint32_t lo = 0, hi = np;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_key[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup of BLOCK threads per query; windows of up to CAP = PER * BLOCK rows (the launcher picks the instance by k_in).
template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_collapse_hits(CollapseParams p) {
    constexpr uint32_t CAP = PER * BLOCK, WAVES = BLOCK / 64;
    __shared__ uint64_t s_key[CAP];                       // sorted keys; afterwards, as 32-bit words, the window row of every output slot
    __shared__ uint32_t s_ks[CAP];                        // by window index: same | CL_KEEP
    __shared__ uint32_t s_pos[CAP];                       // by window index: the row's number among the kept rows, CL_NONE if not kept
    __shared__ uint32_t s_wsum[WAVES];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t np = hw::pow2_at_least(n);             // (the same value in every thread)
    // ---- the keys
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint64_t key = CL_DEAD;
        if (j < n) {
            const uint32_t d = rows[j].doc;
            uint32_t grp = SS_NO_GROUP;
            if ((uint64_t)d < p.n_docs) grp = p.group[d];
            const uint64_t gk = grp != SS_NO_GROUP ? (uint64_t)grp : (1ull << 32 | j);
            key = gk << CL_J_BITS | j;
        }
        s_key[j] = key;
    }
    __syncthreads();
    // ---- bitonic sort, ascending: a group's rows end up side by side in window order
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t a = s_key[i], b = s_key[o];
        if ((a > b) == up) {
            s_key[i] = b;
            s_key[o] = a;
        }
    });
    // ---- rank inside the group and the group's size, back to window order
    for (uint32_t i = tid; i < n; i += BLOCK) {           // (the n live keys are the first n)
        const uint64_t key = s_key[i];
        const uint64_t gk = key >> CL_J_BITS;
        const uint32_t j = (uint32_t)key & ((1u << CL_J_BITS) - 1u);
        uint32_t rank = 0, same = 1;
        if (!(gk >> 32)) {                                // (a row of its own: alone in its group)
            const uint32_t b = lower_key(s_key, np, gk << CL_J_BITS), e = lower_key(s_key, np, (gk + 1) << CL_J_BITS);
            rank = i - b;
            same = e - b;
        }
        s_ks[j] = same | (rank < p.g ? CL_KEEP : 0u);
    }
    __syncthreads();
    // ---- number the kept rows: thread t owns window rows [t * PER, (t + 1) * PER)
    uint32_t mine = 0;
#pragma unroll
    for (int c = 0; c < PER; c++) {
        const uint32_t j = tid * PER + c;
        if (j < n && (s_ks[j] & CL_KEEP)) mine++;
    }
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();                                      // (also: every thread has read the sorted keys, s_key may be rewritten)
    uint32_t before = incl - mine, n_kept = 0;
#pragma unroll
    for (uint32_t v = 0; v < WAVES; v++) {
        const uint32_t w = s_wsum[v];
        if (v < wave) before += w;
        n_kept += w;
    }
#pragma unroll
    for (int c = 0; c < PER; c++) {
        const uint32_t j = tid * PER + c;
        if (j < n) s_pos[j] = (s_ks[j] & CL_KEEP) ? before++ : CL_NONE;
    }
    const uint32_t n_out = hw::page_len(n_kept, p.first, p.k);                   // <= k, <= n
    __syncthreads();
    // ---- which window row every output slot takes
    uint32_t* const s_src = reinterpret_cast<uint32_t*>(s_key);                  // [n_out], n_out <= n <= CAP
    for (uint32_t j = tid; j < n; j += BLOCK) {
        const uint32_t pos = s_pos[j];
        if (pos != CL_NONE && pos >= p.first && pos - p.first < n_out) s_src[pos - p.first] = j;
    }
    __syncthreads();
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_src[r]; });
    if (p.same_out)
        for (uint32_t r = tid; r < n_out; r += BLOCK) p.same_out[(size_t)q * p.k + r] = s_ks[s_src[r]] & ~CL_KEEP;
    if (tid == 0) {
        p.n_hits_out[q] = (int32_t)n_out;
        if (p.n_kept_out) p.n_kept_out[q] = (int32_t)n_kept;
    }
}

// windows of up to 128 rows: one wave, two rows a lane; longer ones: four waves, up to four rows a lane
constexpr int CL_SMALL = 64, CL_SMALL_PER = 2, CL_LARGE = 256, CL_LARGE_PER = 4;
static_assert(CL_LARGE * CL_LARGE_PER >= SS_MAX_TOPK, "k_collapse_hits holds a whole window in LDS");

struct CollapseArgs {
    int32_t n_q, k_in, g, first, k;
    const ss_hit* hits;                                   // device memory ...
    const int32_t* n_hits;                                // ... both
    ss_hit* hits_out;                                     // host or device, the caller's
    int32_t* n_hits_out;
    uint32_t* same_out;                                   // nullable
    int32_t* n_kept_out;                                  // nullable
};

// The kernel behind rows that are in device memory, and the way back of host outputs.  `last_reader` (nullable) is recorded behind the
// kernel.  Returns without waiting when every output is device memory and `staged` is false.
int32_t collapse_run(ss_scorer* s, const CollapseArgs& a, ss::Event* last_reader, bool staged) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)a.n_q, (size_t)a.k, a.hits_out, a.n_hits_out, a.n_kept_out, a.same_out, sizeof(uint32_t), &o));
    CollapseParams p{};
    p.group = s->groups.p;
    p.n_docs = s->n_docs;
    p.hits = a.hits;
    p.n_hits = a.n_hits;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.same_out = static_cast<uint32_t*>(o.extra);
    p.n_kept_out = o.n_kept;
    p.k_in = (uint32_t)a.k_in; p.g = (uint32_t)a.g; p.first = (uint32_t)a.first; p.k = (uint32_t)a.k;
    if (a.k_in <= CL_SMALL * CL_SMALL_PER)
        hipLaunchKernelGGL((k_collapse_hits<CL_SMALL, CL_SMALL_PER>), dim3((unsigned)a.n_q), dim3(CL_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_collapse_hits<CL_LARGE, CL_LARGE_PER>), dim3((unsigned)a.n_q), dim3(CL_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    if (last_reader) SS_HIP(ctx, last_reader->record(st));
    return hw::rows_out_finish(s, o, staged);
}

int32_t collapse_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t g, int32_t first,
                      int32_t k, ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, "ss_collapse_hits", "k_in", n_q, k_in, k, first, "g", g));
    SS_TRY(hw::check_page_arrays(ctx, "ss_collapse_hits", n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    if (!s->has_groups) return ctx->fail(SS_ERR_STATE, "ss_collapse_hits: no group table registered (ss_scorer_set_doc_groups)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_collapse_hits", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const CollapseArgs a{n_q, k_in, g, first, k, w.hits, w.n_hits, hits_out, n_hits_out, same_out, n_kept_out};
    return collapse_run(s, a, nullptr, w.staged);
}

int32_t score_collapsed_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                             const double* topic_probs, const int32_t* mask_id, int32_t k_window, int32_t g, int32_t first, int32_t k,
                             ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks of this call; the scoring call below makes its own (mask ids, the prior, the queries) before it enqueues anything
    SS_TRY(hw::check_paging(ctx, "ss_score_topk_collapsed", "k_window", n_q, k_window, k, first, "g", g));
    if (!q_ptr || (n_q > 0 && (!hits_out || !n_hits_out)))
        return ctx->fail(SS_ERR_INVALID, "ss_score_topk_collapsed: q_ptr, hits_out or n_hits_out is NULL");
    if (!s->has_groups) return ctx->fail(SS_ERR_STATE, "ss_score_topk_collapsed: no group table registered (ss_scorer_set_doc_groups)");
    if (topic_probs && s->k_topics == 0)
        return ctx->fail(SS_ERR_STATE, "ss_score_topk_collapsed: topic_probs given but no prior set (ss_scorer_set_prior)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    // ---- the scoring call with k_window, rows in the turn's block
    TurnRows tr;
    if (const int32_t rc = ss::score_into_turn(s, n_q, q_ptr, q_terms, topic_probs, mask_id, k_window, &tr, query_len)) {
        const std::string why = ctx->last_error;          // (the shared steps name ss_score_topk; nothing has touched the outputs)
        return ctx->fail(rc, "ss_score_topk_collapsed: scoring the queries at k_window failed: %s", why.c_str());
    }
    if (tr.turn < 0) return ctx->fail(SS_ERR_STATE, "ss_score_topk_collapsed: internal: the scoring call took no turn");
    // k_collapse_hits is the last reader of the turn's rows: the turn's batch_ev is recorded again behind it
    const CollapseArgs a{n_q, k_window, g, first, k, tr.hits, tr.n_hits, hits_out, n_hits_out, same_out, n_kept_out};
    return collapse_run(s, a, &s->turn[tr.turn].batch_ev, false);
}

}  // namespace

extern "C" {

int32_t ss_scorer_set_doc_groups(ss_scorer* s, const uint32_t* group) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    // the scorer's outstanding batches (pipelined calls, tickets) may be followed by a kernel that reads the old table: that kernel is
    // on the context's stream, which is drained — with the wave streams, as ss_scorer_set_doc_masks does — before the table is replaced
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    s->drop_group_ranks();                          // (group_topk.hip: they describe the old table; the next call that needs them builds them)
    if (!group) {
        s->groups.release();
        s->has_groups = false;
        return SS_OK;
    }
    ss::DevBuf<uint32_t> nb;
    SS_HIP(ctx, nb.alloc((size_t)s->n_docs));
    if (s->n_docs) {
        SS_HIP(ctx, hipMemcpyAsync(nb.p, group, (size_t)s->n_docs * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
        SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    s->groups = std::move(nb);
    s->has_groups = true;
    return SS_OK;
}

int32_t ss_collapse_hits(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t g, int32_t first,
                         int32_t k, ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    return hw::guarded(s, "ss_collapse_hits", [&] { return collapse_impl(s, n_q, k_in, hits, n_hits, g, first, k, hits_out, n_hits_out, same_out, n_kept_out); });
}

int32_t ss_score_topk_collapsed(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                                const double* topic_probs, const int32_t* mask_id, int32_t k_window, int32_t g, int32_t first, int32_t k,
                                ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    return hw::guarded(s, "ss_score_topk_collapsed", [&] {
        return score_collapsed_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, mask_id, k_window, g, first, k, hits_out, n_hits_out,
                                    same_out, n_kept_out);
    });
}

}  // extern "C"
