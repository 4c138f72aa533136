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
// Device hits / n_hits / outputs: the call only enqueues on the context's stream.  Otherwise the host arrays go through scorer-owned
// grow-only device blocks and only the entries the definition names are copied back.
#include "scorer.hpp"

#include <algorithm>

namespace {

constexpr uint64_t CL_DEAD = ~0ull;                       // the key of a slot behind the window: sorts behind every live key
constexpr uint32_t CL_J_BITS = 10;                        // j < SS_MAX_TOPK = 2^10
constexpr uint32_t CL_KEEP = 0x80000000u;                 // s_ks[j] = same | (kept ? CL_KEEP : 0)
constexpr uint32_t CL_NONE = 0xFFFFFFFFu;                 // s_pos[j] of a row that is not kept
static_assert(SS_MAX_TOPK == (1 << CL_J_BITS), "a window index takes CL_J_BITS bits of a key");
constexpr uint32_t CL_ROW_WORDS = sizeof(ss_hit) / 8;      // a row as 8-byte words
static_assert(sizeof(ss_hit) == 40 && alignof(ss_hit) == 8, "a row is five 8-byte words");

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
    const int32_t nr = p.n_hits[q];
    const uint32_t n = nr < 0 ? 0u : (uint32_t)nr > p.k_in ? p.k_in : (uint32_t)nr;   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    uint32_t np = 1;
    while (np < n) np <<= 1;                              // (the same value in every thread)
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
    const uint32_t n_out = n_kept > p.first ? (n_kept - p.first < p.k ? n_kept - p.first : p.k) : 0u;   // <= k, <= n
    __syncthreads();
    // ---- which window row every output slot takes
    uint32_t* const s_src = reinterpret_cast<uint32_t*>(s_key);                  // [n_out], n_out <= n <= CAP
    for (uint32_t j = tid; j < n; j += BLOCK) {
        const uint32_t pos = s_pos[j];
        if (pos != CL_NONE && pos >= p.first && pos - p.first < n_out) s_src[pos - p.first] = j;
    }
    __syncthreads();
    // ---- the rows, as 8-byte words: lane x moves word x % 5 of slot x / 5
    const uint64_t* const in_w = reinterpret_cast<const uint64_t*>(rows);
    uint64_t* const out_w = reinterpret_cast<uint64_t*>(p.hits_out + (size_t)q * p.k);
    for (uint32_t x = tid; x < n_out * CL_ROW_WORDS; x += BLOCK) {
        const uint32_t r = x / CL_ROW_WORDS, w = x - r * CL_ROW_WORDS;
        out_w[x] = in_w[(size_t)s_src[r] * CL_ROW_WORDS + w];
    }
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
// kernel.  Returns without waiting when every output is device memory and `wait` is false.
int32_t collapse_run(ss_scorer* s, const CollapseArgs& a, ss::Event* last_reader, bool wait) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)a.n_q, n_rows = nq * (size_t)a.k;
    const bool dev_h = ss::on_device(a.hits_out), dev_n = ss::on_device(a.n_hits_out);
    const bool dev_s = a.same_out && ss::on_device(a.same_out), dev_k = a.n_kept_out && ss::on_device(a.n_kept_out);
    if (!dev_h) SS_HIP(ctx, ensure(s->d_col_out, n_rows));
    if (!dev_n) SS_HIP(ctx, ensure(s->d_col_nout, nq));
    if (a.same_out && !dev_s) SS_HIP(ctx, ensure(s->d_col_same, n_rows));
    if (a.n_kept_out && !dev_k) SS_HIP(ctx, ensure(s->d_col_kept, nq));
    CollapseParams p{};
    p.group = s->groups.p;
    p.n_docs = s->n_docs;
    p.hits = a.hits;
    p.n_hits = a.n_hits;
    p.hits_out = dev_h ? a.hits_out : s->d_col_out.p;
    p.n_hits_out = dev_n ? a.n_hits_out : s->d_col_nout.p;
    p.same_out = !a.same_out ? nullptr : dev_s ? a.same_out : s->d_col_same.p;
    p.n_kept_out = !a.n_kept_out ? nullptr : dev_k ? a.n_kept_out : s->d_col_kept.p;
    p.k_in = (uint32_t)a.k_in; p.g = (uint32_t)a.g; p.first = (uint32_t)a.first; p.k = (uint32_t)a.k;
    if (a.k_in <= CL_SMALL * CL_SMALL_PER)
        hipLaunchKernelGGL((k_collapse_hits<CL_SMALL, CL_SMALL_PER>), dim3((unsigned)a.n_q), dim3(CL_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_collapse_hits<CL_LARGE, CL_LARGE_PER>), dim3((unsigned)a.n_q), dim3(CL_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    if (last_reader) SS_HIP(ctx, last_reader->record(st));
    const bool all_dev = dev_h && dev_n && (!a.same_out || dev_s) && (!a.n_kept_out || dev_k);
    if (all_dev) {
        if (wait) SS_HIP(ctx, hipStreamSynchronize(st));
        return SS_OK;                                     // ordered on the ctx stream; nothing comes back
    }
    // ---- host outputs: the counts whole, of the rows exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq), h_kept;
    std::vector<ss_hit> h_rows;
    std::vector<uint32_t> h_same;
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), p.n_hits_out, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (a.n_kept_out && !dev_k) {
        h_kept.resize(nq);
        SS_HIP(ctx, hipMemcpyAsync(h_kept.data(), p.n_kept_out, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (!dev_h) {
        h_rows.resize(n_rows);
        SS_HIP(ctx, hipMemcpyAsync(h_rows.data(), p.hits_out, n_rows * sizeof(ss_hit), hipMemcpyDeviceToHost, st));
    }
    if (a.same_out && !dev_s) {
        h_same.resize(n_rows);
        SS_HIP(ctx, hipMemcpyAsync(h_same.data(), p.same_out, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(a.n_hits_out, h_n.data(), nq * sizeof(int32_t));
    if (a.n_kept_out && !dev_k) std::memcpy(a.n_kept_out, h_kept.data(), nq * sizeof(int32_t));
    for (size_t q = 0; q < nq; q++) {
        const size_t cnt = (size_t)h_n[q], o = q * (size_t)a.k;
        if (!dev_h) std::memcpy(a.hits_out + o, h_rows.data() + o, cnt * sizeof(ss_hit));
        if (a.same_out && !dev_s) std::memcpy(a.same_out + o, h_same.data() + o, cnt * sizeof(uint32_t));
    }
    return SS_OK;
}

// the checks the two entry points share (k_in: the window's width); SS_OK = go on
int32_t check_paging(ss_ctx* ctx, const char* entry, const char* window, int32_t n_q, int32_t k_in, int32_t g, int32_t first, int32_t k) {
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_q < 0", entry);
    if (k_in < 1 || k < 1 || g < 1 || first < 0)
        return ctx->fail(SS_ERR_INVALID, "%s: %s = %d, k = %d, g = %d must be >= 1 and first = %d >= 0", entry, window, k_in, k, g, first);
    if (k_in > SS_MAX_TOPK || k > SS_MAX_TOPK)
        return ctx->fail(SS_ERR_UNSUPPORTED, "%s: %s = %d or k = %d exceeds SS_MAX_TOPK = %d", entry, window, k_in, k, SS_MAX_TOPK);
    return SS_OK;
}

int32_t collapse_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t g, int32_t first,
                      int32_t k, ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(check_paging(ctx, "ss_collapse_hits", "k_in", n_q, k_in, g, first, k));
    if (n_q > 0 && (!hits || !n_hits || !hits_out || !n_hits_out))
        return ctx->fail(SS_ERR_INVALID, "ss_collapse_hits: hits, n_hits, hits_out or n_hits_out is NULL");
    const size_t nq = (size_t)n_q, n_rows_in = nq * (size_t)k_in;
    if (n_q > 0) {
        const uintptr_t ib = (uintptr_t)hits, ie = ib + n_rows_in * sizeof(ss_hit);
        const uintptr_t ob = (uintptr_t)hits_out, oe = ob + nq * (size_t)k * sizeof(ss_hit);
        if (ib < oe && ob < ie) return ctx->fail(SS_ERR_INVALID, "ss_collapse_hits: hits_out overlaps hits");
    }
    if (!s->has_groups) return ctx->fail(SS_ERR_STATE, "ss_collapse_hits: no group table registered (ss_scorer_set_doc_groups)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool dev_h = ss::on_device(hits), dev_n = ss::on_device(n_hits);
    std::vector<int32_t> h_n;
    if (!dev_n) {
        h_n.assign(n_hits, n_hits + nq);
        for (size_t q = 0; q < nq; q++)
            if (h_n[q] < 0 || h_n[q] > k_in)
                return ctx->fail(SS_ERR_INVALID, "ss_collapse_hits: n_hits[%zu] = %d outside 0 .. k_in = %d", q, h_n[q], k_in);
    }
    // (host rows and counts: the caller's array and h_n outlive their copies, a call with any host array waits before it returns)
    if (!dev_h) {
        SS_HIP(ctx, ensure(s->d_col_hits, n_rows_in));
        SS_HIP(ctx, hipMemcpyAsync(s->d_col_hits.p, hits, n_rows_in * sizeof(ss_hit), hipMemcpyHostToDevice, st));
    }
    if (!dev_n) {
        SS_HIP(ctx, ensure(s->d_col_n, nq));
        SS_HIP(ctx, hipMemcpyAsync(s->d_col_n.p, h_n.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    const CollapseArgs a{n_q, k_in, g, first, k, dev_h ? hits : s->d_col_hits.p, dev_n ? n_hits : s->d_col_n.p,
                         hits_out, n_hits_out, same_out, n_kept_out};
    return collapse_run(s, a, nullptr, !dev_h || !dev_n);
}

int32_t score_collapsed_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                             const double* topic_probs, const int32_t* mask_id, int32_t k_window, int32_t g, int32_t first, int32_t k,
                             ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks of this call; the scoring call below makes its own (mask ids, the prior, the queries) before it enqueues anything
    SS_TRY(check_paging(ctx, "ss_score_topk_collapsed", "k_window", n_q, k_window, g, first, k));
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
    if (!s) return SS_ERR_INVALID;
    try {
        return collapse_impl(s, n_q, k_in, hits, n_hits, g, first, k, hits_out, n_hits_out, same_out, n_kept_out);
    } catch (const std::bad_alloc&) {
        return s->ctx->fail(SS_ERR_OOM, "ss_collapse_hits: host allocation failed");
    }
}

int32_t ss_score_topk_collapsed(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                                const double* topic_probs, const int32_t* mask_id, int32_t k_window, int32_t g, int32_t first, int32_t k,
                                ss_hit* hits_out, int32_t* n_hits_out, uint32_t* same_out, int32_t* n_kept_out) {
    if (!s) return SS_ERR_INVALID;
    try {
        return score_collapsed_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, mask_id, k_window, g, first, k, hits_out, n_hits_out,
                                    same_out, n_kept_out);
    } catch (const std::bad_alloc&) {
        return s->ctx->fail(SS_ERR_OOM, "ss_score_topk_collapsed: host allocation failed");
    }
}

}  // extern "C"
