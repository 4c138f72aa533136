// hit_window.hpp — the HIP side of the calls that take a window of result rows (hits [n_q][k_in], n_hits [n_q], each in host or device
// memory) and post-process it; hit_window_plan.hpp holds the pure host part.  explain.hip, passage.hip, collapse.hip, dedup.hip,
// field.hip, vector.hip and diversify.hip include this file.
//
//   host    window_check / window_stage    the window in: the host counts snapshotted and checked, then rows and snapshot uploaded
//           rows_out_prepare / _finish     a paged call's outputs: hits_out, n_hits_out, optional n_kept_out and one per-row extra
//           entries_out_prepare / _finish  the one output of a call whose output is indexed by the input window
//           query_table_fill / _upload     the queries' table of ss_explain_hits / ss_best_passages through a QueryTurn
//           guarded                        std::bad_alloc of an entry point's body -> SS_ERR_OOM
//   device  window_len, pow2_at_least, page_len, bitonic_sort, copy_page — the pieces the window kernels share
//
// Host arrays go through the scorer's HitWindowBlocks (scorer.hpp states their invariant): every function here that hands out or
// fills one of the blocks is paired with a finish that waits for the context's stream, or sets WindowIn::staged, which makes the
// call's finish wait.  With every array in device memory a call only enqueues on the context's stream.
#pragma once
#include "hit_window_plan.hpp"
#include "scorer.hpp"

#include <new>

namespace ss {
namespace hitwin {

// ---------------------------------------------------------------- host side
// The body of an entry point whose host containers may throw.
template <typename F>
inline int32_t guarded(ss_ctx* ctx, const char* entry, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "%s: host allocation failed", entry);
    }
}
template <typename F>
inline int32_t guarded(ss_scorer* s, const char* entry, F&& body) {
    return s ? guarded(s->ctx, entry, static_cast<F&&>(body)) : SS_ERR_INVALID;
}

// hit_window_plan.hpp's paging check with the ABI's codes and the context's error text
inline int32_t check_paging(ss_ctx* ctx, const char* entry, const char* window, int32_t n_q, int32_t k_in, int32_t k, int32_t first,
                            const char* extra = nullptr, int32_t extra_v = 1) {
    char msg[256];
    const int32_t rc = check_paging(msg, sizeof(msg), entry, window, SS_MAX_TOPK, n_q, k_in, k, first, extra, extra_v);
    return rc == OK ? SS_OK : ctx->fail(rc == INVALID ? SS_ERR_INVALID : SS_ERR_UNSUPPORTED, "%s", msg);
}
// ... and what follows it in every paged call that is given its rows: the four arrays, and hits_out apart from hits
inline int32_t check_page_arrays(ss_ctx* ctx, const char* entry, int32_t n_q, int32_t k_in, int32_t k, const ss_hit* hits, const int32_t* n_hits,
                                 const ss_hit* hits_out, const int32_t* n_hits_out) {
    if (n_q == 0) return SS_OK;
    if (!hits || !n_hits || !hits_out || !n_hits_out) return ctx->fail(SS_ERR_INVALID, "%s: hits, n_hits, hits_out or n_hits_out is NULL", entry);
    if (overlaps(hits, (size_t)n_q * (size_t)k_in * sizeof(ss_hit), hits_out, (size_t)n_q * (size_t)k * sizeof(ss_hit)))
        return ctx->fail(SS_ERR_INVALID, "%s: hits_out overlaps hits", entry);
    return SS_OK;
}

// The window of a call.  After window_stage: hits and n_hits are device memory.
struct WindowIn {
    const ss_hit* hits = nullptr;
    const int32_t* n_hits = nullptr;
    size_t n_q = 0, k_in = 0;
    bool dev_h = false, dev_n = false;
    bool staged = false;                                  // an input came from host memory: the call waits before it returns
    std::vector<int32_t> h_n;                             // host counts: the snapshot that was checked and is uploaded
};

// Step 1, which enqueues nothing: where the arrays are, and host counts copied once and refused outside 0 .. k_in (`window`: the
// width argument's name).  What the caller does to its n_hits afterwards does not reach the device.
inline int32_t window_check(ss_ctx* ctx, const char* entry, const char* window, int32_t n_q, int32_t k_in, const ss_hit* hits,
                            const int32_t* n_hits, WindowIn* w) {
    w->hits = hits;
    w->n_hits = n_hits;
    w->n_q = (size_t)n_q;
    w->k_in = (size_t)k_in;
    w->dev_h = ss::on_device(hits);
    w->dev_n = ss::on_device(n_hits);
    if (w->dev_n) return SS_OK;
    w->h_n.assign(n_hits, n_hits + w->n_q);
    const size_t bad = first_bad_count(w->h_n.data(), w->n_q, k_in);
    if (bad != NONE) return ctx->fail(SS_ERR_INVALID, "%s: n_hits[%zu] = %d outside 0 .. %s = %d", entry, bad, w->h_n[bad], window, k_in);
    return SS_OK;
}
// Step 2: host arrays into the shared blocks.  (The caller's rows and the snapshot outlive their copies: a staged call waits.)
inline int32_t window_stage(ss_scorer* s, WindowIn* w) {
    ss_ctx* ctx = s->ctx;
    const size_t n_rows = w->n_q * w->k_in;
    if (!w->dev_h) SS_HIP(ctx, ensure(s->win.rows_in, n_rows));
    if (!w->dev_n) SS_HIP(ctx, ensure(s->win.n_in, w->n_q));
    if (!w->dev_h) {
        SS_HIP(ctx, hipMemcpyAsync(s->win.rows_in.p, w->hits, n_rows * sizeof(ss_hit), hipMemcpyHostToDevice, ctx->stream));
        w->hits = s->win.rows_in.p;
    }
    if (!w->dev_n) {
        SS_HIP(ctx, hipMemcpyAsync(s->win.n_in.p, w->h_n.data(), w->n_q * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        w->n_hits = s->win.n_in.p;
    }
    w->staged = !w->dev_h || !w->dev_n;
    return SS_OK;
}

// The outputs of a paged call: where the kernel writes (the caller's array when it is device memory, else a shared block) and the
// caller's own.  n_kept and the extra (one element of extra_elem bytes per output row) are NULL when the caller gave none.
struct RowsOut {
    ss_hit* hits = nullptr;
    int32_t* n_hits = nullptr;
    int32_t* n_kept = nullptr;
    void* extra = nullptr;
    size_t n_q = 0, k = 0, extra_elem = 0;
    ss_hit* c_hits = nullptr;                             // the caller's; NULL: nothing to bring back
    int32_t *c_n = nullptr, *c_kept = nullptr;
    void* c_extra = nullptr;
};
inline int32_t rows_out_prepare(ss_scorer* s, size_t n_q, size_t k, ss_hit* hits_out, int32_t* n_hits_out, int32_t* n_kept_out, void* extra_out,
                                size_t extra_elem, RowsOut* o) {
    ss_ctx* ctx = s->ctx;
    const size_t n_rows = n_q * k;
    o->n_q = n_q; o->k = k; o->extra_elem = extra_elem;
    o->hits = hits_out; o->n_hits = n_hits_out; o->n_kept = n_kept_out; o->extra = extra_out;
    if (!ss::on_device(hits_out)) {
        SS_HIP(ctx, ensure(s->win.rows_out, n_rows));
        o->c_hits = hits_out;
        o->hits = s->win.rows_out.p;
    }
    if (!ss::on_device(n_hits_out)) {
        SS_HIP(ctx, ensure(s->win.n_out, n_q));
        o->c_n = n_hits_out;
        o->n_hits = s->win.n_out.p;
    }
    if (n_kept_out && !ss::on_device(n_kept_out)) {
        SS_HIP(ctx, ensure(s->win.kept_out, n_q));
        o->c_kept = n_kept_out;
        o->n_kept = s->win.kept_out.p;
    }
    if (extra_out && !ss::on_device(extra_out)) {
        SS_HIP(ctx, ensure(s->win.extra, n_rows * extra_elem));
        o->c_extra = extra_out;
        o->extra = s->win.extra.p;
    }
    return SS_OK;
}
// Behind the launch.  Every output in device memory: returns at once, or waits if an input was staged.  Otherwise the call waits and the
// host arrays get the counts whole and, of the rows and the extra, exactly the entries the kernel wrote.
inline int32_t rows_out_finish(ss_scorer* s, const RowsOut& o, bool staged) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (!o.c_hits && !o.c_n && !o.c_kept && !o.c_extra) {
        if (staged) SS_HIP(ctx, hipStreamSynchronize(st));
        return SS_OK;                                     // ordered on the ctx stream; nothing comes back
    }
    const size_t n_rows = o.n_q * o.k;
    std::vector<int32_t> h_n(o.n_q), h_kept(o.c_kept ? o.n_q : 0);
    std::vector<unsigned char> h_rows(o.c_hits ? n_rows * sizeof(ss_hit) : 0), h_extra(o.c_extra ? n_rows * o.extra_elem : 0);
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), o.n_hits, o.n_q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (o.c_kept) SS_HIP(ctx, hipMemcpyAsync(h_kept.data(), o.n_kept, o.n_q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (o.c_hits) SS_HIP(ctx, hipMemcpyAsync(h_rows.data(), o.hits, h_rows.size(), hipMemcpyDeviceToHost, st));
    if (o.c_extra) SS_HIP(ctx, hipMemcpyAsync(h_extra.data(), o.extra, h_extra.size(), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (o.c_n) std::memcpy(o.c_n, h_n.data(), o.n_q * sizeof(int32_t));
    if (o.c_kept) std::memcpy(o.c_kept, h_kept.data(), o.n_q * sizeof(int32_t));
    if (o.c_hits) copy_written(o.c_hits, h_rows.data(), o.n_q, o.k, sizeof(ss_hit), h_n.data());
    if (o.c_extra) copy_written(o.c_extra, h_extra.data(), o.n_q, o.k, o.extra_elem, h_n.data());
    return SS_OK;
}

// The output of a call that writes one array indexed by its input window, [n_q][k_in][inner_stride] elements: `dev` is where the
// kernel writes.
struct EntriesOut {
    void* dev = nullptr;
    void* caller = nullptr;                               // NULL: the caller's array is device memory
    size_t bytes = 0;
};
inline int32_t entries_out_prepare(ss_scorer* s, void* out, size_t bytes, EntriesOut* o) {
    o->dev = out;
    o->bytes = bytes;
    if (ss::on_device(out)) return SS_OK;
    SS_HIP(s->ctx, ensure(s->win.extra, bytes));
    o->caller = out;
    o->dev = s->win.extra.p;
    return SS_OK;
}
// Behind the launch, as rows_out_finish: a host array gets exactly the entries written for the window's counts (those of the snapshot,
// or — device counts — brought back with the array and clamped as the kernels clamp them) and, of each entry, the first
// inner_ptr[q + 1] - inner_ptr[q] elements (inner_ptr NULL: all inner_stride).
inline int32_t entries_out_finish(ss_scorer* s, const EntriesOut& o, const WindowIn& w, size_t elem, size_t inner_stride = 1,
                                  const uint32_t* inner_ptr = nullptr) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (!o.caller) {
        if (w.staged) SS_HIP(ctx, hipStreamSynchronize(st));
        return SS_OK;
    }
    std::vector<unsigned char> h_out(o.bytes);
    std::vector<int32_t> h_n(w.dev_n ? w.n_q : 0);
    if (w.dev_n) SS_HIP(ctx, hipMemcpyAsync(h_n.data(), w.n_hits, w.n_q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipMemcpyAsync(h_out.data(), o.dev, o.bytes, hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    copy_written(o.caller, h_out.data(), w.n_q, w.k_in, elem, w.dev_n ? h_n.data() : w.h_n.data(), inner_stride, inner_ptr);
    return SS_OK;
}

// One output array of a call whose results came back to the host in one block (`src`: the array's place in it), to the caller's `dst` in
// host or device memory: copy_written's entries — rows [n_q][stride] of `elem` bytes, of row q the first n_written[q] — or, n_written
// NULL, all n_q x stride of them.  An array in device memory gets the same entries by copies that wait.
inline hipError_t give_rows(void* dst, const unsigned char* src, size_t n_q, size_t stride, size_t elem, const int32_t* n_written) {
    if (!ss::on_device(dst)) {
        if (n_written) copy_written(dst, src, n_q, stride, elem, n_written);
        else std::memcpy(dst, src, n_q * stride * elem);
        return hipSuccess;
    }
    if (!n_written) return hipMemcpy(dst, src, n_q * stride * elem, hipMemcpyHostToDevice);
    for (size_t q = 0; q < n_q; q++) {
        const size_t o = q * stride * elem;
        if (n_written[q] > 0)
            if (const hipError_t e = hipMemcpy(static_cast<unsigned char*>(dst) + o, src + o, (size_t)n_written[q] * elem, hipMemcpyHostToDevice)) return e;
    }
    return hipSuccess;
}

// The queries' table of a call in the pinned block of `turn`: ptr [n_q + 1] rebased to 0 | the tokens | words_per_token - 1 more
// words per token, left for the caller to fill before the upload.  Waits for the turn's last reader; enqueues nothing.
struct QueryTable {
    uint32_t* h = nullptr;                                // the pinned block: h[0 .. n_q] ptr, h + n_q + 1 the tokens
    size_t n_q = 0, n_tok = 0, words = 0;
};
inline int32_t query_table_fill(ss_ctx* ctx, QueryTurn& turn, const std::vector<uint32_t>& h_ptr, const uint32_t* q_terms, size_t words_per_token,
                                QueryTable* t) {
    SS_HIP(ctx, turn.ev.wait());                          // the call TURNS calls ago has read this turn's blocks
    const size_t nq = h_ptr.size() - 1, tok0 = h_ptr[0];
    t->n_q = nq;
    t->n_tok = h_ptr[nq] - tok0;
    t->words = nq + 1 + words_per_token * t->n_tok;
    SS_HIP(ctx, turn.h_q.ensure(t->words * sizeof(uint32_t)));
    t->h = turn.h_q.as<uint32_t>();
    for (size_t q = 0; q <= nq; q++) t->h[q] = h_ptr[q] - (uint32_t)tok0;
    SS_HIP(ctx, ss::copy_in(ctx->stream, t->h + nq + 1, q_terms ? q_terms + tok0 : nullptr, t->n_tok * sizeof(uint32_t)));
    SS_HIP(ctx, ensure(turn.d_q, t->words));
    return SS_OK;
}
// the table to the turn's device block; the caller records turn.ev behind the kernel that reads it
inline hipError_t query_table_upload(ss_ctx* ctx, QueryTurn& turn, const QueryTable& t) {
    return hipMemcpyAsync(turn.d_q.p, t.h, t.words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
}

// ---------------------------------------------------------------- device side
constexpr uint32_t ROW_WORDS = sizeof(ss_hit) / 8;        // a result row as 8-byte words
static_assert(sizeof(ss_hit) == 40 && alignof(ss_hit) == 8, "a row is five 8-byte words");

// the rows of a window that count: n_hits[q] clamped to 0 .. k_in
__device__ __forceinline__ uint32_t window_len(int32_t nr, uint32_t k_in) {
    return nr < 0 ? 0u : (uint32_t)nr > k_in ? k_in : (uint32_t)nr;
}
// the smallest power of two >= n (1 for n = 0)
__device__ __forceinline__ uint32_t pow2_at_least(uint32_t n) {
    uint32_t np = 1;
    while (np < n) np <<= 1;
    return np;
}
// the rows of the page [first, first + k) of n_avail rows
__device__ __forceinline__ uint32_t page_len(uint32_t n_avail, uint32_t first, uint32_t k) {
    return n_avail > first ? (n_avail - first < k ? n_avail - first : k) : 0u;
}
// The bitonic network over np slots (a power of two) by the BLOCK threads of a workgroup.  cas(i, o, up): slots i < o; exchange them if
// (slot i sorts behind slot o) == up.  Ends behind a barrier.
template <int BLOCK, typename Cas>
__device__ __forceinline__ void bitonic_sort(uint32_t np, Cas cas) {
    for (uint32_t k2 = 2; k2 <= np; k2 <<= 1) {
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = threadIdx.x; i < np; i += BLOCK) {
                const uint32_t o = i ^ j2;
                if (o > i) cas(i, o, (i & k2) == 0);
            }
            __syncthreads();
        }
    }
}
// The page's rows as 8-byte words: lane x moves word x % 5 of output slot x / 5, so that a wave's stores are one contiguous run.
// src(r): the window row that output slot r takes.
template <int BLOCK, typename Src>
__device__ __forceinline__ void copy_page(const ss_hit* rows, ss_hit* out, uint32_t n_out, Src src) {
    const uint64_t* const in_w = reinterpret_cast<const uint64_t*>(rows);
    uint64_t* const out_w = reinterpret_cast<uint64_t*>(out);
    for (uint32_t x = threadIdx.x; x < n_out * ROW_WORDS; x += BLOCK) {
        const uint32_t r = x / ROW_WORDS, w = x - r * ROW_WORDS;
        out_w[x] = in_w[(size_t)src(r) * ROW_WORDS + w];
    }
}

}  // namespace hitwin
}  // namespace ss
