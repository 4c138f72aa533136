// index.hip — the inverted-index object (index.hpp): upload and validation, destroy, read-out, and what a caller may set on it
// (whole-corpus document frequencies, positional postings, given magnitudes).  The TF-IDF build over it is tfidf.hip, the incremental
// update index_update.hip, the doc-major view doc_view.hip.
#include "index.hpp"
#include <algorithm>
#include <memory>
#include <new>

namespace {

constexpr int TPB = 256;

// validate: term_ptr non-decreasing, doc ids in range, count adjacent non-ascending pairs
__global__ void k_check_ptr(const uint64_t* __restrict__ term_ptr, uint64_t n_terms, const uint32_t* __restrict__ post_doc,
                            unsigned long long* __restrict__ n_boundary_desc, uint32_t* __restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    const uint64_t a = term_ptr[t], b = term_ptr[t + 1];
    if (b < a) { atomicOr(err, 1u); return; }
    // a legitimate descent can only sit at the start of a non-empty list
    if (b > a && a > 0 && post_doc[a] <= post_doc[a - 1]) atomicAdd(n_boundary_desc, 1ull);
}
__global__ void k_check_df(const uint64_t* __restrict__ term_ptr, const uint64_t* __restrict__ df, uint64_t n_terms,
                           uint32_t* __restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    if (df[t] < term_ptr[t + 1] - term_ptr[t]) atomicOr(err, 1u);
}
// positional postings: pos_ptr must be non-decreasing (k_phrase_match reads pos[pos_ptr[i] .. pos_ptr[i+1]))
__global__ void k_check_pos(const uint64_t* __restrict__ pos_ptr, uint64_t n_post, uint32_t* __restrict__ err) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (; i < n_post; i += stride) bad = bad || pos_ptr[i + 1] < pos_ptr[i];
    if (bad) atomicOr(err, 1u);
}
__global__ void k_check_docs(const uint32_t* __restrict__ post_doc, uint64_t n_post, uint64_t n_docs,
                             unsigned long long* __restrict__ n_desc, uint32_t* __restrict__ err) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long local = 0;
    bool bad = false;
    for (; i < n_post; i += stride) {
        const uint32_t d = post_doc[i];
        if (d >= n_docs) bad = true;
        if (i > 0 && d <= post_doc[i - 1]) local++;
    }
    if (bad) atomicOr(err, 2u);
    // wave-reduce then one atomic per wave
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(n_desc, local);
}

}  // namespace

extern "C" {

int32_t ss_index_create(ss_ctx* ctx, uint64_t n_docs, uint64_t n_terms, const uint64_t* term_ptr,
                        const uint32_t* post_doc, const float* post_tf, ss_index** out) {
    if (!ctx) return SS_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out) return ctx->fail(SS_ERR_INVALID, "ss_index_create: out is NULL");
    *out = nullptr;
    if (!term_ptr) return ctx->fail(SS_ERR_INVALID, "ss_index_create: term_ptr is NULL");
    if (n_docs == 0 || n_docs >= 0xFFFFFFF0ull || n_terms >= 0xFFFFFFF0ull)
        return ctx->fail(SS_ERR_INVALID, "ss_index_create: n_docs/n_terms out of range");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    std::unique_ptr<ss_index> idx(new (std::nothrow) ss_index());
    if (!idx) return ctx->fail(SS_ERR_OOM, "ss_index_create: host OOM");
    idx->ctx = ctx;
    idx->n_docs = n_docs;
    idx->n_terms = n_terms;
    idx->h_term_ptr.resize(n_terms + 1);
    SS_HIP(ctx, idx->term_ptr.alloc(n_terms + 1));
    SS_HIP(ctx, hipMemcpyAsync(idx->term_ptr.p, term_ptr, (n_terms + 1) * sizeof(uint64_t), hipMemcpyDefault, st));
    SS_HIP(ctx, hipMemcpyAsync(idx->h_term_ptr.data(), idx->term_ptr.p, (n_terms + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (idx->h_term_ptr[0] != 0) return ctx->fail(SS_ERR_INVALID, "ss_index_create: term_ptr[0] != 0");
    const uint64_t P = idx->h_term_ptr[n_terms];
    idx->n_post = P;
    if (P && (!post_doc || !post_tf)) return ctx->fail(SS_ERR_INVALID, "ss_index_create: NULL postings");
    SS_HIP(ctx, idx->post_doc.alloc(P));
    SS_HIP(ctx, idx->post_w.alloc(P));
    SS_HIP(ctx, idx->mag.alloc(n_docs));
    SS_HIP(ctx, idx->mag2.alloc(n_docs));
    if (P) {
        SS_HIP(ctx, hipMemcpyAsync(idx->post_doc.p, post_doc, P * sizeof(uint32_t), hipMemcpyDefault, st));
        SS_HIP(ctx, hipMemcpyAsync(idx->post_w.p, post_tf, P * sizeof(float), hipMemcpyDefault, st));
    }
    SS_HIP(ctx, hipMemsetAsync(idx->mag.p, 0, n_docs * sizeof(double), st));

    // validation (the scorer relies on strictly ascending doc ids inside a term)
    ss::DevBuf<unsigned long long> d_cnt;
    ss::DevBuf<uint32_t> d_err;
    SS_HIP(ctx, d_cnt.alloc(2));
    SS_HIP(ctx, d_err.alloc(1));
    SS_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), st));
    SS_HIP(ctx, hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), st));
    if (n_terms) hipLaunchKernelGGL(k_check_ptr, dim3(ss::div_up(n_terms, TPB)), dim3(TPB), 0, st, idx->term_ptr.p, n_terms,
                                    idx->post_doc.p, d_cnt.p, d_err.p);
    if (P) hipLaunchKernelGGL(k_check_docs, dim3(std::min<unsigned>(ss::div_up(P, TPB), 16384u)), dim3(TPB), 0, st,
                              idx->post_doc.p, P, n_docs, d_cnt.p + 1, d_err.p);
    unsigned long long h_cnt[2] = {0, 0};
    uint32_t h_err = 0;
    SS_HIP(ctx, ss::fetch(ctx, st, h_cnt, d_cnt.p, sizeof(h_cnt), &h_err, d_err.p, sizeof(h_err)));
    SS_HIP(ctx, hipGetLastError());
    if (h_err & 1) return ctx->fail(SS_ERR_INVALID, "ss_index_create: term_ptr is not non-decreasing");
    if (h_err & 2) return ctx->fail(SS_ERR_INVALID, "ss_index_create: posting holds a doc id >= n_docs");
    if (h_cnt[1] != h_cnt[0])
        return ctx->fail(SS_ERR_UNSORTED, "ss_index_create: %llu posting(s) not strictly ascending by doc id inside a term",
                         h_cnt[1] - h_cnt[0]);
    *out = idx.release();
    return SS_OK;
}

int32_t ss_index_destroy(ss_index* idx) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (idx->users > 0) return ctx->fail(SS_ERR_STATE, "ss_index_destroy: index still used by %d scorer(s)", idx->users);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete idx;
    return SS_OK;
}

int32_t ss_index_get_info(const ss_index* idx, uint64_t* n_docs, uint64_t* n_terms, uint64_t* n_post) {
    if (!idx) return SS_ERR_INVALID;
    if (n_docs) *n_docs = idx->n_docs;
    if (n_terms) *n_terms = idx->n_terms;
    if (n_post) *n_post = idx->n_post;
    return SS_OK;
}

int32_t ss_index_read(ss_index* idx, uint64_t* term_ptr_out, uint32_t* post_doc_out, float* post_w_out) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (term_ptr_out) SS_HIP(ctx, hipMemcpyAsync(term_ptr_out, idx->term_ptr.p, (idx->n_terms + 1) * sizeof(uint64_t), hipMemcpyDefault, st));
    if (post_doc_out && idx->n_post) SS_HIP(ctx, hipMemcpyAsync(post_doc_out, idx->post_doc.p, idx->n_post * sizeof(uint32_t), hipMemcpyDefault, st));
    if (post_w_out && idx->n_post) SS_HIP(ctx, hipMemcpyAsync(post_w_out, idx->post_w.p, idx->n_post * sizeof(float), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

int32_t ss_index_read_positions(ss_index* idx, uint64_t* pos_ptr_out, float* pos_out) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->pos_ptr.p) return ctx->fail(SS_ERR_STATE, "ss_index_read_positions: the table holds no positional postings");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (pos_ptr_out) SS_HIP(ctx, hipMemcpyAsync(pos_ptr_out, idx->pos_ptr.p, (idx->n_post + 1) * sizeof(uint64_t), hipMemcpyDefault, st));
    if (pos_out && idx->pos.n) SS_HIP(ctx, hipMemcpyAsync(pos_out, idx->pos.p, idx->pos.n * sizeof(float), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

int32_t ss_index_set_doc_freq(ss_index* idx, const uint64_t* df) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (idx->weighted) return ctx->fail(SS_ERR_STATE, "ss_index_set_doc_freq: table is already weighted");
    if (!df) { idx->has_df_global = false; idx->df_global.release(); return SS_OK; }
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t T = idx->n_terms;
    SS_HIP(ctx, idx->df_global.alloc(T));
    ss::DevBuf<uint32_t> err;
    SS_HIP(ctx, err.alloc(1));
    SS_HIP(ctx, hipMemsetAsync(err.p, 0, sizeof(uint32_t), st));
    if (T) {
        SS_HIP(ctx, hipMemcpyAsync(idx->df_global.p, df, T * sizeof(uint64_t), hipMemcpyDefault, st));
        hipLaunchKernelGGL(k_check_df, dim3(ss::div_up(T, TPB)), dim3(TPB), 0, st, idx->term_ptr.p, idx->df_global.p, T, err.p);
    }
    uint32_t h_err = 0;
    SS_HIP(ctx, ss::fetch(ctx, st, &h_err, err.p, sizeof(uint32_t)));
    if (h_err) {
        idx->df_global.release();
        idx->has_df_global = false;
        return ctx->fail(SS_ERR_INVALID, "ss_index_set_doc_freq: a document frequency is smaller than the local list");
    }
    idx->has_df_global = true;
    return SS_OK;
}

int32_t ss_index_set_positions(ss_index* idx, const uint64_t* pos_ptr, const float* pos) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!pos_ptr) return ctx->fail(SS_ERR_INVALID, "ss_index_set_positions: pos_ptr is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t P = idx->n_post;
    SS_HIP(ctx, idx->pos_ptr.alloc(P + 1));
    SS_HIP(ctx, hipMemcpyAsync(idx->pos_ptr.p, pos_ptr, (P + 1) * sizeof(uint64_t), hipMemcpyDefault, st));
    uint64_t ends[2] = {0, 0};
    SS_HIP(ctx, ss::fetch(ctx, st, &ends[0], idx->pos_ptr.p, sizeof(uint64_t), &ends[1], idx->pos_ptr.p + P, sizeof(uint64_t)));
    if (ends[0] != 0) { idx->pos_ptr.release(); return ctx->fail(SS_ERR_INVALID, "ss_index_set_positions: pos_ptr[0] != 0"); }
    if (P) {
        // monotone + first 0 + last = total  =>  every range lies inside pos[0, total)
        ss::DevBuf<uint32_t> err;
        SS_HIP(ctx, err.alloc(1));
        SS_HIP(ctx, hipMemsetAsync(err.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_check_pos, dim3(std::min<unsigned>(ss::div_up(P, TPB), 16384u)), dim3(TPB), 0, st, idx->pos_ptr.p, P, err.p);
        uint32_t h_err = 0;
        SS_HIP(ctx, ss::fetch(ctx, st, &h_err, err.p, sizeof(uint32_t)));
        if (h_err) { idx->pos_ptr.release(); return ctx->fail(SS_ERR_INVALID, "ss_index_set_positions: pos_ptr is not non-decreasing"); }
    }
    if (ends[1] && !pos) { idx->pos_ptr.release(); return ctx->fail(SS_ERR_INVALID, "ss_index_set_positions: pos is NULL"); }
    SS_HIP(ctx, idx->pos.alloc(ends[1]));
    if (ends[1]) SS_HIP(ctx, hipMemcpyAsync(idx->pos.p, pos, ends[1] * sizeof(float), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

int32_t ss_index_set_weighted(ss_index* idx, const double* mag) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!mag) return ctx->fail(SS_ERR_INVALID, "ss_index_set_weighted: mag is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    SS_HIP(ctx, hipMemcpyAsync(idx->mag.p, mag, idx->n_docs * sizeof(double), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    idx->weighted = true;
    idx->mag2_valid = false;       // given magnitudes: their squares are not the exact sums an incremental update needs
    return SS_OK;
}

}  // extern "C"
