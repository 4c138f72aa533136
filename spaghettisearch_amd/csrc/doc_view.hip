// doc_view.hip — the doc-major view of one inverted table and the heaviest terms of a doc.
//
// The table is term-major (index.hpp): nothing on the device can say which terms doc d holds.  The view is the transpose,
//     doc_ptr u64[n_docs+1] | doc_term u32[P] | doc_w f32[P],
// row d = the terms with a posting of d in ascending term id, each with post_w as it stood when the view was built.  It is a
// snapshot and a pure function of the table: every step below is a stable sort, a search or a gather, none depends on timing.
//
// Build (ss_index_build_doc_view):
//   1. rocprim's stable radix sort of (post_doc[p], p) over ceil(log2 n_docs) key bits -> sorted docs, perm.  Term lists are
//      ascending by doc and follow each other in term order, so the postings of a doc keep their term order: row d comes out
//      ascending by term for free.
//   2. k_doc_ptr: doc_ptr[d] = first position of the sorted docs that is >= d (one binary search per doc: no counters, no scan).
//   3. k_post_term: term id of every posting (binary search of term_ptr, in posting order: neighbours share their path).
//   4. k_gather_view: doc_term[i] = post_term[perm[i]], doc_w[i] = post_w[perm[i]].
// Temporaries are freed as the build goes (sorted docs after 2, the sort's scratch after 1, post_term and perm after 4).
//
// k_doc_top_terms: one wave64 per requested doc, lanes striding the row; m rounds of a wave-wide maximum over the keys strictly
// below the previous winner.  key = ordered weight << 32 | ~term, ordered = the usual order-preserving transform of the float's
// bits with both zeros mapped to +0 and every NaN to 0: weight descending as float32 VALUES, then ascending term id, NaN last.
// Selection and copying only: the weights written are the stored bits.
#include "index.hpp"

#include <rocprim/rocprim.hpp>

namespace {

constexpr int TPB = 256;
inline unsigned grid_for(uint64_t n) { return ss::div_up(std::max<uint64_t>(n, 1), TPB); }

// doc_ptr[d] = number of postings whose doc is below d, d = 0 .. n_docs (sorted: ascending docs of all P postings)
__global__ __launch_bounds__(TPB) void k_doc_ptr(const uint32_t* __restrict__ sorted, uint32_t P, uint64_t n_docs, uint64_t* __restrict__ doc_ptr) {
    const uint64_t d = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (d > n_docs) return;
    uint32_t lo = 0, hi = P;                              // first position with sorted[pos] >= d
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)sorted[mid] < d) lo = mid + 1; else hi = mid;
    }
    doc_ptr[d] = lo;
}

// the term of posting p: the last t with term_ptr[t] <= p (empty lists share their start with the next one and are passed over)
__global__ __launch_bounds__(TPB) void k_post_term(const uint64_t* __restrict__ term_ptr, uint64_t n_terms, uint32_t P, uint32_t* __restrict__ post_term) {
    const uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P) return;
    uint64_t lo = 0, hi = n_terms;                        // term_ptr[lo] <= p < term_ptr[hi]  (term_ptr[0] = 0, term_ptr[n_terms] = P)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (term_ptr[mid] <= p) lo = mid; else hi = mid;
    }
    post_term[p] = (uint32_t)lo;
}

__global__ __launch_bounds__(TPB) void k_gather_view(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ post_term,
                                                     const float* __restrict__ post_w, uint32_t P, uint32_t* __restrict__ doc_term,
                                                     float* __restrict__ doc_w) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    const uint32_t p = perm[i];
    doc_term[i] = post_term[p];
    doc_w[i] = post_w[p];
}

// weight descending as float32 values (-0 = +0), NaN below everything: larger key = earlier
__device__ __forceinline__ uint32_t ordered_weight(float w) {
    if (w != w) return 0u;
    if (w == 0.0f) return 0x80000000u;                    // both zeros: the key of +0
    const uint32_t b = __float_as_uint(w);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // (~b = 0 only for a NaN's bits)
}

constexpr int TT_WAVES = 4;                               // waves (= requested docs) per workgroup

// Row i of the outputs = the first min(m, row length) entries of docs[i]'s view row in the order above; entries past n_out[i] are
// not written.  docs[] has been checked on the host (every id < n_docs).  w_out nullable.
__global__ __launch_bounds__(TT_WAVES * 64) void k_doc_top_terms(const uint64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ doc_term,
                                                                 const float* __restrict__ doc_w, const uint32_t* __restrict__ docs, uint64_t n,
                                                                 int32_t m, uint32_t* __restrict__ terms_out, float* __restrict__ w_out,
                                                                 int32_t* __restrict__ n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * TT_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                   // (a whole wave leaves: no lane of it takes part in the shuffles below)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = docs[i];
    const uint64_t b = doc_ptr[d], e = doc_ptr[d + 1];
    const uint32_t len = (uint32_t)(e - b);
    const uint32_t take = len < (uint32_t)m ? len : (uint32_t)m;
    const uint32_t* __restrict__ rt = doc_term + b;
    const float* __restrict__ rw = doc_w + b;
    uint64_t prev = ~0ull;                                // no key reaches it (its weight part would be a NaN's bits)
    for (uint32_t r = 0; r < take; r++) {
        uint64_t best = 0;                                // below every key (weight part 0 is a NaN, whose term part ~t is not 0)
        uint32_t best_j = 0;
        for (uint32_t j = lane; j < len; j += 64) {
            const uint64_t key = (uint64_t)ordered_weight(rw[j]) << 32 | (uint32_t)~rt[j];
            if (key < prev && key > best) { best = key; best_j = j; }
        }
        uint64_t win = best;
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(win, off, 64);
            win = o > win ? o : win;
        }
        // Keys are distinct inside a row — a term list holds a doc once (strictly ascending docs: ss_index_create, ss_index_apply_delta)
        // — so exactly one lane holds the winner; win = 0 (no key left, only if that invariant were broken) writes nothing.
        if (best == win && win != 0) {
            terms_out[i * (uint64_t)m + r] = rt[best_j];
            if (w_out) w_out[i * (uint64_t)m + r] = rw[best_j];
        }
        prev = win;
    }
    if (lane == 0) n_out[i] = (int32_t)take;
}

int32_t build_doc_view(ss_index* idx) {
    ss_ctx* ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t P64 = idx->n_post, N = idx->n_docs, T = idx->n_terms;
    if (P64 >= ((uint64_t)1 << 32)) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_index_build_doc_view: %llu postings (the view indexes them with 32 bits)", (unsigned long long)P64);
    const uint32_t P = (uint32_t)P64;
    idx->drop_doc_view();                                 // a view that exists goes FIRST (the header says so): the build's peak stays at 16 B per posting
    ss::DevBuf<uint64_t> dptr;
    ss::DevBuf<uint32_t> dterm;
    ss::DevBuf<float> dw;
    SS_HIP(ctx, dptr.alloc(N + 1));
    if (P == 0) {
        SS_HIP(ctx, hipMemsetAsync(dptr.p, 0, (N + 1) * sizeof(uint64_t), st));
    } else {
        ss::DevBuf<uint32_t> perm;
        SS_HIP(ctx, perm.alloc(P));
        {
            ss::DevBuf<uint32_t> sorted;
            SS_HIP(ctx, sorted.alloc(P));
            {
                unsigned bits = 1;
                while (bits < 32 && ((uint64_t)1 << bits) < N) bits++;
                rocprim::counting_iterator<uint32_t> iota(0u);
                size_t tmp_bytes = 0;
                SS_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const uint32_t*)idx->post_doc.p, sorted.p, iota, perm.p, (size_t)P, 0u, bits, st));
                ss::DevBuf<char> tmp;
                SS_HIP(ctx, tmp.alloc(tmp_bytes));
                SS_HIP(ctx, rocprim::radix_sort_pairs(tmp.p, tmp_bytes, (const uint32_t*)idx->post_doc.p, sorted.p, iota, perm.p, (size_t)P, 0u, bits, st));
            }                                             // (tmp goes: DevBuf::release waits for the device before a block can be reused)
            hipLaunchKernelGGL(k_doc_ptr, dim3(grid_for(N + 1)), dim3(TPB), 0, st, (const uint32_t*)sorted.p, P, N, dptr.p);
            SS_HIP(ctx, hipGetLastError());
        }                                                 // (sorted goes, likewise)
        ss::DevBuf<uint32_t> post_term;
        SS_HIP(ctx, post_term.alloc(P));
        SS_HIP(ctx, dterm.alloc(P));
        SS_HIP(ctx, dw.alloc(P));
        hipLaunchKernelGGL(k_post_term, dim3(grid_for(P)), dim3(TPB), 0, st, (const uint64_t*)idx->term_ptr.p, T, P, post_term.p);
        hipLaunchKernelGGL(k_gather_view, dim3(grid_for(P)), dim3(TPB), 0, st, (const uint32_t*)perm.p, (const uint32_t*)post_term.p,
                           (const float*)idx->post_w.p, P, dterm.p, dw.p);
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, hipStreamSynchronize(st));                // the view is complete, and an error of the build is reported, when the call returns
    idx->dv_ptr = std::move(dptr);
    idx->dv_term = std::move(dterm);
    idx->dv_w = std::move(dw);
    idx->has_doc_view = true;
    return SS_OK;
}

}  // namespace

namespace ss {
void launch_doc_top_terms(const ss_index* idx, const uint32_t* d_docs, uint64_t n, int32_t m, uint32_t* d_terms, float* d_w, int32_t* d_n, hipStream_t st) {
    hipLaunchKernelGGL(k_doc_top_terms, dim3(ss::div_up(n, TT_WAVES)), dim3(TT_WAVES * 64), 0, st, (const uint64_t*)idx->dv_ptr.p,
                       (const uint32_t*)idx->dv_term.p, (const float*)idx->dv_w.p, d_docs, n, m, d_terms, d_w, d_n);
}
}  // namespace ss

extern "C" {

int32_t ss_index_build_doc_view(ss_index* idx) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    try {
        return build_doc_view(idx);
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "ss_index_build_doc_view: host allocation failed");
    }
}

int32_t ss_index_drop_doc_view(ss_index* idx) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_index_drop_doc_view: the table has no doc view");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    idx->drop_doc_view();
    return SS_OK;
}

int32_t ss_index_read_doc_view(ss_index* idx, uint64_t* doc_ptr_out, uint32_t* doc_term_out, float* doc_w_out) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_index_read_doc_view: the table has no doc view (ss_index_build_doc_view)");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t P = idx->dv_term.n;
    if (doc_ptr_out) SS_HIP(ctx, hipMemcpyAsync(doc_ptr_out, idx->dv_ptr.p, (idx->n_docs + 1) * sizeof(uint64_t), hipMemcpyDefault, st));
    if (doc_term_out && P) SS_HIP(ctx, hipMemcpyAsync(doc_term_out, idx->dv_term.p, P * sizeof(uint32_t), hipMemcpyDefault, st));
    if (doc_w_out && P) SS_HIP(ctx, hipMemcpyAsync(doc_w_out, idx->dv_w.p, P * sizeof(float), hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

int32_t ss_index_doc_top_terms(ss_index* idx, uint64_t n, const uint32_t* docs, int32_t m, uint32_t* terms_out, float* w_out, int32_t* n_out) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_index_doc_top_terms: the table has no doc view (ss_index_build_doc_view)");
    if (m < 1 || m > SS_MAX_QUERY_TERMS) return ctx->fail(SS_ERR_INVALID, "ss_index_doc_top_terms: m = %d outside 1 .. %d", m, SS_MAX_QUERY_TERMS);
    if (n && (!docs || !terms_out || !n_out)) return ctx->fail(SS_ERR_INVALID, "ss_index_doc_top_terms: NULL argument");
    if (n == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    try {
        std::vector<uint32_t> h_docs(n);
        SS_HIP(ctx, ss::copy_in(st, h_docs.data(), docs, n * sizeof(uint32_t)));
        for (uint64_t i = 0; i < n; i++)
            if ((uint64_t)h_docs[i] >= idx->n_docs)
                return ctx->fail(SS_ERR_INVALID, "ss_index_doc_top_terms: docs[%llu] = %u, the table has %llu docs", (unsigned long long)i, h_docs[i],
                                 (unsigned long long)idx->n_docs);
        // outputs in device memory are written by the kernel itself; an output in host memory gets a device block of its own and only
        // the entries the kernel wrote are copied out (entries past n_out[i] stay as the caller left them)
        const bool dev_t = ss::on_device(terms_out), dev_w = w_out && ss::on_device(w_out), dev_n = ss::on_device(n_out);
        const size_t rows = (size_t)n * (size_t)m;
        ss::DevBuf<uint32_t> d_docs, d_terms;
        ss::DevBuf<float> d_w;
        ss::DevBuf<int32_t> d_n;
        SS_HIP(ctx, d_docs.alloc(n));
        if (!dev_t) SS_HIP(ctx, d_terms.alloc(rows));
        if (w_out && !dev_w) SS_HIP(ctx, d_w.alloc(rows));
        if (!dev_n) SS_HIP(ctx, d_n.alloc(n));
        SS_HIP(ctx, hipMemcpyAsync(d_docs.p, h_docs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        ss::launch_doc_top_terms(idx, d_docs.p, n, m, dev_t ? terms_out : d_terms.p, !w_out ? nullptr : dev_w ? w_out : d_w.p, dev_n ? n_out : d_n.p, st);
        SS_HIP(ctx, hipGetLastError());
        std::vector<int32_t> h_n;
        std::vector<uint32_t> h_terms;
        std::vector<float> h_w;
        const bool host_rows = !dev_t || (w_out && !dev_w);
        if (!dev_n || host_rows) {
            h_n.resize(n);
            SS_HIP(ctx, hipMemcpyAsync(h_n.data(), dev_n ? n_out : d_n.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        if (!dev_t) {
            h_terms.resize(rows);
            SS_HIP(ctx, hipMemcpyAsync(h_terms.data(), d_terms.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        if (w_out && !dev_w) {
            h_w.resize(rows);
            SS_HIP(ctx, hipMemcpyAsync(h_w.data(), d_w.p, rows * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        SS_HIP(ctx, hipStreamSynchronize(st));
        if (!dev_n) std::memcpy(n_out, h_n.data(), n * sizeof(int32_t));
        for (uint64_t i = 0; i < n && host_rows; i++) {
            const size_t cnt = (size_t)h_n[i], o = (size_t)i * (size_t)m;
            if (!dev_t) std::memcpy(terms_out + o, h_terms.data() + o, cnt * sizeof(uint32_t));
            if (w_out && !dev_w) std::memcpy(w_out + o, h_w.data() + o, cnt * sizeof(float));
        }
        return SS_OK;
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "ss_index_doc_top_terms: host allocation failed");
    }
}

}  // extern "C"
