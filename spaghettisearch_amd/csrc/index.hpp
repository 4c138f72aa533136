// index.hpp — one device-resident inverted table (inv[0] title / inv[1] body of the reference,
// database/database.go:85-99) as a term-major CSR over dense ids.
//
// HBM layout:  term_ptr u64[T+1] | post_doc u32[P] (strictly ascending inside a term) |
//              post_w f32[P] (normalised tf until ss_tfidf_build, tf*idf after) | mag f64[n_docs]
// Host keeps df per term (u32[T]) so that query planning needs no device round trip.
// index.hip: create / destroy / read / set_*; tfidf.hip: the weight and magnitude build; index_update.hip: deltas and resize.
#pragma once
#include "common.hpp"

struct ss_index {
    ss_ctx* ctx = nullptr;
    uint64_t n_docs = 0, n_terms = 0, n_post = 0;
    ss::DevBuf<uint64_t> term_ptr;
    ss::DevBuf<uint32_t> post_doc;
    ss::DevBuf<float> post_w;
    ss::DevBuf<double> mag;        // sqrt(sum w^2) per doc, valid once `weighted`
    ss::DevBuf<double> mag2;       // sum w^2 per doc (before the square root): what an incremental update adds to / subtracts from
    bool mag2_valid = false;       // mag2 matches the table (set by ss_tfidf_build / ss_index_refresh_magnitudes, not by ss_index_set_weighted)
    ss::DevBuf<uint64_t> pos_ptr;  // [P+1] positional postings (phrase search), optional
    ss::DevBuf<float> pos;         // positions as stored by the reference: float32, -100 = anchor/meta text
    ss::DevBuf<uint64_t> df_global; // [T] whole-corpus document frequencies when this table is one doc-range shard (optional)
    bool has_df_global = false;
    std::vector<uint64_t> h_term_ptr;  // host copy for query planning
    bool weighted = false;
    int users = 0;                 // scorers holding this index
    // doc-major view (doc_view.hip, optional): doc_ptr u64[n_docs+1] | doc_term u32[P] | doc_w f32[P], row d = the terms of doc d in
    // ascending term id with post_w as it stood at the build.  A snapshot: whatever changes postings or weights drops it.
    ss::DevBuf<uint64_t> dv_ptr;
    ss::DevBuf<uint32_t> dv_term;
    ss::DevBuf<float> dv_w;
    bool has_doc_view = false;
    void drop_doc_view() {
        dv_ptr.release();
        dv_term.release();
        dv_w.release();
        has_doc_view = false;
    }
    // MinHash signatures (dedup.hip, optional): sig u32[n_docs][sig_slots], row d = per slot the least hash of the terms of the view's
    // row d.  A snapshot of its own: whatever changes postings drops it, dropping or rebuilding the view does not.
    ss::DevBuf<uint32_t> sig;
    int32_t sig_slots = 0;
    bool has_signatures = false;
    void drop_signatures() {
        sig.release();
        sig_slots = 0;
        has_signatures = false;
    }
};

namespace ss {
// doc_view.hip: k_doc_top_terms over `n` doc ids in device memory (each < n_docs: checked by the caller); needs the view
void launch_doc_top_terms(const ss_index* idx, const uint32_t* d_docs, uint64_t n, int32_t m, uint32_t* d_terms, float* d_w, int32_t* d_n, hipStream_t st);
}  // namespace ss
