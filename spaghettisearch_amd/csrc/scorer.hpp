// scorer.hpp — the scorer object and everything of the scoring path that crosses a translation unit: score.hip (slice, phrase
// and merge kernels, scorer lifecycle), score_wave.hip, score_small.hip and constraint.hip (their kernels and launchers) and
// score_call.hip (the host side of a scoring call).  Every file that defines one of the ss:: functions below includes this
// header, so a definition is checked against the one prototype its callers see.  The calls that post-process a window of result rows
// (explain, passage, collapse, dedup, field and vector .hip) share the staging of their host arrays: hit_window.hpp on top of this file,
// the scorer's HitWindowBlocks and QueryTurn below.
// Launchers take the kernel parameters as `const void* params`: ScoreParams / ConstraintParams live in score_common.hpp's
// anonymous namespace (every translation unit has its own copy of the device code) and cannot appear in a shared prototype.
#pragma once
#include "score_common.hpp"

namespace ss {
// score.hip: thin launchers of its kernels (params: ScoreParams)
// k_score_slices over `n` slices from launch position `first` of params' order; raises the dynamic-LDS limits of the kernel (and of
// k_merge_topk, which goes with the unmasked kernel's mark) when the call's candidate buffer outgrows what the marks record.
// That happens here, at the launch — behind the call's timing event and whatever the call has enqueued before its slices kernel
// (allowed sets, k_score_small, phrase and wave kernels), and only in a call that launches a slices kernel; k_merge_topk is only
// ever launched behind one.  It matters on a scorer's first such call and when cb grows: a failure then returns the error with
// those earlier kernels already enqueued (they write this turn's workspaces and, for k_score_small, hits of a call that fails).
hipError_t launch_score_slices(const void* params, unsigned first, unsigned n, bool masked, int* lds_attr, int* lds_attr_masked, hipStream_t st);
void launch_phrase(const void* params, unsigned n_parts, unsigned n_q, hipStream_t st);   // k_phrase_match (n_parts > 0) + k_phrase_close
void launch_merge_topk(const void* params, unsigned n_q, hipStream_t st);
void launch_merge_flat(const void* params, unsigned n_merge, hipStream_t st);

// score_wave.hip
size_t score_wave_prep_bytes(unsigned n_slices);
void launch_wave_prep(const void* params, unsigned n_slices, void* prep, hipStream_t st);
void launch_score_wave(const void* params, unsigned n_slices, const void* prep, hipStream_t st);
int score_wave_max_lists();
int score_wave_max_k();
// score_small.hip: one workgroup per small query (every posting scored exactly, hits written by the kernel itself)
uint32_t score_small_cap();
uint32_t score_small_cap_a();
int score_small_max_k();
int score_small_max_lists();
int32_t launch_score_small(const void* params, unsigned n_a, unsigned n_b, hipStream_t st);
void launch_small_copy(const void* params, unsigned n_small, hipStream_t st);
void score_small_report();
void score_wave_diag_dump();
uint32_t constraint_blocks(uint64_t n_words);
void launch_constraint_masks(const void* params, uint32_t n_sets, hipStream_t st);
// field.hip (params: FieldParams): k_field_masks over the params' sets; the geometry for callers and tests
uint32_t field_mask_docs();                     // docs of one workgroup
uint32_t field_mask_group();                    // sets that share one read of the field columns
void launch_field_masks(const void* params, hipStream_t st);
}  // namespace ss
struct ss_scorer;
struct QueryConstraints;
struct QueryRanges;
namespace ss {
// vector.hip, for hybrid.hip: the query vectors as the vector kernels load them (ss_vector_topk's staging: *staged is set when they
// came from host memory, so the call waits before it returns), and k_vec_hit_scores as ss_hit_vector_scores launches it over rows
// and counts in device memory
int32_t vec_queries_to_device(ss_scorer* s, const int8_t* qvec, size_t bytes, const int8_t** out, bool* staged);
void launch_vec_hit_scores(ss_scorer* s, const int8_t* d_qvec, const ss_hit* d_hits, const int32_t* d_n_hits, int32_t n_q, int32_t k_in,
                           int32_t* d_out, hipStream_t st);
// vector.hip, for maxsim.hip: k_vec_sort_hits as ss_rerank_hits_by_vector launches it, over rows, counts and the scores of the window's
// entries [n_q][k_in] (SS_NO_VEC_SCORE: a row without a score) in device memory; d_scores_out [n_q][k] may be NULL.  Enqueues only.
void launch_vec_sort_hits(const int32_t* d_scores, const ss_hit* d_hits, const int32_t* d_n_hits, int32_t n_q, int32_t k_in, int32_t first,
                          int32_t k, ss_hit* d_hits_out, int32_t* d_n_hits_out, int32_t* d_scores_out, hipStream_t st);
// vector.hip, for maxsim_topk.hip: k_vec_merge as ss_vector_topk launches it, one workgroup per query over its n_chunks * k partial keys
// (unused slots 0) in device memory.  n_chunks * k < 2^32.  Enqueues only.
void launch_vec_merge(const uint64_t* d_part, uint32_t n_chunks, int32_t n_q, int32_t k, ss_vec_hit* d_hits_out, int32_t* d_n_hits_out,
                      hipStream_t st);
// maxsim.hip, for maxsim_topk.hip: qt_ptr fetched to the host and checked with qtok as ss_hit_maxsim_scores checks them (*qt: the tiles of
// 16 query-token slots the call's largest m_q needs; enqueues nothing that writes), and the query tokens 16-byte aligned on the device
// with qt_ptr rebased in s->d_ms_qptr (*staged is set when they came from host memory, so the call waits before it returns)
int32_t maxsim_check_query_tokens(ss_ctx* ctx, const char* entry, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok,
                                  std::vector<uint32_t>* h_ptr, uint32_t* qt);
int32_t maxsim_query_tokens_to_device(ss_scorer* s, const std::vector<uint32_t>& h_ptr, const int8_t* qtok, const int8_t** d_qtok, bool* staged);
// vector.hip, for vector_lists.hip: k_vec_topk and k_vec_merge as ss_vector_topk launches them, over any table [n_rows > 0][vec_dim] of
// int8 rows in device memory, without masks: d_qvec [n_q][vec_dim] 16-byte aligned, rows and counts to device memory.  Enqueues only.
int32_t vec_table_topk(ss_scorer* s, const char* who, const int8_t* table, uint64_t n_rows, int32_t n_q, const int8_t* d_qvec, int32_t k,
                       ss_vec_hit* d_hits, int32_t* d_n_hits);
// vector_lists.hip, for vector.hip: ss_scorer_set_doc_vectors drops the lists, which describe the old table
void vec_lists_drop(ss_scorer* s);
}  // namespace ss

// Where a scoring call left its rows when they stay inside the scorer (ss::score_into_turn): the block of the plan turn the call took.
// The block is that turn's until the turn comes round again, i.e. until the scorer has waited for the turn's batch_ev: whoever reads it
// on the context's stream records the turn's batch_ev again behind the reader.
struct TurnRows {
    size_t rows = 0, n_q = 0;                   // in: hits and counts to make room for
    ss_hit* hits = nullptr;                     // out: [n_q][k]
    int32_t* n_hits = nullptr;                  // out: [n_q]
    int turn = -1;                              // out: -1 if the call took no turn (it failed before staging)
};
namespace ss {
// score_call.hip (query_len: as ss_score_topk's, NULL = term count)
int32_t score_into_turn(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const double* topic_probs,
                        const int32_t* mask_id, int32_t k, TurnRows* out, const int32_t* query_len = nullptr);
// score_call.hip, for facet.hip: the allowed sets of a batch exactly as ss_score_topk_filtered forms them for the same mask ids,
// constraint arrays and range clauses.  Runs that call's checks (its codes, nothing enqueued on a refusal), takes the next plan turn,
// and enqueues k_constraint_masks / k_field_masks on the context's stream into the turn's set buffer.  The sets are the turn's: whoever
// reads them on the context's stream records the turn's batch_ev again behind the reader.
struct AllowedSets {
    std::vector<int32_t> set_of;                // [n_q] the row of `words` that is the query's allowed set, -1: every doc
    const uint32_t* words = nullptr;            // device: the turn's sets, or the registered masks when no query has a constraint
    uint64_t stride = 0;                        // words per row (bits at and past n_docs of a row may be set)
    int turn = -1;
};
int32_t allowed_sets_into_turn(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const int32_t* mask_id, const QueryConstraints* cons,
                               const QueryRanges* ranges, AllowedSets* out);
}  // namespace ss

// Everything one plan turn owns.  A scoring call takes the next turn (acquire_turn) and waits for batch_ev there, i.e. for the batch
// that used the turn TURNS calls ago, before any of these buffers is grown or rewritten.
struct Turn {
    // pinned staging for the plan, double-buffered: a call that returns results in device memory does not wait
    // for the GPU, so the next call plans (and fills the other buffer) while this one's copy and kernels run
    ss::PinBuf h_plan;
    ss::DevBuf<unsigned char> d_plan, d_wprep; // the plan on the device, one buffer per turn: batch i+1's upload runs beside batch i's kernels
    ss::DevBuf<Rec> d_x[4];                    // phrase result lists: scoring records (one set per turn: batches overlap)
    ss::DevBuf<float> d_xw[4];                 // ... and their float32 weight sums
    ss::DevBuf<uint32_t> d_xcnt, d_pcnt;
    ss::DevBuf<uint64_t> d_so_key;             // the slices' candidates, one set per turn ("score.pipeline": batch i's merge reads its set while batch i+1 fills the other)
    ss::DevBuf<uint32_t> d_so_doc, d_so_cnt, d_qcnt;
    size_t qcnt_zeroed = 0;                    // counters known to be zero (k_merge_flat leaves its query's counter at zero)
    ss::DevBuf<ss_hit> d_small_stage;          // k_score_small's rows of a pipelined batch (k_small_copy moves them on the caller's stream)
    ss::DevBuf<int32_t> d_small_stage_n;
    ss::DevBuf<uint32_t> d_sets;               // ss_score_topk_constrained: the batch's allowed sets [n_sets][stride], built by k_constraint_masks
    ss::DevBuf<ss_hit> d_hits;                 // ss_similar_topk / ss_related_terms: the batch's rows, read by k_drop_seed / k_hit_docs on the caller's stream
    ss::DevBuf<int32_t> d_n;
    ss::PinBuf h_rel;                          // ss_related_terms: the queries' own terms go up through it (see d_rel_q below)
    ss::Event batch_ev;                        // recorded behind the kernels of the batch that read this turn's buffers, and again behind whoever reads the turn's rows last
    ss::Event wave_ev;                         // "score.pipeline": behind k_score_wave on the context's wave stream; the merge on the caller's stream waits for it
    ss::Event slice_ev;                        // ... and behind the k_score_slices part of a split batch on ANOTHER wave stream
    ss::Event set_ev;                          // ... behind k_constraint_masks, when k_score_small runs on another stream
    ss::PinBuf h_facet;                        // ss_facet_counts / ss_field_topk / ss_top_groups / ss_field_stats / ss_field_histogram (match_set.hpp): the list table (and bucket table) go up through it (one set per turn,
    ss::DevBuf<unsigned char> d_facet;         // free after the wait for batch_ev like the plan's)
};

// ss_explain_hits / ss_best_passages: neither takes a plan turn (they score nothing), so each has TURNS turns of its own.  Per turn: the
// pinned block the queries' table goes up through (ss::hitwin::query_table_fill), its device copy, and an event behind the kernel that
// read them (waited for before the block is rewritten: the call never waits for its own copy).
struct QueryTurn {
    ss::PinBuf h_q;
    ss::DevBuf<uint32_t> d_q;
    ss::Event ev;
};

// Device blocks of the HOST arrays of the calls that take a window of result rows (hit_window.hpp), one set for all of them, grow-only.
// The invariant: a call that touches one of these blocks synchronizes the context's stream before it returns.  So nothing in flight
// reads a block when a later call grows (frees) it, and whichever entry point comes next may take every block for its own arrays.
struct HitWindowBlocks {
    ss::DevBuf<ss_hit> rows_in, rows_out;      // hits [n_q][k_in], hits_out [n_q][k]
    ss::DevBuf<int32_t> n_in, n_out, kept_out; // n_hits, n_hits_out, n_kept_out [n_q]
    ss::DevBuf<unsigned char> extra;           // the one further output of a call, as bytes: per output row (same, similar, values, scores)
                                               // or per entry of the input window (ss_term_match, ss_passage, field values, scores)
};

struct ss_scorer {
    ss_ctx* ctx = nullptr;
    ss_index* title = nullptr;
    ss_index* body = nullptr;
    uint64_t n_docs = 0, n_terms = 0;
    ss::DevBuf<Rec> t_rec, b_rec;              // scoring records {doc, impact}
    // combined lists (k_score_wave): title + body postings of a term merged by doc, field in bit 31 of the doc word
    ss::DevBuf<Rec> c_rec;
    ss::DevBuf<uint32_t> c_skip;
    ss::DevBuf<float> c_w;
    ss::DevBuf<uint64_t> c_ptr;
    bool has_combined = false;
    uint64_t c_pad_block = 0;
    ss::DevBuf<float> t_kth, b_kth;             // [T][KTH_N] k'-th largest impact per term (threshold floor)
    bool clean = true;                          // weights >= 0 and finite, magnitudes positive and finite where a weight is not 0
    bool prior_clean = true;                    // every prior value >= 0 and finite
    ss::DevBuf<double> prior;
    std::vector<double> prior_max, prior_min;   // per topic
    int k_topics = 0;
    ss::DevBuf<uint32_t> masks;                 // ss_scorer_set_doc_masks: [n_masks][mask_words] allow-lists
    int32_t n_masks = 0;
    uint64_t mask_words = 0;
    int lds_attr = 0, lds_attr_masked = 0;
    // per-call workspaces, grow-only (no hipMalloc/hipFree on the steady-state query path)
    // Turns of per-batch buffers: the host runs at most TURNS batches ahead.  (Three were measured for the pipelined mode, so that a
    // batch's plan upload and k_wave_prep — which do not fit beside k_score_wave's three waves of 168 VGPRs per SIMD — are enqueued
    // one batch earlier: 0.395 against 0.399 ms per batch, not worth a third set of buffers.)
#ifndef SS_TURNS
#define SS_TURNS 3
#endif
    static constexpr int TURNS = SS_TURNS;
    unsigned wave_turn = 0;                    // which wave stream the next pipelined batch takes
    Turn turn[TURNS];
    int plan_turn = 0;
    ss::PinBuf h_res;                // pinned landing block of small host results (one device-to-host copy for hits + counts)
    static constexpr size_t H_RES_BYTES = 128 << 10;
    ss::DevBuf<uint32_t> d_qticket;
    size_t qticket_zeroed = 0;         // tickets known to be zero (every fused call leaves them so)
    // ss_similar_topk's seeds, their terms and term counts: written and read on the context's stream only (grow-only), the terms
    // brought to the host through a pinned block
    ss::DevBuf<uint32_t> d_sim_seeds, d_sim_terms;
    ss::DevBuf<int32_t> d_sim_cnt;
    ss::PinBuf h_sim;
    // ss_related_terms (related.hip): the hits' docs, their heaviest terms (ids, weights, counts), the queries' own terms and the
    // device blocks of host outputs: written and read on the context's stream only (grow-only).  The queries' own terms go up through a
    // pinned block per turn (Turn::h_rel), rewritten only after the wait for the turn's batch_ev: the call never waits for its own copy.
    ss::DevBuf<uint32_t> d_rel_docs, d_rel_terms, d_rel_q, d_rel_out_terms;
    ss::DevBuf<float> d_rel_w;
    ss::DevBuf<int32_t> d_rel_cnt;
    ss::DevBuf<double> d_rel_out_score;
    // ss_explain_hits / ss_best_passages: their own turns.  win: the device blocks of host arrays of every call that takes a window.
    QueryTurn exp[TURNS], pas[TURNS];
    int exp_turn = 0, pas_turn = 0;
    HitWindowBlocks win;
    // ss_scorer_set_doc_groups (collapse.hip): [n_docs] the group of every doc, SS_NO_GROUP = a group of its own.
    ss::DevBuf<uint32_t> groups;
    bool has_groups = false;
    // ss_scorer_set_doc_fields (field.hip): [n_fields][n_docs] signed 64-bit values per doc.  ss_doc_field_masks: the set table of a
    // call and the device block of a HOST words_out (grow-only; the call waits before it returns).
    ss::DevBuf<int64_t> fields;
    int32_t n_fields = 0;
    ss::DevBuf<unsigned char> d_fld_tab;
    ss::DevBuf<uint32_t> d_fld_words;
    // ss_scorer_set_doc_vectors (vector.hip): [n_docs][vec_dim] signed 8-bit values, vec_dim 0 = no table.  ss_vector_topk: the chunks'
    // partial key lists, the queries' mask ids (through a pinned block whose last copy ev_vec_mid stands behind), the dynamic LDS
    // already granted to k_vec_topk<QT> and the device blocks of HOST hits_out / n_hits_out (d_vec_hits, d_vec_n: grow-only; the call
    // waits before it returns).  d_vec_q: query vectors that are host memory or not 16-byte aligned.  d_vec_scores: the re-rank's
    // scores between its two kernels.
    ss::DevBuf<int8_t> vec;
    int32_t vec_dim = 0;
    ss::DevBuf<uint64_t> d_vec_part;
    ss::DevBuf<int8_t> d_vec_q;
    ss::DevBuf<int32_t> d_vec_mid, d_vec_n, d_vec_scores;
    ss::PinBuf h_vec_mid;
    ss::Event ev_vec_mid;
    int vec_lds_attr[5] = {0, 0, 0, 0, 0};
    ss::DevBuf<ss_vec_hit> d_vec_hits;
    // ss_scorer_set_vector_lists (vector_lists.hip; vl_n_lists 0 = none): the centroids [vl_n_lists][vec_dim], the list-major copy of
    // the vector rows with the doc of every row, list_begin [vl_n_lists + 1] and, on the host, the list lengths in descending order
    // (the plan's slot bound).  vl_rows: docs that are in a list.  ss_vector_topk_probed, all grow-only and used on the context's
    // stream: the probe rows [n_q][P] and their counts, per list the queries' count / run begin / fill cursor (d_vl_cnt: 3 arrays), the
    // runs of (query, probe rank) pairs, the items' scan, per pair its first partial slot and per query its slot count, the partial
    // lists, the device blocks of HOST outputs, the dynamic LDS already granted to k_vec_topk_lists<QT>.  ss_vector_assign_lists: the
    // centroids it is given and the top-1 rows of one batch.
    int32_t vl_n_lists = 0;
    uint64_t vl_rows = 0;
    ss::DevBuf<int8_t> vl_centroids, vl_vec;
    ss::DevBuf<uint32_t> vl_row_doc, vl_list_begin;
    std::vector<uint32_t> vl_len_desc;
    ss::DevBuf<ss_vec_hit> d_vl_probe, d_vl_hits, d_vl_assign;
    ss::DevBuf<int32_t> d_vl_probe_n, d_vl_n, d_vl_assign_n, d_vl_mid;
    ss::DevBuf<uint32_t> d_vl_cnt, d_vl_run, d_vl_slot, d_vl_nslots, d_vl_probes_out;
    ss::DevBuf<uint64_t> d_vl_item_begin, d_vl_part;
    ss::DevBuf<int8_t> d_vl_cent;
    int vl_lds_attr[5] = {0, 0, 0, 0, 0};
    ss::DevBuf<ss_hit> d_hits;
    // ss_score_docs / ss_fuse_hits / ss_hybrid_topk (hybrid.hip).  hyb: the turns the queries' table goes up through, as exp / pas.
    // The blocks, grow-only, written and read on the context's stream only: the device copies of HOST docs / vec / n_vec (the call
    // waits before it returns, as with HitWindowBlocks); between k_fuse_hits and k_fuse_page the candidates [n_q][3][k_lex + k_vec]
    // (doc | lex_rank + vec_rank << 16 | slot) and the counts [3][n_q] (union, docs without a lexical row, docs without a vector
    // score), those docs, their rows from k_score_docs and their scores from k_vec_hit_scores (whose input rows carry .doc only);
    // ss_hybrid_topk's vector window.
    QueryTurn hyb[TURNS];
    int hyb_turn = 0;
    ss::DevBuf<uint32_t> d_hyb_docs_in, d_hyb_cand, d_hyb_miss_docs;
    ss::DevBuf<ss_vec_hit> d_hyb_vec_in, d_hyb_vec_win;
    ss::DevBuf<int32_t> d_hyb_nvec_in, d_hyb_counts, d_hyb_miss_scores, d_hyb_nvec_win;
    ss::DevBuf<ss_hit> d_hyb_miss_rows, d_hyb_miss_vec_rows;
    // ss_diversify_hits (diversify.hip), grow-only, written and read on the context's stream only: the Gram matrices of one group of
    // queries [group][pitch][pitch] (bounded by option "div.scratch_bytes"; the groups of a call re-use it in stream order) and the
    // rows' relevance from k_vec_hit_scores [n_q][k_in].
    ss::DevBuf<int32_t> d_div_gram, d_div_rel;
    // ss_scorer_set_doc_tokens (maxsim.hip): tok [tok_rows][tok_dim] signed 8-bit token vectors, doc d's at rows tok_ptr[d] ..
    // tok_ptr[d + 1]; tok_dim 0 = no table.  Independent of vec / vec_dim.  ss_hit_maxsim_scores / ss_rerank_hits_by_maxsim, grow-only and
    // used on the context's stream: d_ms_q, query tokens that are host memory or not 16-byte aligned; d_ms_qptr, the call's qt_ptr (up
    // through a pinned block whose last copy ev_ms_qptr stands behind); d_ms_scores, the re-rank's scores between its two kernels; the
    // dynamic LDS already granted to k_maxsim_scores<QT>.
    ss::DevBuf<int8_t> tok;
    ss::DevBuf<uint64_t> tok_ptr;
    int32_t tok_dim = 0;
    uint64_t tok_rows = 0;
    ss::DevBuf<int8_t> d_ms_q;
    ss::DevBuf<uint32_t> d_ms_qptr;
    ss::DevBuf<int32_t> d_ms_scores;
    ss::PinBuf h_ms_qptr;
    ss::Event ev_ms_qptr;
    int ms_lds_attr[5] = {0, 0, 0, 0, 0};
    // ss_maxsim_topk (maxsim_topk.hip): tok_cut [tok_slices + 1], the first doc at or behind every multiple of mtp::SLICE_TOKENS tokens
    // (maxsim_topk_plan.hpp; built, freed and replaced with the token table; tok_slices 0 = a table without a token, or none).  Grow-only
    // and used on the context's stream: the chunks' partial key lists, the queries' mask ids (up through a
    // pinned block whose last copy ev_mst_mid stands behind) and the device blocks of HOST hits_out / n_hits_out.
    ss::DevBuf<uint32_t> tok_cut;
    uint64_t tok_slices = 0;
    ss::DevBuf<uint64_t> d_mst_part;
    ss::DevBuf<int32_t> d_mst_mid, d_mst_n;
    ss::DevBuf<ss_vec_hit> d_mst_hits;
    ss::PinBuf h_mst_mid;
    ss::Event ev_mst_mid;
    // ss_facet_counts (facet.hip): the device block of HOST outputs, totals | mask counts | bucket counts (grow-only; the call waits
    // before it returns)
    ss::DevBuf<uint32_t> d_facet_out;
    // ss_field_topk (field_topk.hip), grow-only, written and read on the context's stream only: the partial lists of one group of
    // queries, keys | doc ids | run counts (bounded by option "ftopk.scratch_bytes"; the groups of a call re-use it in stream order), and
    // the device block of HOST outputs, values | docs | n_out | n_match (the call waits before it returns)
    ss::DevBuf<unsigned char> d_ftopk_part, d_ftopk_out;
    // ss_top_groups / ss_scorer_group_values (group_topk.hip).  The group ranks of the registered table, built by the first call that
    // needs them and dropped with the table (drop_group_ranks): gval [n_groups] the table's distinct values != SS_NO_GROUP ascending,
    // grank [n_docs] the index of group[d] in gval (0xFFFFFFFF for SS_NO_GROUP).  Grow-only, written and read on the context's stream
    // only: the counter rows of one group of queries [group][row stride] (bounded by option "gtopk.scratch_bytes"; the groups of a call
    // re-use it in stream order) and the device block of HOST outputs, rows | n_out | n_groups | n_ungrouped | n_match (the call waits
    // before it returns)
    ss::DevBuf<uint32_t> gval, grank;
    uint32_t n_groups = 0;
    bool has_group_ranks = false;
    void drop_group_ranks() {
        gval.release();
        grank.release();
        n_groups = 0;
        has_group_ranks = false;
    }
    ss::DevBuf<uint32_t> d_gtopk_rows;
    ss::DevBuf<unsigned char> d_gtopk_out;
    // ss_field_stats / ss_field_histogram (field_stats.hip), grow-only, written and read on the context's stream only: the partial
    // entries [group][runs][fields] or the counter rows [group][row stride] of one group of queries (bounded by option
    // "fstats.scratch_bytes"; the groups of a call re-use the block in stream order) and the device block of HOST outputs, stats |
    // n_match or counts | tails (the call waits before it returns)
    ss::DevBuf<unsigned char> d_fstats_part, d_fstats_out;
    // ss_hit_proximity / ss_rerank_hits_by_proximity / ss_score_topk_proximity (proximity.hip).  prx: the turns the queries' table goes
    // up through, as exp / pas.  Grow-only, written and read on the context's stream only: the entries of a re-rank's window
    // [n_q][k_in] as six dwords each, between k_hit_proximity and k_prox_sort_hits, and the device block of HOST scores_out / prox_out,
    // scores | entries (the call waits before it returns)
    QueryTurn prx[TURNS];
    int prx_turn = 0;
    ss::DevBuf<uint32_t> d_prx_entries;
    ss::DevBuf<unsigned char> d_prx_out;
    // ss_hit_features / ss_rerank_hits_by_model (rank_model.hip).  Grow-only, written and read on the context's stream only: the
    // feature matrix of a re-rank's window [n_q][k_in][SS_RANK_N_FEATURES] and its scores [n_q][k_in], between k_hit_features,
    // k_forest_eval and k_model_sort_hits, and the device block of HOST prox | vec_scores | query_len (the call waits before it returns)
    ss::DevBuf<double> d_rm_feat, d_rm_scores;
    ss::DevBuf<unsigned char> d_rm_in;
    // ss_score_topk_submit / _collect: batches in flight whose hits go to HOST memory.  A slot: device buffers the kernels write and
    // an event behind them.
    static constexpr int INFLIGHT = SS_SCORE_INFLIGHT;
    struct AsyncSlot {
        ss::DevBuf<ss_hit> hits;
        ss::DevBuf<int32_t> n_hits;
        ss::Event ev;                        // behind the batch's kernels on the caller's stream
        void* pin = nullptr;                 // "score.collect_pinned": the copy-out lands here first
        size_t pin_cap = 0;
        bool pin_mode = false;
        uint64_t ticket = 0;                 // 0 = free
        bool collecting = false;             // a collect call is waiting for / copying this slot outside the lock
        void* pin_n = nullptr;               // pinned landing block of the counts (a small copy into pageable memory costs ~20 us more)
        size_t pin_n_cap = 0;
        int32_t n_q = 0, k = 0;
    } aslot[INFLIGHT];
    uint64_t next_ticket = 1;
    hipStream_t out_stream = nullptr;        // collect's copies
    ss::DevBuf<int32_t> d_nhits;
    // What the members cannot do themselves.  (ss_scorer_destroy has set the device and drained the context's streams before this runs.)
    ~ss_scorer() {
        if (out_stream) { (void)hipStreamSynchronize(out_stream); (void)hipStreamDestroy(out_stream); }
        for (auto& a : aslot) {
            if (a.pin) ctx->pin_free(a.pin, a.pin_cap);
            if (a.pin_n) ctx->pin_free(a.pin_n, a.pin_n_cap);
        }
    }
};

template <typename T>
inline hipError_t ensure(ss::DevBuf<T>& b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    return b.alloc(n + n / 2 + 16);
}
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// A pointer array of the ABI (`name`_ptr: n + 1 offsets, host or device memory) copied to `dst` and checked to be non-decreasing;
// `entry`: the entry point the caller sees in the error.  What else a site demands of its array (a first offset of 0, a bound on
// every step) it checks itself.
inline int32_t fetch_ptr_array(ss_ctx* ctx, const char* entry, const char* name, const uint32_t* src, size_t n, uint32_t* dst) {
    SS_HIP(ctx, ss::copy_in(ctx->stream, dst, src, (n + 1) * sizeof(uint32_t)));
    for (size_t q = 0; q < n; q++)
        if (dst[q + 1] < dst[q]) return ctx->fail(SS_ERR_INVALID, "%s: %s_ptr not non-decreasing", entry, name);
    return SS_OK;
}

// the constraint arrays of ss_score_topk_constrained (NULL pointers: none)
struct QueryConstraints { const uint32_t *req_ptr, *req_terms, *exc_ptr, *exc_terms; };
// the range clauses of ss_score_topk_filtered (rng_ptr NULL: none)
struct QueryRanges { const uint32_t* rng_ptr; const ss_doc_range* rng; };
