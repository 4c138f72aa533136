/*
 * spaghetti_rank.h — C ABI of the MI355X-native ranking hot path.
 *
 * This is the drop-in boundary for SpaghettiSearch's ranking path.  The
 * reference has no FFI/plugin layer: its boundary is three exported Go
 * functions.  A cgo shim that keeps those three signatures
 * (go/ranking, go/retrieval) binds exactly the entry points
 * declared here; each entry point cites the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns int32 status, 0 = SS_OK; ss_last_error() gives text.
 *     The Go shim turns any non-zero status into panic(err), matching the
 *     reference's error policy (pagerank.go:20,29,49,57,76,81).
 *   - input pointers may be host OR device memory (copied with
 *     hipMemcpyDefault before the call returns: cgo forbids retaining Go
 *     pointers).  Output pointers likewise, caller-allocated.
 *   - opaque handles are freed by the matching *_destroy.
 *   - one ss_ctx per GPU per process (one process per GPU for multi-GPU).
 *   - compute entry points are thread-safe on a shared handle
 *     (retrieval.Retrieve is called from one goroutine per HTTP request,
 *     cmd/server/server.go:47); calls on one ctx are serialised internally.
 *   - there is NO CPU fallback: without a gfx950 device ss_init fails.
 */
#ifndef SPAGHETTI_RANK_H
#define SPAGHETTI_RANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 5): ss_score_topk_submit / ss_score_topk_collect exist; ss_graph_create may return while its last build kernels
 * still run on the context's stream (everything that reads the graph is ordered behind them); "score.pipeline" defaults to 2
 * internal wave streams and ss_last_kernel_ms(1) is the device time of the last scoring call's kernels on the stream that
 * carries its merge.  A binding checks ss_abi_version() == SS_ABI_VERSION at load.
 * Added under 4, nothing changed: ss_scorer_set_doc_masks and ss_score_topk_masked (per-query doc allow-lists);
 * ss_score_topk_constrained (required and excluded query terms); ss_index_build_doc_view / _drop_doc_view / _read_doc_view,
 * ss_index_doc_top_terms and ss_similar_topk (doc-major view of a table, a doc's heaviest terms, "similar pages");
 * SS_MAX_FEEDBACK_DOCS and ss_related_terms (refinement words from a query's top hits);
 * ss_term_match and ss_explain_hits (which query tokens matched each result row, and where);
 * ss_passage and ss_best_passages (per result row the body window that covers most of the query's terms);
 * SS_NO_GROUP, ss_scorer_set_doc_groups, ss_collapse_hits and ss_score_topk_collapsed (at most g rows per site, with paging);
 * SS_MAX_WORD_BYTES, SS_MAX_EDIT_DIST, SS_MAX_SUGGEST, ss_lexicon, ss_lexicon_create / _set_freq / _get_info / _read_order / _destroy,
 * ss_lexicon_prefix and ss_lexicon_suggest (the words of the vocabulary on the device: word list by prefix, spelling suggestions);
 * SS_MAX_SIG_SLOTS, SS_SIG_EMPTY, ss_index_build_signatures / _drop_signatures / _read_signatures and ss_dedup_hits (a MinHash
 * signature per doc, near-duplicate rows dropped from a result window);
 * SS_MAX_LINKS, SS_LINKS_PARENTS / _CHILDREN, ss_graph_set_link_key, ss_graph_top_links and ss_graph_hit_links (the best parents or
 * children of a page by a registered per-node key, and its edge count);
 * SS_MAX_DOC_FIELDS, SS_MAX_RANGE_CLAUSES, SS_NO_FIELD_VALUE, ss_doc_range, ss_scorer_set_doc_fields, ss_doc_field_masks,
 * ss_score_topk_filtered, ss_sort_hits_by_field and ss_hit_fields (per-doc integer fields: range filters, sort by field, read-out);
 * SS_MAX_VEC_DIM, SS_NO_VEC_SCORE, ss_vec_hit, ss_scorer_set_doc_vectors, ss_vector_topk, ss_hit_vector_scores and
 * ss_rerank_hits_by_vector (one int8 vector per doc: exact nearest neighbours by integer dot product, a window re-ranked by it);
 * SS_FUSE_RRF / _WEIGHTED, ss_fuse_params, ss_fused, ss_score_docs, ss_fuse_hits and ss_hybrid_topk (the lexical row of any given doc,
 * a lexical and a vector list fused into one ranked, paged list, and both searches plus the fusion in one call);
 * SS_MAX_VEC_LISTS, SS_NO_LIST, ss_scorer_set_vector_lists, ss_vector_assign_lists and ss_vector_topk_probed (the vector table cut into
 * lists around centroids: the exact top k over the docs of the n_probe lists nearest to a query, not over every doc);
 * ss_pr_lean_sweeps (how many sweeps of a state were launched in the lean form of option "pr.lean_sweeps");
 * SS_DIV_WEIGHT_MAX, ss_div_info and ss_diversify_hits (a window re-ranked greedily by relevance minus similarity to the rows already
 * chosen: maximal marginal relevance over the doc vectors);
 * SS_MAX_FACET_BUCKETS and ss_facet_counts (how many docs a query matches: in all, per registered allow-list, per value bucket);
 * ss_field_topk (the exact top k of ALL docs a query matches, ordered by a doc field);
 * ss_group_count, ss_scorer_group_values and ss_top_groups (the m groups of the doc -> group table that hold most of a query's matches);
 * SS_MAX_COMPLETE and ss_lexicon_complete (the m most frequent words that start with a prefix: word completions);
 * ss_proximity, ss_hit_proximity, ss_rerank_hits_by_proximity and ss_score_topk_proximity (per result row the smallest body span that
 * holds every query term the doc has, and a window re-ranked by it);
 * SS_RANK_N_FEATURES, SS_MAX_RANK_FEATURES, SS_MAX_RANK_TREES, ss_tree_node, ss_rank_model, ss_rank_model_info, ss_rank_model_create /
 * _destroy / _get_info / _eval, ss_hit_features and ss_rerank_hits_by_model (learned ranking: the signals of a window's rows as a
 * feature matrix, a tree ensemble evaluated per row, a window re-ranked by its scores);
 * SS_MAX_QUERY_TOKENS, ss_scorer_set_doc_tokens, ss_hit_maxsim_scores and ss_rerank_hits_by_maxsim (one int8 vector per doc token and
 * per query token: late-interaction MaxSim scores of a window's rows, a window re-ranked by them);
 * ss_maxsim_topk (the exact top k by that score over every doc of the token table);
 * SS_MAX_HIST_BINS, ss_field_stat, ss_hist_tail, ss_field_stats and ss_field_histogram (over ALL docs a query matches: the smallest and
 * largest value, the exact sum and the number of missing values of a doc field, and the matches per bin of a field). */
#define SS_ABI_VERSION 4

enum {
    SS_OK = 0,
    SS_ERR_INVALID = 1,      /* bad argument (null handle, k<=0, ids out of range, ...) */
    SS_ERR_NO_DEVICE = 2,    /* no usable gfx950 device / HIP runtime error at init */
    SS_ERR_HIP = 3,          /* HIP runtime error (text in ss_last_error) */
    SS_ERR_OOM = 4,          /* device or host allocation failed */
    SS_ERR_UNSORTED = 5,     /* a posting list is not strictly ascending by doc id */
    SS_ERR_STATE = 6,        /* call sequence error (e.g. scoring before tfidf build) */
    SS_ERR_UNSUPPORTED = 7,  /* e.g. k > SS_MAX_TOPK, k_topics > SS_MAX_TOPICS */
    SS_ERR_COMM = 8          /* RCCL error (text in ss_last_error) */
};

#define SS_MAX_TOPK 1024     /* largest k accepted by ss_score_topk */
#define SS_MAX_TOPICS 64     /* largest k_topics accepted by every entry point (also by the opt-in two-vector form, "pr.affine") */
#define SS_MAX_QUERY_TERMS 64
#define SS_MAX_CONSTRAINT_TERMS 16   /* required + excluded terms per query, after de-duplication (ss_score_topk_constrained) */
#define SS_UNKNOWN_TERM 0xFFFFFFFFu /* term id for "key not found" (main_retrieve.go:193,218) */

typedef struct ss_ctx ss_ctx;
typedef struct ss_graph ss_graph;
typedef struct ss_pr ss_pr;
typedef struct ss_index ss_index;
typedef struct ss_scorer ss_scorer;

/* Result row.  The Go shim maps it into retrieval.Rank_combined
 * (retrieval/util.go:25-36: PageRank, FinalRank) and decorates only the k
 * winners with DocInfo/summary (get_metadata.go:79-235 stays host-side Go). */
typedef struct ss_hit {
    uint32_t doc;      /* dense doc id assigned by the shim (md5-hex docHash <-> id) */
    uint32_t _pad;
    double title;      /* TitleRank after cosine normalisation, get_metadata.go:58,64-66 */
    double body;       /* BodyRank  after cosine normalisation, get_metadata.go:57,61-63 */
    double pagerank;   /* sqd, get_metadata.go:39-42,68 */
    double final;      /* FinalRank, get_metadata.go:69 */
} ss_hit;

typedef struct ss_graph_info {
    uint64_t n_nodes, n_edges;
    uint64_t n_nondangling;      /* nodes with out-degree > 0 */
    uint64_t n_rows_local;       /* destination rows owned by this rank */
    uint64_t n_edges_local;      /* in-edges of those rows */
    uint32_t max_indeg;
    int32_t rank, world;
} ss_graph_info;

/* ---- context ---------------------------------------------------------- */
int32_t ss_abi_version(void);
int32_t ss_init(int32_t device_id, ss_ctx** out);
int32_t ss_shutdown(ss_ctx* ctx);
/* Use the caller's HIP stream (e.g. torch's current stream) for all work of this ctx.
 * NULL = the library's own non-blocking stream (default).  DEVICE pointers passed to any entry
 * point must hold their final contents with respect to the ctx stream: share the producer's
 * stream here, or synchronise the producer first.  Host pointers need nothing. */
int32_t ss_set_stream(ss_ctx* ctx, void* hip_stream);
int32_t ss_synchronize(ss_ctx* ctx);
/* Tuning and diagnostic switches of one context (no reference counterpart; nothing reads the environment).  The
 * defaults are the measured best; tests use the switches to reach kernel variants that the defaults would not pick
 * at test sizes ("pr.force_narrow", "tfidf.bucket_min", "score.exact_all", "score.separate_merge"), experiments to
 * sweep a parameter.  Unknown names are SS_ERR_INVALID; SS_OPTION_DEFAULT restores the default.  An option is read
 * when the object it concerns is created or the call it concerns is made.
 * "score.pipeline" (default 2 internal streams; 0 = every scoring kernel on the context's stream): ss_score_topk calls whose outputs
 * are device buffers run their scoring kernel on an internal stream and only the per-query merge — the kernel that writes the
 * hits — on the context's stream, behind an event: the next batch's scoring starts under this batch's merge and tail.  Batches of
 * the wave kernel since round 4; batches that are all k_score_slices (short lists, many terms, quoted phrases) too unless
 * "score.pipeline_slices" = 0.  Nothing changes for the caller: the hits are complete in the order of the context's stream,
 * and a consumer enqueued between two calls sees the first call's hits. */
#define SS_OPTION_DEFAULT INT64_MIN
int32_t ss_set_option(ss_ctx* ctx, const char* name, int64_t value);
const char* ss_last_error(ss_ctx* ctx); /* ctx may be NULL: last global error */

/* ---- multi-GPU: one context (= one GPU) per rank, collectives inside the library (RCCL over xGMI) -----------
 * The reference has no distributed code; this is what parallelises the TODO at ranking/pagerank.go:52 across GPUs.
 * Rank 0 makes the 128-byte id and hands it to every rank by any channel the host has (file, pipe, environment);
 * every rank then joins with its own context.  ss_comm_init blocks until all `world` ranks have called it.  One
 * process per GPU is the intended shape; a process holding several contexts calls ss_comm_init for each from its
 * own thread.  Collectives run on the context's stream. */
#define SS_COMM_ID_BYTES 128
int32_t ss_comm_unique_id(void* id_out /*[SS_COMM_ID_BYTES]*/);
int32_t ss_comm_init(ss_ctx* ctx, const void* id /*[SS_COMM_ID_BYTES]*/, int32_t rank, int32_t world);
/* 2-D decomposition (topic groups x doc shards): split the ranks into groups by color, renumbered by key inside a group; the
 * context's communicator becomes the group's.  A host with 8 GPUs and 16 topics can then run two groups of four doc shards,
 * each on 8 topics: a rank receives 3/4 of HALF the contribution table per sweep instead of 7/8 of all of it.
 *   ss_comm_split(ctx, rank / 4, rank % 4); ss_graph_create(..., rank % 4, 4); ss_pagerank_run_sharded(g, ..., 8, n_topic + 8 * (rank / 4), ...) */
int32_t ss_comm_split(ss_ctx* ctx, int32_t color, int32_t key);
int32_t ss_comm_destroy(ss_ctx* ctx);
int32_t ss_comm_info(ss_ctx* ctx, int32_t* rank_out /* -1: no communicator */, int32_t* world_out);
/* The exchange steps of the index side: whole-corpus document frequencies = all-reduce(sum) of the
 * shards' list lengths (feed the result to ss_index_set_doc_freq); corpus top-k = all-gather of the shards' hit
 * lists (feed the result to ss_merge_hits).  Host or device buffers; recv holds world * bytes_per_rank, rank order.
 * With host buffers the call returns when the result is there; with device buffers it only enqueues. */
int32_t ss_comm_allreduce_u64(ss_ctx* ctx, uint64_t* buf, uint64_t n);
int32_t ss_comm_allgather(ss_ctx* ctx, const void* send, void* recv, uint64_t bytes_per_rank);

/* ---- link graph: ranking/pagerank.go:17-44 ---------------------------- */
/* Graph as the reference holds it: forw[2] rows parent -> children, flattened
 * to an out-edge CSR over dense ids (node set = parents U children, Q1;
 * frontier pages are nodes with out-degree 0).  The library builds its own
 * HBM layout (in-edge lists, degree-binned row order, non-dangling-first
 * numbering) on the device.  rank/world: this process owns the destination
 * rows of shard `rank` of `world` (doc-range sharding);
 * single GPU = (0, 1).  The input arrays (host or device memory) have been
 * read when the call returns; the last kernels of the layout build may still
 * be running on the context's stream — everything else that touches the
 * graph is ordered behind them there (ss_synchronize to time the build;
 * option "graph.late_free" = 0 makes the call wait itself). */
int32_t ss_graph_create(ss_ctx* ctx, uint64_t n_nodes, uint64_t n_edges,
                        const uint64_t* out_ptr /*[n_nodes+1]*/, const uint32_t* out_dst /*[n_edges]*/,
                        int32_t rank, int32_t world, ss_graph** out);
/* Incremental update of the resident link graph (indexer/indexer.go:302: re-indexing a changed page rewrites
 * its forw[2] row, and setInverted :350-408 may add child pages never seen before).  The child lists of the `changed`
 * parents (distinct node ids) are replaced by new_children[new_ptr[i] .. new_ptr[i+1]); n_nodes_new >= n_nodes admits new
 * nodes (ids n_nodes .. n_nodes_new-1: new children, or new parents when they are in `changed`).  The library keeps the
 * adjacency resident, patches it on the device and rebuilds its layout from it: no upload of the unchanged rows.  The result
 * is the graph ss_graph_create would build from the updated rows (same layout, bit-identical PageRank).  No PageRank state
 * may exist on the graph; on an error the graph is unchanged. */
int32_t ss_graph_apply_delta(ss_graph* g, uint64_t n_nodes_new, uint64_t n_changed, const uint32_t* changed /*[n_changed]*/,
                             const uint64_t* new_ptr /*[n_changed+1]*/, const uint32_t* new_children);
int32_t ss_graph_get_info(const ss_graph* g, ss_graph_info* info);
int32_t ss_graph_destroy(ss_graph* g);

/* Links of a hit: the best parents ("linked from") and children ("links to") of a page, and how many it has.  The reference's result
 * card carries both (Rank_combined.Parents / .Children, retrieval/util.go:25-36): resultFormat (util.go:56-92) takes the first five
 * stored children and the first five parents of a Go map iteration — a different five on every request — and resolves each to a URL
 * (get_metadata.go:224-292).  Here the five are the BEST five by a per-node key the caller registers (one topic's PageRank row, say),
 * read from the graph that is resident for PageRank anyway; resolving ids to URLs stays host work.  Defined bit for bit:
 *   Key.        ss_graph_set_link_key registers key [n_nodes] float64 (host or device memory, copied: 8 bytes per node); NULL clears.
 *               It lives until it is replaced or cleared, until ss_graph_apply_delta SUCCEEDS (the node count may change; a failed
 *               delta leaves it) and until the graph is destroyed.  It may be set while PageRank states exist on the graph and is
 *               independent of them.
 *   Edges.      The children edges of node v are out_dst[out_ptr[v] .. out_ptr[v+1]) of the graph as it stands (as created, or as last
 *               patched by ss_graph_apply_delta); the parent edges of v are one entry u per edge u -> v.  Duplicate edges and
 *               self-loops are edges like any other.
 *   degree.     The number of edges of the row, duplicates counted, saturated at 2^32 - 1.
 *   Candidates. The DISTINCT node ids among the row's edges (a self-loop makes v a candidate of its own row).
 *   Order.      With a key: key[u] descending as float64 VALUES (-0.0 and +0.0 are equal), then ascending node id; NaN keys last,
 *               among themselves by id — the convention of ss_related_terms.  Without a key: ascending node id.
 *   Output.     Row i of links_out [n][m] holds the first n_out[i] = min(m, #candidates) candidates in that order; entries past
 *               n_out[i] are left untouched.  degree_out (nullable) is written for every row that is written.
 *   Nothing.    A node id >= n_nodes gives n_out = 0 and degree = 0, both written: defined, not an error, in both calls and whether
 *               the ids are host or device memory; no id makes a kernel read outside the graph.
 *   Hits form.  ss_graph_hit_links: entry (q, j) describes hits[q * k + j].doc taken as a node id.  Of a hit only .doc is read, and
 *               n_hits[q]; entries with j >= n_hits[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle, a NULL required pointer with n or n_q above 0,
 * dir not SS_LINKS_PARENTS / SS_LINKS_CHILDREN, m < 1, k < 1, n_q < 0: SS_ERR_INVALID; m > SS_MAX_LINKS, k > SS_MAX_TOPK, n * m or
 * n_q * k * m >= 2^31, or a graph that is not (rank 0, world 1) — a shard holds only its own rows' in-edges; requires a (0,1) graph
 * like ss_pagerank_run: SS_ERR_UNSUPPORTED; n_hits[q] outside [0, k]: SS_ERR_INVALID when n_hits is host memory, clamped by the
 * kernel when it is device memory.  n == 0 or n_q == 0 is SS_OK and does nothing.
 * Every pointer may be host or device memory.  When all given pointers are device memory the calls only enqueue on the ctx stream and
 * NEVER wait, so ss_graph_hit_links can sit behind ss_best_passages; otherwise they stage through blocks the graph owns and return
 * when the outputs are written.  One exception: the temporaries are sized from the largest degree of the direction, and the largest
 * OUT-degree is not on the host after ss_graph_create (max_indeg is).  The first call for SS_LINKS_CHILDREN on a graph computes it on
 * the device and waits for it, once; the value is kept until ss_graph_apply_delta succeeds.
 * Rows longer than option "links.wave_max" (default 1024, 32 .. 4096) are cut into chunks of option "links.chunk_edges" (default 1024,
 * 32 .. 4096) edges that are selected independently and then merged: the same bytes for every value.  The temporaries hold
 * n * m * ceil(largest degree / chunk) ids; SS_ERR_OOM if that memory cannot be had.  No copy of the edges is made.
 * Serialised on the ctx like the scoring calls; no _submit / _collect form. */
#define SS_MAX_LINKS      64
#define SS_LINKS_PARENTS  0
#define SS_LINKS_CHILDREN 1
int32_t ss_graph_set_link_key(ss_graph* g, const double* key /*[n_nodes], NULL clears*/);
int32_t ss_graph_top_links(ss_graph* g, int32_t dir, uint64_t n, const uint32_t* nodes /*[n]*/, int32_t m,
                           uint32_t* links_out /*[n][m]*/, int32_t* n_out /*[n]*/, uint32_t* degree_out /*[n] nullable*/);
int32_t ss_graph_hit_links(ss_graph* g, int32_t dir, int32_t n_q, int32_t k,
                           const ss_hit* hits /*[n_q][k]*/, const int32_t* n_hits /*[n_q]*/, int32_t m,
                           uint32_t* links_out /*[n_q][k][m]*/, int32_t* n_out /*[n_q][k]*/,
                           uint32_t* degree_out /*[n_q][k] nullable*/);

/* ---- PageRank: ranking/pagerank.go:14-145 ------------------------------ */
/* One call = the whole of UpdateTopicSensitivePagerank's compute: all k_topics
 * power iterations (pagerank.go:54-63 runs them sequentially; here they run as
 * one K-wide sweep per iteration), device-resident loop incl. the stop rule
 * (pagerank.go:93,115-119).  n_topic[k] = int(numPages) of category k.
 * eps < 0 never converges (fixed-iteration benchmarking); max_iter = 0 means
 * unbounded.  rank_out [k_topics][n_nodes] topic-major, original ids;
 * iters_out [k_topics].  Requires a (0,1) graph. */
int32_t ss_pagerank_run(ss_graph* g, double damping, double eps, int32_t max_iter,
                        int32_t k_topics, const int32_t* n_topic,
                        double* rank_out, int32_t* iters_out);

/* Step-wise form of the same loop, for multi-GPU hosts (one process per GPU;
 * the host owns the collective, e.g. torch.distributed/RCCL) and for timing.
 *   ss_pr_create   : allocate state for k_topics vectors on this rank's rows
 *   ss_pr_begin    : x0 = 1/n_topic (pagerank.go:103-106) + first contributions
 *   ss_pr_step     : one K-wide sweep over the local rows (computeRankInherited
 *                    :126-145 as a pull SpMV + fused normalise/delta :115-119)
 *   ss_pr_finalize : combine per-rank partial sums, apply the stop rule.
 *                    world==1: folded into begin/step, must not be called.
 *   exchange       : world>1: after begin/step either ss_pr_exchange (RCCL inside the library) or the host
 *                    all-gathers `send` (send_bytes from every rank, rank order) into `recv` itself,
 *                    then ss_pr_finalize.
 * All calls enqueue on the ctx stream and return without waiting, except
 * ss_pr_status / ss_pr_read_*.
 */
int32_t ss_pr_create(ss_graph* g, double damping, double eps, int32_t max_iter,
                     int32_t k_topics, const int32_t* n_topic, ss_pr** out);
int32_t ss_pr_destroy(ss_pr* pr);
/* OPT-IN, beyond what the reference executes: true topic-sensitive PageRank.  The reference advertises
 * Haveliwala's TSPR (README.md:9) but its topics differ only by the start value 1/numPages (pagerank.go:54-63,104): every
 * node teleports with the absolute (1-d) (pagerank.go:117).  With a teleport set per topic — set_ptr[k_topics+1] into
 * set_nodes (DISTINCT original node ids; an empty set keeps that topic on the reference's uniform teleport) — topic k's
 * teleport mass (1-d)*N is spread over its set only: cur[v] = (cur[v] + (v in set_k ? (1-d)*N/|set_k| : 0)) / total,
 * everything else (total, stop rule, start value) as in the reference.  Call after ss_pr_create, before ss_pr_begin;
 * NULL restores the reference behaviour.  Sharded graphs: every rank passes the full sets. */
int32_t ss_pr_set_teleport(ss_pr* pr, const uint64_t* set_ptr /*[k_topics+1]*/, const uint32_t* set_nodes);
int32_t ss_pr_begin(ss_pr* pr);
int32_t ss_pr_step(ss_pr* pr, int32_t n_steps);
/* Diagnostic: sweeps of this state launched in the lean form so far (option "pr.lean_sweeps", default on).  A state in
 * fixed-iteration mode (eps < 0) on one rank, K >= 3, without teleport sets runs every sweep of an ss_pr_step call except the last
 * two without loading or storing ranks; ranks, status and iteration counts behind the call are those of full sweeps. */
int32_t ss_pr_lean_sweeps(ss_pr* pr, int64_t* n_out);
int32_t ss_pr_finalize(ss_pr* pr);
int32_t ss_pr_exchange_buffers(ss_pr* pr, void** send_dev, uint64_t* send_bytes,
                               void** recv_dev, uint64_t* recv_bytes);
/* world>1, in-library exchange (needs ss_comm_init with the graph's rank/world): all-gather of the ranks' contribution
 * slices into the full table on the context's stream — the per-iteration collective of the doc-range-sharded sweep.
 * allreduce = 0: all-gather of the non-dangling slices (0.32*N*K*8 bytes received per rank and sweep at the benchmark
 * graph); allreduce = 1: the form the north star names — every rank contributes its slice inside a zeroed full-size
 * table and the tables are summed (all-reduce, ~2x the bytes on the wire, bit-identical result: x + 0 is exact).
 * Call between ss_pr_begin/ss_pr_step and ss_pr_finalize.  Enqueues only. */
int32_t ss_pr_exchange(ss_pr* pr, int32_t allreduce);
/* The whole sharded power iteration of one rank: begin, {sweep, exchange, finalize} until the device-side stop rule
 * (pagerank.go:93) has fired for every topic on every rank (the ranks agree: they finalize the same gathered sums).
 * The K topic vectors run as topic blocks (option "pr.topic_blocks", default 2 above 8 topics) whose exchanges are
 * enqueued on a second stream of the context: block b's collective overlaps block b+1's sweep.
 * Topics are independent, so the results are those of running every block's topics on their own.
 * ids_out [n_rows_local] original node ids of this rank's rows, rank_out [k_topics][n_rows_local], iters_out [k_topics].
 * Every rank writes its own rows of forw[3]; no gather of the result is needed.  k_topics <= 16 per call. */
int32_t ss_pagerank_run_sharded(ss_graph* g, double damping, double eps, int32_t max_iter, int32_t k_topics,
                                const int32_t* n_topic, int32_t allreduce, uint32_t* ids_out, double* rank_out, int32_t* iters_out);
/* The same pipeline for the shards of ONE process: shards[s] = shard s of `world` of the same graph, all on one context
 * (one device); the all-gather is played by device-to-device copies on the context's second stream.  Tests run the
 * topic-blocked, overlapped schedule through this on one GPU (RCCL refuses two ranks on one device), and a host that wants
 * several shards on one device can use it as it is.  rank_out [k_topics][n_nodes] in original ids (host memory). */
int32_t ss_pagerank_run_group(ss_graph* const* shards, int32_t world, double damping, double eps, int32_t max_iter, int32_t k_topics,
                              const int32_t* n_topic, double* rank_out, int32_t* iters_out);
/* Waits for the stream; iters_out[k_topics] = iterations executed per topic,
 * *n_active = topics still iterating, *sweeps = K-wide sweeps executed. */
int32_t ss_pr_status(ss_pr* pr, int32_t* iters_out, int32_t* n_active, int32_t* sweeps,
                     double* last_delta_out /*[k_topics] nullable*/, double* last_total_out /*[k_topics] nullable*/);
/* Local rows of this rank: ids_out[n_rows_local] original node ids,
 * rank_out[k_topics][n_rows_local]. */
int32_t ss_pr_read_local(ss_pr* pr, uint32_t* ids_out, double* rank_out);
/* world==1 only: rank_out[k_topics][n_nodes] in original id order. */
int32_t ss_pr_read(ss_pr* pr, double* rank_out);

/* Diagnostic (bench.py roofline.gather_ceiling_ms; no reference counterpart): average milliseconds of a gather-ONLY
 * pass over this state's in-edge stream and contribution table with the sweep's own load shape — what the access
 * pattern of computeRankInherited (pagerank.go:126-145) costs on this chip with every other part of the sweep
 * removed.  mode 0 = the graph's index stream, 1 = uniformly random rows (no hub reuse), 2 = consecutive rows;
 * + 8 * p selects the cache policy of the gathers (p = 0 default, 1 non-temporal, 2 sc1, 3 / 4 default for the rows
 * below SS_PR_PROBE_HOT and non-temporal / sc1 for the others: tools/pr_probe_pol.py).  States that run the 8- or
 * 16-wide sweep only. */
int32_t ss_pr_probe(ss_pr* pr, int32_t mode, int32_t n_reps, float* ms_out);

/* ---- inverted index + TF-IDF: ranking/term_weighting.go:10-123 --------- */
/* One inverted table (inv[0] title or inv[1] body), term-major CSR over dense
 * term/doc ids; post_tf = listPos[0] (normalised tf, indexer.go:362).  Each
 * term's postings must be strictly ascending by doc id (SS_ERR_UNSORTED). */
int32_t ss_index_create(ss_ctx* ctx, uint64_t n_docs, uint64_t n_terms,
                        const uint64_t* term_ptr /*[n_terms+1]*/, const uint32_t* post_doc,
                        const float* post_tf, ss_index** out);
int32_t ss_index_destroy(ss_index* idx);
/* UpdateTermWeights: idf = float32(log2(total_docs/df)) (:37), w = tf*idf in
 * place (:42), mag[doc] = sqrt(sum float64(float32(w*w))) (:44,:72).
 * total_docs = len(forw[3]) = number of PageRank nodes (:13-17, Q7).
 * w_out [P] / mag_out [n_docs] / idf_out [n_terms] nullable (the shim writes
 * them back to inv[*] / forw[4]).  Not idempotent, like the reference. */
int32_t ss_tfidf_build(ss_index* idx, uint64_t total_docs,
                       float* w_out, double* mag_out, float* idf_out);
/* Doc-range sharding (one shard of the table per GPU): a term's list here is only the
 * slice of its postings that falls into this shard's doc range, but len(docs) in
 * term_weighting.go:37 is the length of the WHOLE list.  df [n_terms] = whole-corpus document
 * frequencies (the host sums the shards' list lengths, one all-reduce); call before
 * ss_tfidf_build.  NULL restores df = local list length.  A doc's postings all live in its own
 * shard, so magnitudes need no exchange. */
int32_t ss_index_set_doc_freq(ss_index* idx, const uint64_t* df /*[n_terms]*/);
/* Load precomputed weights/magnitudes instead (tables already weighted). */
int32_t ss_index_set_weighted(ss_index* idx, const double* mag /*[n_docs]*/);
/* Positional postings for phrase search: listPos[1:] of every posting (parser/parser.go:195-207:
 * float32 positions, -100 for anchor/meta text), pos_ptr[n_postings+1] into pos[]. */
int32_t ss_index_set_positions(ss_index* idx, const uint64_t* pos_ptr, const float* pos);

/* Incremental update of a resident table (indexer/indexer.go:420-641 checkAndUpdate and the re-index
 * that follows it): every posting of del_docs goes (the changed page's old title/body words, :455-531), the single
 * postings (del_term[i], del_doc[i]) go (anchor words of the page's children in inv[0], :533-616; a pair that is not
 * there is ignored like Go's delete on a missing key), the postings (add_term[i], add_doc[i], add_w[i]) arrive (the
 * re-indexed page; a pair must not exist unless this delta deletes it).  The delta is merged into the resident CSR on
 * the device — no re-flatten, no re-upload — and every list is re-validated to be strictly ascending by doc; on any
 * error the table is unchanged.  Weights are taken as given (the reference stores whatever listPos[0] holds).
 * Magnitudes: when the table's squared magnitudes are resident (after ss_tfidf_build or ss_index_refresh_magnitudes), the
 * delta brings the magnitudes of the docs it touches (deleted docs, docs of deleted pairs, docs of new postings) up to date
 * itself: their squares are summed AGAIN from the merged table, in ascending term order — the order in which
 * term_weighting.go:29-46 reaches a doc — so they are what a full pass over the updated table gives, bit for bit, for any
 * weights (idf = log2(N/df) with N the PageRank node count can be 20, 1e-5 or negative: squares dozens of binary orders
 * apart, which a "subtract what left" patch would not survive); a doc left without postings has magnitude exactly 0;
 * ss_index_read_magnitudes reads them back for the forw[4] rows.  After ss_index_set_weighted (magnitudes given from outside) they are NOT touched: call
 * ss_index_refresh_magnitudes.  Positional postings: kept postings keep theirs; ss_index_apply_delta gives the new postings
 * empty position lists, ss_index_apply_delta_pos takes theirs (add_pos_ptr[n_add+1] into add_pos, in the order of the add
 * arrays; parser.go:195-207).  Doc and term ids must exist: grow the table first (ss_index_resize) when a re-indexed page
 * brings new words or new child pages (indexer.go:350-408).  Scorers on this table must be destroyed before and created
 * again after. */
int32_t ss_index_apply_delta(ss_index* idx, uint64_t n_del_docs, const uint32_t* del_docs,
                             uint64_t n_del, const uint32_t* del_term, const uint32_t* del_doc,
                             uint64_t n_add, const uint32_t* add_term, const uint32_t* add_doc, const float* add_w);
int32_t ss_index_apply_delta_pos(ss_index* idx, uint64_t n_del_docs, const uint32_t* del_docs,
                                 uint64_t n_del, const uint32_t* del_term, const uint32_t* del_doc,
                                 uint64_t n_add, const uint32_t* add_term, const uint32_t* add_doc, const float* add_w,
                                 const uint64_t* add_pos_ptr /*[n_add+1] nullable*/, const float* add_pos);
/* Grow the doc and / or term space of a resident table (new docs have no postings and magnitude 0, new terms empty lists). */
int32_t ss_index_resize(ss_index* idx, uint64_t n_docs_new, uint64_t n_terms_new);
/* mag_out[i] = magnitude of docs[i] as it stands (host or device arrays). */
int32_t ss_index_read_magnitudes(ss_index* idx, uint64_t n, const uint32_t* docs, double* mag_out);
/* mag[doc] = sqrt(sum float64(float32(w*w))) over the table's CURRENT weights (term_weighting.go:44,72), without the
 * idf multiplication of ss_tfidf_build.  mag_out [n_docs] nullable. */
int32_t ss_index_refresh_magnitudes(ss_index* idx, double* mag_out);
/* The table as it stands (after updates): sizes, then the arrays (each nullable; host or device). */
int32_t ss_index_get_info(const ss_index* idx, uint64_t* n_docs, uint64_t* n_terms, uint64_t* n_post);
int32_t ss_index_read(ss_index* idx, uint64_t* term_ptr_out /*[n_terms+1]*/, uint32_t* post_doc_out, float* post_w_out);
/* the positional postings as they stand (each nullable): pos_ptr_out [n_post+1], pos_out [pos_ptr[n_post]] */
int32_t ss_index_read_positions(ss_index* idx, uint64_t* pos_ptr_out, float* pos_out);

/* Doc-major view of a table: which terms does doc d hold?  (The tables are term-major; the reference keeps a page's words on the Go
 * side, Words_mapping, cut to the five heaviest by sortMap, retrieval/util.go:116-149, and walks a page's old words to delete
 * its postings, indexer.go:494-531.)  The view holds doc_ptr u64[n_docs+1] | doc_term u32[n_post] | doc_w f32[n_post]: row d =
 * doc_term / doc_w [doc_ptr[d] .. doc_ptr[d+1]) lists the terms that have a posting of d in ASCENDING TERM ID, each with the
 * posting's weight as it stands when the view is built (tf before ss_tfidf_build, tf*idf after).  It is a snapshot and a pure
 * function of the table: two builds give identical bytes.  Resident size 8 bytes per posting + 8 per doc; the build needs about
 * as much again for its temporaries, which are freed before the call returns.  Building where a view exists replaces it: the old
 * view is freed FIRST (so that the peak does not grow by another 8 bytes per posting), and a build that fails (SS_ERR_OOM,
 * SS_ERR_HIP) leaves the table WITHOUT a view, not with the old one.
 * Every call that changes postings or weights frees the view: ss_tfidf_build, ss_index_apply_delta(_pos), ss_index_resize (and
 * ss_index_destroy); ss_index_set_weighted and ss_index_set_doc_freq change neither and leave it.  Without a view
 * ss_index_drop_doc_view, ss_index_read_doc_view, ss_index_doc_top_terms, ss_similar_topk and ss_related_terms return SS_ERR_STATE.
 * A table of 2^32 postings or more is SS_ERR_UNSUPPORTED (the build indexes postings with 32 bits).  The calls wait for their
 * work: the view is complete, and host outputs are there, when they return. */
int32_t ss_index_build_doc_view(ss_index* idx);
int32_t ss_index_drop_doc_view(ss_index* idx);
/* the view as it stands: doc_ptr_out [n_docs+1], doc_term_out [n_post], doc_w_out [n_post], each nullable, host or device */
int32_t ss_index_read_doc_view(ss_index* idx, uint64_t* doc_ptr_out, uint32_t* doc_term_out, float* doc_w_out);
/* The heaviest terms of docs[0 .. n): row i of terms_out [n][m] / w_out [n][m] (nullable) holds the first n_out[i] = min(m, row
 * length) entries of docs[i]'s view row in the order: weight descending as float32 VALUES (-0.0 and +0.0 are equal), then
 * ascending term id; NaN weights last, among themselves by term id.  Selection and copying only: the weights are the stored
 * bits.  Entries past n_out[i] are left untouched.  1 <= m <= SS_MAX_QUERY_TERMS and every doc id < n_docs, else SS_ERR_INVALID
 * before anything is enqueued; a doc may appear more than once.  Pointers host or device. */
int32_t ss_index_doc_top_terms(ss_index* idx, uint64_t n, const uint32_t* docs /*[n]*/, int32_t m,
                               uint32_t* terms_out /*[n][m]*/, float* w_out /*[n][m] nullable*/, int32_t* n_out /*[n]*/);

/* ---- scoring: retrieval/main_retrieve.go:50-103, get_metadata.go:31-69 -- */
int32_t ss_scorer_create(ss_ctx* ctx, ss_index* title, ss_index* body, ss_scorer** out);
int32_t ss_scorer_destroy(ss_scorer* s);
/* forw[3] ranks for the PageRank blend (get_metadata.go:31-42):
 * rank [k_topics][n_docs] topic-major (ss_pagerank_run's layout). k_topics=0 clears. */
int32_t ss_scorer_set_prior(ss_scorer* s, int32_t k_topics, const double* rank);
/* Batch of OR queries.  q_ptr[n_q+1] into q_terms (term ids in query order,
 * duplicates kept, SS_UNKNOWN_TERM for unknown words); query_len[n_q]
 * (len(queryTokenised)+len(phraseTokenised), main_retrieve.go:90; NULL = term
 * count); topic_probs [n_q][k_topics] or NULL (nil map => sqd = 0,
 * main_retrieve.go:88).  hits_out [n_q][k], n_hits_out [n_q] (host or device).
 * Order: FinalRank descending (util.go:48-54), ties ascending doc id, NaN last;
 * reference k = 50 (main_retrieve.go:99-100).
 * The QUERY arrays (q_ptr, q_terms, query_len, topic_probs, and p_ptr / p_terms below) are consumed on the HOST: the
 * slice plan of a batch (which lists, which doc ranges, which kernel) is made on the CPU from the host copy of the
 * tables' term_ptr, as the query words themselves arrive from a host-side tokenizer (main_retrieve.go:17-36).  Pass host
 * arrays; device pointers are accepted and cost one blocking copy back each (~16 KB for 1024 queries).
 * Results in HOST memory: the call returns when they are there.  Results in DEVICE memory (both
 * pointers): the kernels write them directly and the call returns once the work is enqueued on the
 * ctx stream — later work on that stream sees them; ss_synchronize waits for them. */
int32_t ss_score_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                      const int32_t* query_len, const double* topic_probs, int32_t k,
                      ss_hit* hits_out, int32_t* n_hits_out);

/* The same batch with results in HOST memory and several batches in flight (a server that has the next batch of requests
 * ready while this one runs): ss_score_topk_submit enqueues the batch into device buffers that belong to the ticket, records an event
 * behind its kernels and returns the ticket (never 0) without waiting; ss_score_topk_collect waits for THAT batch's event, copies the
 * rows to the caller (a plain device-to-host copy at collect time; option "score.collect_pinned" = 1 stages it through pinned
 * memory) and writes hits_out [n_q][k],
 * n_hits_out [n_q] (host memory, the n_q and k of the submit).  Up to SS_SCORE_INFLIGHT tickets may be outstanding
 * (SS_ERR_STATE beyond); collect them in any order.  The host's plan for batch i+1 and its copy-out of batch i-1 run under the
 * kernels of batch i: 1024-query batches go host-to-host at the device's batch rate instead of one batch alone plus the copies. */
#define SS_SCORE_INFLIGHT 3
int32_t ss_score_topk_submit(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                             const uint32_t* p_ptr /* NULL: no quoted phrases (ss_score_topk); else as ss_score_topk_phrase */,
                             const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, int32_t k,
                             uint64_t* ticket_out);
int32_t ss_score_topk_collect(ss_scorer* s, uint64_t ticket, ss_hit* hits_out, int32_t* n_hits_out);

/* ss_score_topk plus the quoted-phrase part of retrieval.Retrieve (retrieval/phrase.go:11-170,
 * util.go:162-203, merged at main_retrieve.go:73-78).  p_ptr[n_q+1] into p_terms: the tokens of ALL quoted
 * phrases of a query, concatenated into one phrase as the reference does (main_retrieve.go:26); a doc
 * matches if it holds every phrase term (body or title) and, per field, the term positions shifted by
 * the term's index intersect; its float32 weight sums are added to TitleRank/BodyRank.  query_len NULL =
 * len(query tokens)+len(phrase tokens) (main_retrieve.go:90).  At most SS_MAX_PHRASE_TERMS per phrase.
 * Needs ss_index_set_positions on both tables. */
#define SS_MAX_PHRASE_TERMS 16
int32_t ss_score_topk_phrase(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                             const uint32_t* p_ptr, const uint32_t* p_terms, const int32_t* query_len,
                             const double* topic_probs, int32_t k, ss_hit* hits_out, int32_t* n_hits_out);

/* Doc masks: top-k over PART of the corpus ("results in category X only", "hide these pages").  No reference counterpart.
 * Register allow-lists on a scorer: words [n_masks][(n_docs+31)/32], bit (d & 31) of word d >> 5 = doc d allowed
 * (n_docs = the scorer's; bits past n_docs ignored).  Host or device memory, copied.  n_masks = 0 / NULL clears.
 * Replaces the previous set after the scorer's outstanding work (pipelined batches, tickets) has finished with it.
 * The masks live as long as the scorer: after an index update (destroy scorers before, re-create after) register them again. */
int32_t ss_scorer_set_doc_masks(ss_scorer* s, int32_t n_masks, const uint32_t* words);

/* ss_score_topk_phrase with a per-query allow-list: mask_id [n_q] (-1 = unrestricted; NULL = all -1), p_ptr NULL = no phrases.
 * Row q = the first min(k, m) rows of query q's unrestricted ranking (FinalRank desc, ties doc asc, NaN last)
 * restricted to the docs its mask allows -- NOT a post-filter of the unrestricted top-k.
 * Outputs as ss_score_topk (device outputs: the call only enqueues, pipelined like any other batch).  A mask_id below -1
 * or at / above n_masks is SS_ERR_INVALID and nothing is enqueued.  With no masked query the call IS ss_score_topk_phrase /
 * ss_score_topk (same kernels, bit-identical rows).  There is no masked form of ss_score_topk_submit / _collect. */
int32_t ss_score_topk_masked(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                             const uint32_t* p_ptr, const uint32_t* p_terms, const int32_t* query_len,
                             const double* topic_probs, const int32_t* mask_id, int32_t k,
                             ss_hit* hits_out, int32_t* n_hits_out);

/* Query operators: ss_score_topk_masked plus required ("+word") and excluded ("-word") terms per query.  No reference counterpart.
 * Doc d CONTAINS term t if d has a posting of t in the title or the body table (any weight, zero included).  Doc d is allowed for
 * query q iff d is in mask(q) (the allow-list mask_id[q], every doc for -1), contains every term of req_terms[req_ptr[q] ..
 * req_ptr[q+1]) and no term of exc_terms[exc_ptr[q] .. exc_ptr[q+1]).  Row q = the first min(k, m) rows of query q's unrestricted
 * ranking (FinalRank desc, ties doc asc, NaN last) restricted to its allowed docs: byte for byte what ss_score_topk_masked returns
 * with that allowed set registered as the query's allow-list.
 * Constraint terms only filter: they add nothing to the score, to query_len or to the candidates (a caller who wants "+foo" scored
 * too puts foo in q_terms as well).  A term id >= n_terms (SS_UNKNOWN_TERM included) has no postings: an unknown required term
 * leaves the row empty, an unknown excluded term does nothing; a term both required and excluded leaves the row empty; duplicates
 * change nothing.  req_ptr / exc_ptr [n_q+1] (NULL = none) start at 0 and never decrease, else SS_ERR_INVALID; more than
 * SS_MAX_CONSTRAINT_TERMS distinct required + excluded ids in one query is SS_ERR_UNSUPPORTED; a bad mask_id is SS_ERR_INVALID as
 * in ss_score_topk_masked.  Every check comes before anything is enqueued and leaves the outputs untouched.
 * Inputs are read on the host like the query arrays (device pointers cost one blocking copy each); outputs as ss_score_topk (device
 * outputs: the call only enqueues, pipelined like any other batch).  The allowed sets are built on the device for the call, one
 * per distinct (mask, required, excluded) combination: n_docs / 8 bytes each (1.25 MB at 10M docs), SS_ERR_OOM if that memory
 * cannot be had.  A call without a constraint IS ss_score_topk_masked (same kernels, bit-identical rows).
 * There is no constrained form of ss_score_topk_submit / _collect. */
int32_t ss_score_topk_constrained(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                                  const uint32_t* p_ptr, const uint32_t* p_terms, const int32_t* query_len,
                                  const double* topic_probs, const int32_t* mask_id,
                                  const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                                  const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                                  int32_t k, ss_hit* hits_out, int32_t* n_hits_out);

/* Similar pages: the heaviest body terms of a page as a new query.  No reference counterpart (the reference ships the material:
 * every Rank_combined carries the page's five heaviest words).  Query q = the ss_index_doc_top_terms row of seeds[q] (a doc id)
 * in the BODY table's view with this m, in that order; query_len = its term count.  R = the row ss_score_topk_masked returns for
 * that query with k + 1, topic_probs[q] and mask_id[q] (mask_id NULL: ss_score_topk).  Output row q = R without the hit whose doc
 * is seeds[q] if it is there, cut to k: n_hits = min(k, |R| - [seed in R]); a seed without body postings gives an empty row.
 * 1 <= k <= SS_MAX_TOPK - 1 (beyond: SS_ERR_UNSUPPORTED; k < 1 is SS_ERR_INVALID as in ss_score_topk), 1 <= m <=
 * SS_MAX_QUERY_TERMS, the body view must exist (SS_ERR_STATE), a seed >= n_docs or a bad mask_id is SS_ERR_INVALID: every check
 * comes before anything is enqueued and leaves the outputs untouched.  seeds / topic_probs / mask_id are read on the host like the
 * query arrays.  The call waits once, for the seeds' terms (the slice plan is made on the CPU); outputs as ss_score_topk: with
 * device outputs it returns once the rest is enqueued on the ctx stream.  There is no similar form of ss_score_topk_submit / _collect. */
int32_t ss_similar_topk(ss_scorer* s, int32_t n_q, const uint32_t* seeds /*[n_q] doc ids*/, int32_t m,
                        const double* topic_probs, const int32_t* mask_id /*NULL = none*/, int32_t k,
                        ss_hit* hits_out, int32_t* n_hits_out);

/* Related terms: which words do a query's best pages have in common that the user did not type?  No reference counterpart (the
 * reference ships the material per page, Words_mapping, retrieval/util.go:116-149; it never aggregates over a result list).  The
 * pseudo-relevance-feedback step behind "related searches" / "refine by" and the input of an expanded re-query.  Defined bit for bit:
 *   Hits.       R = the row ss_score_topk_masked returns for query q with k = k_fb, this query_len, topic_probs[q] and mask_id[q]
 *               (mask_id NULL: the ss_score_topk row).  There are no phrases.
 *   Per hit.    For hit j of R in rank order, T_j = the ss_index_doc_top_terms row of doc R[j].doc in the BODY table's view with
 *               m_doc: term ids and the stored float32 weights.  A hit without body postings contributes nothing.
 *   Candidates. Every term of some T_j whose id is not among q_terms[q_ptr[q] .. q_ptr[q+1]).
 *   Score.      score(t) = the float64 sum of (double)w_j(t) over the hits j with t in T_j, added in ASCENDING j, starting from 0.0.
 *               The order is part of the definition: stored weights can lie more than 29 binary orders apart, and then the last
 *               bit depends on it.  (A sum of -0.0 weights alone is +0.0: 0.0 + -0.0.)
 *   Output.     Row q of terms_out [n_q][m] / score_out [n_q][m] (nullable) holds the first n_out[q] = min(m, #candidates)
 *               candidates ordered by score descending as float64 VALUES (-0.0 and +0.0 are equal), then ascending term id; NaN
 *               scores last, among themselves by term id — the convention of ss_index_doc_top_terms, one width up.  score_out
 *               holds the sums' bits.  Entries past n_out[q] are left untouched.
 *   Empty rows. A query without hits gives an empty row; so does a query whose hits hold only query terms.
 * 1 <= k_fb <= SS_MAX_FEEDBACK_DOCS, 1 <= m_doc <= SS_MAX_QUERY_TERMS, 1 <= m <= SS_MAX_QUERY_TERMS, a bad mask_id: SS_ERR_INVALID;
 * no body view, or topic_probs without a prior: SS_ERR_STATE; a bad q_ptr as in ss_score_topk.  Every check comes before anything
 * is enqueued and leaves the outputs untouched.
 * The query arrays are read on the host like every scoring call's.  Outputs host or device memory: when terms_out, n_out and
 * score_out (if given) are all device memory the call only enqueues on the ctx stream and, unlike ss_similar_topk, NEVER waits —
 * hits, their docs' terms, the sums and the selection all stay on the device.  There is no _submit / _collect form. */
#define SS_MAX_FEEDBACK_DOCS 64
int32_t ss_related_terms(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                         const int32_t* query_len, const double* topic_probs, const int32_t* mask_id /*NULL = none*/,
                         int32_t k_fb, int32_t m_doc, int32_t m,
                         uint32_t* terms_out /*[n_q][m]*/, double* score_out /*[n_q][m] nullable*/, int32_t* n_out /*[n_q]*/);

/* Explain hits: which of the query's tokens matched each result row, with what stored weight, and where in the body.  The reference
 * cannot say (queries are a pure OR; to find a word it parses the cached HTML of every candidate, retrieval/get_metadata.go:79-209).
 * What a result card needs for bold matched words, a "Missing: word" line, a snippet anchored at the first occurrence and a
 * "why is this ranked here" view.  Defined bit for bit:
 *   Entries.    Entry (q, j, i) = out[(q * k + j) * t_stride + i] describes hit j of query q, hits[q * k + j], and the query's i-th
 *               TOKEN, q_terms[q_ptr[q] + i].  Token order is kept; duplicate tokens get identical entries.
 *   Written.    Only entries with j < n_hits[q] and i < q_ptr[q+1] - q_ptr[q] are written; all others are left untouched (the
 *               convention of ss_index_doc_top_terms and ss_related_terms).
 *   Read.       Of a hit only .doc is read, and n_hits[q].  The rows may come from any scoring call (ss_score_topk, _phrase, _masked,
 *               _constrained, ss_similar_topk, ss_merge_hits with local ids) or be made up by the caller.
 *   Flags.      Bit 0 is set iff the title table has a posting of the term for the doc, at any weight, zero included
 *               (ss_score_topk_constrained's "contains"); bit 1 the same for the body table.  title_w / body_w are the posting's
 *               stored float32 BITS (a -0.0 or a NaN comes back as it is): the flag, not the value, says "absent".
 *   Nothing.    A term id >= n_terms (SS_UNKNOWN_TERM included) has no postings, nor has a doc id >= n_docs: the entry is all zero.
 *               Defined, not an error; no hit, whatever it holds, makes the kernel read outside the tables.
 *   body_pos.   Bit 2 is set iff the body table has positional postings (ss_index_set_positions), the body posting exists and its
 *               position list holds at least one value v with v >= 0 (NaN compares false; so does -100, the marker of anchor / meta
 *               text, parser/parser.go:195-207).  body_pos is then the smallest such v as a float32 VALUE; a smallest value of zero
 *               comes back as +0.0 whichever zeros the list holds.  Lists need not be sorted.  An empty list, or one of negative or
 *               NaN values only, leaves bit 2 clear and body_pos +0.0.  Title positions are not reported.
 * Checks, all before anything is enqueued and with `out` untouched: NULL handle or out (or hits / n_hits with n_q > 0), n_q < 0,
 * k < 1, t_stride < 1, a bad q_ptr as in ss_score_topk, a query of more than t_stride tokens: SS_ERR_INVALID; k > SS_MAX_TOPK,
 * t_stride > SS_MAX_QUERY_TERMS or n_q * k * t_stride >= 2^31: SS_ERR_UNSUPPORTED; n_hits[q] outside [0, k]: SS_ERR_INVALID when
 * n_hits is host memory, clamped by the kernel when it is device memory.  n_q == 0 is SS_OK and does nothing.
 * q_ptr / q_terms are read on the host like every query array.  hits / n_hits / out may each be host or device memory: when all three
 * are device memory the call only enqueues on the ctx stream and NEVER waits, so it can sit right behind an ss_score_topk whose
 * outputs are device buffers; otherwise it stages through blocks the scorer owns and returns when out is written.
 * It reads the tables as they stand (scorers are destroyed before an index update and re-created after, as ever), is serialised on
 * the ctx like the other scoring calls, and has no _submit / _collect form. */
typedef struct ss_term_match {
    float    title_w;   /* stored weight bits of the title posting of (term, doc); +0.0 bits if there is none */
    float    body_w;    /* the same for the body table */
    uint32_t flags;     /* bit 0: a title posting exists; bit 1: a body posting exists; bit 2: body_pos is valid */
    float    body_pos;  /* see above; +0.0 bits when bit 2 is clear */
} ss_term_match;        /* 16 bytes */
int32_t ss_explain_hits(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                        int32_t k, const ss_hit* hits /*[n_q][k]*/, const int32_t* n_hits /*[n_q]*/,
                        int32_t t_stride, ss_term_match* out /*[n_q][k][t_stride]*/);

/* Best passage per hit: the body window of `width` word positions that covers most of the query's terms: the anchor of a result
 * card's snippet.  The reference's summary (retrieval/get_metadata.go:121-192) shows twenty words around the FIRST word that matches
 * any query token, found by parsing the cached HTML; ss_explain_hits' body_pos gives that anchor.  This call reads the body table's
 * positional postings (ss_index_set_positions; parser/parser.go:195-207: one float32 word index per occurrence, -100 for anchor and
 * meta text) and returns the BEST place instead of the first.  The host slices the cached words at [start, start + width).
 * Defined bit for bit.  Entry (q, j) = out[q * k + j] describes hit j of query q, doc d = hits[q * k + j].doc; of a hit only .doc
 * is read, and n_hits[q].
 *   Occurrences.  For each DISTINCT term id t among the query's tokens, each value v of the body position list of posting (t, d) with
 *                 v >= 0 is one occurrence (v, t); NaN and negative values (the -100 marker) compare false and are none.  Equal
 *                 values of a list count separately; lists need not be sorted.  There are no occurrences when the term id is
 *                 >= n_terms (SS_UNKNOWN_TERM included), d >= n_docs, the posting is missing or the body table has no positions:
 *                 defined, not an error; no hit, whatever it holds, makes the kernel read outside the tables.
 *   Window.       For every occurrence value p, W(p) is the set of occurrences (v, t) with v >= p and
 *                 (double)v < (double)p + (double)width, as that float64 expression evaluates (the window of p = +inf is empty).
 *                 Both zeros are equal.
 *   Best.         The window that maximises n_distinct (distinct term ids in it), then n_occ (occurrences in it), then has the smallest
 *                 p as a float value.  start = that p, a zero as +0.0; last = the largest v in the window; token_mask bit i is set
 *                 iff the term of the query's i-th token (token order as given) has an occurrence in the window: duplicate tokens
 *                 get equal bits.  (n_occ is counted modulo 2^32.)
 *   Written.      Every entry with j < n_hits[q] is written; a doc without occurrences, a query without tokens, or a best window
 *                 that is empty gives 24 zero bytes.  All other entries are left untouched.
 * Checks, all before anything is enqueued and with `out` untouched: NULL handle, out or q_ptr (or hits / n_hits with n_q > 0), n_q < 0,
 * k < 1, width < 1, a bad q_ptr as in ss_score_topk, n_hits[q] outside [0, k] when n_hits is host memory (device memory: clamped by
 * the kernel): SS_ERR_INVALID; k > SS_MAX_TOPK, width > 2^24, a query of more than SS_MAX_QUERY_TERMS tokens or n_q * k >= 2^31:
 * SS_ERR_UNSUPPORTED.  n_q == 0 is SS_OK and does nothing.
 * q_ptr / q_terms are read on the host like every query array.  hits / n_hits / out may each be host or device memory: when all three
 * are device memory the call only enqueues on the ctx stream and NEVER waits, so it chains behind score -> collapse -> explain;
 * otherwise it stages through blocks the scorer owns and returns when out is written.  Docs with more position values under the
 * query's terms than option "passage.lds_events" (default 512, 1 .. 4096) are answered from global memory instead of the LDS:
 * the same bytes, more slowly.  Serialised on the ctx like the other scoring calls; no _submit / _collect form; title positions
 * are not read. */
typedef struct ss_passage {
    float    start;       /* position value of the window's first occurrence; +0.0 bits when n_occ == 0 */
    float    last;        /* largest occurrence value inside the window; +0.0 bits when n_occ == 0 */
    uint32_t n_distinct;  /* distinct query TERM ids with an occurrence in the window */
    uint32_t n_occ;       /* occurrences in the window; 0 = the doc has no passage: all 24 bytes are zero */
    uint64_t token_mask;  /* bit i: the query's i-th token's term occurs in the window */
} ss_passage;             /* 24 bytes */
int32_t ss_best_passages(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                         int32_t k, const ss_hit* hits /*[n_q][k]*/, const int32_t* n_hits /*[n_q]*/,
                         int32_t width, ss_passage* out /*[n_q][k]*/);

/* Term proximity: per hit the smallest body span that holds every query term the doc has at all, and a window re-ranked by it.  The
 * reference's FinalRank (retrieval/get_metadata.go:57-69) is a pure OR: a page where the query stands as neighbouring words ranks like
 * one that holds the words in unrelated paragraphs.  ss_best_passages answers another question (a window of fixed width, for a snippet)
 * and re-orders nothing.  These calls read the same resident material, the body table's positional postings (ss_index_set_positions),
 * and need no other per-doc data.  No reference counterpart.
 * ss_hit_proximity.  Defined bit for bit.  Entry (q, j) = out[q * k + j] describes doc d = hits[q * k + j].doc; of a hit only .doc is read,
 * and n_hits[q].
 *   Occurrences.  As in ss_best_passages, except that +inf is none: for each DISTINCT term id t among the query's tokens, each value v
 *                 of the body position list of posting (t, d) with v >= 0 and v < +inf is one occurrence (v, t); NaN, negative values
 *                 (the -100 marker) and +inf are none.  Equal values count separately; lists need not be sorted; both zeros are
 *                 equal.  There are no occurrences when the term id is >= n_terms (SS_UNKNOWN_TERM included), d >= n_docs, the
 *                 posting is missing or the body table has no positions: defined, not an error; no row, whatever it holds, makes the
 *                 kernel read outside the tables.
 *   Present.      P = the distinct term ids with at least one occurrence; n_present = |P|; token_mask bit i is set iff the term of the
 *                 query's i-th token (token order as given) is in P: duplicate tokens get equal bits.
 *   Span.         Of all pairs of occurrence values a <= b such that every term of P has an occurrence with value in [a, b]: the pair
 *                 with the smallest (double)b - (double)a, as that float64 expression evaluates; of equal differences the one with the
 *                 smallest a as a float value; for that a the smallest such b.  start = a, end = b, a zero as +0.0; n_occ = the
 *                 occurrences with a <= v <= b (counted modulo 2^32).  With |P| = 1 the span is the smallest occurrence alone
 *                 (start == end).
 *   Written.      Every entry with j < n_hits[q] is written; n_present == 0 gives 24 zero bytes.  All other entries are left untouched.
 * Checks, staging, host / device pointers and the clamping of a device n_hits: exactly those of ss_best_passages without `width`.  Docs
 * with more position values under the query's terms than option "proximity.lds_events" (default 512, 1 .. 4096) are answered from
 * global memory instead of the LDS: the same bytes, more slowly.
 * ss_rerank_hits_by_proximity: a stable, paged re-rank in the family of ss_sort_hits_by_field and ss_rerank_hits_by_vector, so that
 * score -> dedup -> collapse -> proximity -> explain -> passages stays on one stream.  Defined bit for bit:
 *   Window.     As in ss_collapse_hits: hits[q * k_in .. q * k_in + n_hits[q]), in the order given.  Of a row .doc and .final are read;
 *               given rows are trusted, as in ss_fuse_hits.
 *   Score.      For a row with doc < n_docs let E be its ss_hit_proximity entry and T the number of distinct term ids among the
 *               query's tokens (SS_UNKNOWN_TERM counts as one id).  Every operation is rounded once, nothing is contracted:
 *                 sp    = (double)E.end - (double)E.start
 *                 prox  = E.n_present < 2 ? 0.0 : (double)(E.n_present - 1) / max(sp, (double)(E.n_present - 1))     (1.0: neighbours)
 *                 cover = T ? (double)E.n_present / (double)T : 0.0
 *                 bonus = prox * cover
 *                 score = w_rank * row.final + w_prox * bonus
 *   Order.      Score descending by numeric comparison (-0.0 ties 0.0); equal scores stay in window order (the sort is stable; the
 *               same doc twice is two rows); NaN scores come after every number, among themselves in window order; rows with
 *               doc >= n_docs come LAST of all, in window order.
 *   Output.     With the sorted rows S_0 .. S_{n-1}: hits_out[q * k + r] = the 40 bytes of S_{first + r} (_pad included) for
 *               r < n_hits_out[q] = clamp(n - first, 0, k); scores_out[q * k + r] (nullable) = that row's score, a NaN as
 *               0x7FF8000000000000, which a row with doc >= n_docs gets too; prox_out[q * k + r] (nullable) = E, 24 zero bytes for a
 *               row with doc >= n_docs.  Entries past n_hits_out[q] are left untouched.
 * So with w_prox == 0 and w_rank > 0, on rows in FinalRank order without NaN, the output is the window with its inside rows first; with
 * w_rank == 0 (and finite finals) the order is bonus descending, then window order.
 * Checks, all before anything is enqueued and with the outputs untouched: those of ss_rerank_hits_by_vector (hits_out overlapping
 * hits included; there is no table to register), those of ss_best_passages for the query arrays, w_rank or w_prox not finite:
 * SS_ERR_INVALID; a scratch for the window's entries that cannot be had: SS_ERR_OOM.  Every pointer but the query arrays may be host
 * or device memory: with every given array in device memory the call only enqueues on the ctx stream and NEVER waits.
 * ss_score_topk_proximity: row q = ss_rerank_hits_by_proximity applied to the row ss_score_topk_masked returns for query q with
 * k = k_window, this query_len, topic_probs[q] and mask_id[q].  Wired as ss_score_topk_collapsed is: the window stays inside the scorer
 * and only the page is written.  Checks: the re-rank's plus those of ss_score_topk_collapsed.  There is no phrase or constrained form:
 * those callers chain the re-rank.
 * A known answer.  Query tokens (A, B, C), T = 3.  Doc X: A {3, 40}, B {5, 41, 90}, C {43, -100}: start 40, end 43, n_present 3,
 * n_occ 3, token_mask 0b111; prox = 2 / max(3, 2) = 2.0 / 3.0, cover = 1.0.  Doc Y: A {7}, B {8}: start 7, end 8, n_present 2, n_occ 2,
 * token_mask 0b011; prox = 1.0, cover = 2.0 / 3.0: the same bonus bits as X.  Doc Z: A {10}: start 10, end 10, n_present 1, n_occ 1,
 * bonus 0.0.  Doc W: none of them: 24 zero bytes, bonus 0.0.  The window (W, Z, Y, X) with w_rank = 0, w_prox = 1 comes back as
 * Y, X, W, Z: X and Y tie and keep window order, and so do W and Z. */
typedef struct ss_proximity {
    float    start;       /* value of the span's first occurrence; +0.0 bits when n_present == 0 */
    float    end;         /* value of the span's last occurrence;  +0.0 bits when n_present == 0 */
    uint32_t n_present;   /* distinct query TERM ids with an occurrence in the doc's body; 0: all 24 bytes are zero */
    uint32_t n_occ;       /* occurrences with start <= value <= end (modulo 2^32) */
    uint64_t token_mask;  /* bit i: the query's i-th token's term is present */
} ss_proximity;           /* 24 bytes */
int32_t ss_hit_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                         int32_t k, const ss_hit* hits /*[n_q][k]*/, const int32_t* n_hits /*[n_q]*/,
                         ss_proximity* out /*[n_q][k]*/);
int32_t ss_rerank_hits_by_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                                    int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/,
                                    double w_rank, double w_prox, int32_t first, int32_t k,
                                    ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                                    double* scores_out /*[n_q][k], nullable*/, ss_proximity* prox_out /*[n_q][k], nullable*/);
int32_t ss_score_topk_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                                const int32_t* query_len, const double* topic_probs, const int32_t* mask_id /*NULL = none*/,
                                int32_t k_window, double w_rank, double w_prox, int32_t first, int32_t k,
                                ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                                double* scores_out /*[n_q][k], nullable*/, ss_proximity* prox_out /*[n_q][k], nullable*/);

/* Learned ranking: a tree ensemble over the signals of a hit, and a window re-ranked by it.  Every re-ranker above hard-wires one signal
 * and hand-set weights; a caller with click logs has a MODEL over all of them (a gradient-boosted forest, "learning to rank").  Training
 * is the caller's work, as producing embeddings and tokenising are: a trained model arrives as flat arrays.  No reference counterpart.
 * ss_rank_model_create.  A model: n_features columns, an optional linear part, a base and n_trees >= 0 trees (0: a linear model).  Tree
 * t is nodes[tree_ptr[t] .. tree_ptr[t + 1]), its root the first of them; left / right are indices INSIDE the tree.  The arrays are host
 * memory and are copied.  The score of a feature row x is defined bit for bit; every operation is rounded once, nothing is contracted:
 *     acc = base
 *     for f = 0 .. n_features-1, if linear != NULL and linear[f] != 0.0 and x[f] is not NaN:   acc = acc + linear[f] * x[f]
 *     for t = 0 .. n_trees-1:   walk tree t from its node 0 to a leaf L;   acc = acc + L.value
 *     score = acc               (a NaN result is written as 0x7FF8000000000000)
 *   A walk at a split goes left iff x[feature] <= value by numeric comparison (-0.0 <= 0.0; +-inf are ordinary thresholds and values); a
 *   NaN x[feature] goes left iff nan_left.
 *   The whole model is validated on the host, and nothing is uploaded when it fails.  SS_ERR_INVALID: n_features < 1, n_trees < 0,
 *   tree_ptr[0] != 0 or tree_ptr decreasing, an empty tree, a feature outside [-1, n_features), a split whose left or right is <= its own
 *   index or >= the tree's size, nan_left > 1, a NaN split value, a leaf value, base or linear weight that is not finite, a NULL array
 *   that is needed.  SS_ERR_UNSUPPORTED: n_features > SS_MAX_RANK_FEATURES, n_trees > SS_MAX_RANK_TREES, more than 2^24 nodes.  Because
 *   children have larger indices than their parent every walk ends within the tree's node count: no model that passes can make a kernel
 *   loop or read outside its arrays, on any feature values; the kernel bounds its walk by the tree's size as well.
 * ss_rank_model_get_info: the figures of the model; max_depth = the splits on the longest path from a node 0 to a leaf.
 * ss_rank_model_eval: scores_out[r] = the score of row x[r * n_features ..) for r < n_rows; x and scores_out host or device memory (with
 * both in device memory the call only enqueues on the ctx stream); n_rows < 0 is SS_ERR_INVALID, n_rows >= 2^31 SS_ERR_UNSUPPORTED.
 * The forest is walked out of the LDS in chunks of consecutive whole trees of at most option "rank.lds_nodes" nodes together (default
 * 1024, 1 .. 1024); a tree with more nodes is walked from global memory.  The order of the additions is the tree order and the scores are
 * the same bytes for every value.  A workgroup holds 256 rows of a model of at most 16 features, 64 rows of a wider one.
 * ss_rank_model_destroy waits for the ctx stream first.
 * ss_hit_features: the feature row of every row of a window, out[(q * k_in + j) * SS_RANK_N_FEATURES + c], written for j < n_hits[q]; every
 * other entry is left untouched.  E = prox[q * k_in + j], "absent" = the quiet NaN 0x7FF8000000000000:
 *     c 0..3    the row's title, body, pagerank, final: their 8 bytes as given (rows are trusted, as in ss_fuse_hits)
 *     c 4       (double)j, the window position
 *     c 5       (double)query_len[q]; absent without query_len
 *     c 6       (double)E.n_present
 *     c 7       sp = (double)E.end - (double)E.start
 *     c 8       prox = E.n_present < 2 ? 0.0 : (double)(E.n_present - 1) / max(sp, (double)(E.n_present - 1)), exactly
 *               ss_rerank_hits_by_proximity's
 *     c 9       (double)E.n_occ; columns 6..9 are all absent without prox
 *     c 10      (double)vec_scores[q * k_in + j]; absent without vec_scores or for SS_NO_VEC_SCORE
 *     c 11..14  (double)value[f][doc] of field f = 0..3 (int64 -> double, round to nearest even); absent when no table is registered,
 *               f >= n_fields, doc >= n_docs or the value is SS_NO_FIELD_VALUE
 * No registered table is required, and no doc id makes the kernel read outside one.  Checks, staging, host / device pointers and the
 * clamping of a device n_hits: those of ss_hit_fields without its table; prox, vec_scores and query_len may each be host or device memory.
 * ss_rerank_hits_by_model: the score of a row = the model's score of its ss_hit_features entry; Window, Order and Output word for word
 * those of ss_rerank_hits_by_proximity (score descending by numeric comparison, stable, NaN scores behind every number in window order,
 * rows with doc >= n_docs last of all with score NaN, the 40 bytes of a row copied, entries past n_hits_out[q] untouched).  So with a
 * linear model of linear[3] = 1 and nothing else, on rows in FinalRank order without NaN, the page is the window's page.  Checks, all
 * before anything is enqueued and with the outputs untouched: those of ss_rerank_hits_by_vector without a table to register; a model
 * with n_features != SS_RANK_N_FEATURES or of another context: SS_ERR_INVALID; the scratch for the feature matrix and the scores cannot
 * be had: SS_ERR_OOM.  With every given array in device memory the call only enqueues on the ctx stream and NEVER waits.
 * A known answer.  15 features, base 0.5, linear all zero but linear[3] = 2.0; T0 = [{f 8, value 0.5, nan_left 0, l 1, r 2}, leaf 0.0,
 * leaf 1.0], T1 = [{f 11, value 100, nan_left 1, l 1, r 2}, leaf 0.25, leaf -0.25].  Row A (final 1.0, prox 1.0, field0 50): 0.5 + 2.0
 * + 1.0 + 0.25 = 3.75.  Row B (final 1.5, no prox entry: NaN goes right; field0 SS_NO_FIELD_VALUE: NaN goes left): 0.5 + 3.0 + 1.0 +
 * 0.25 = 4.75.  Row C (final 1.0, prox 0.25, field0 200): 0.5 + 2.0 + 0.0 - 0.25 = 2.25.  The window (A, B, C) comes back as B, A, C. */
#define SS_RANK_N_FEATURES   15     /* columns of ss_hit_features */
#define SS_MAX_RANK_FEATURES 64     /* columns a model may read (ss_rank_model_eval takes any n_features up to this) */
#define SS_MAX_RANK_TREES    8192
typedef struct ss_rank_model ss_rank_model;
typedef struct ss_tree_node {       /* 24 bytes */
    int32_t  feature;   /* >= 0: split on this column; -1: leaf */
    uint32_t left;      /* node index inside the tree, > this node's own index (ignored in a leaf) */
    uint32_t right;     /* likewise */
    uint32_t nan_left;  /* 0 / 1: where a NaN feature value goes (ignored in a leaf) */
    double   value;     /* split: go left iff x <= value (numeric: -0.0 <= 0.0); leaf: the tree's output */
} ss_tree_node;
typedef struct ss_rank_model_info {
    int32_t  n_features, n_trees;
    uint32_t n_nodes, max_tree_nodes;
    uint32_t max_depth, _pad;
} ss_rank_model_info;               /* 24 bytes */
int32_t ss_rank_model_create(ss_ctx* ctx, int32_t n_features, const double* linear /*[n_features], nullable*/, double base,
                             int32_t n_trees, const uint32_t* tree_ptr /*[n_trees+1]*/, const ss_tree_node* nodes,
                             ss_rank_model** out);
int32_t ss_rank_model_destroy(ss_rank_model* m);
int32_t ss_rank_model_get_info(ss_rank_model* m, ss_rank_model_info* out);
int32_t ss_rank_model_eval(ss_rank_model* m, int64_t n_rows, const double* x /*[n_rows][n_features]*/, double* scores_out /*[n_rows]*/);
int32_t ss_hit_features(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/,
                        const ss_proximity* prox /*[n_q][k_in], nullable: ss_hit_proximity's output*/,
                        const int32_t* vec_scores /*[n_q][k_in], nullable: ss_hit_vector_scores' output*/,
                        const int32_t* query_len /*[n_q], nullable*/,
                        double* out /*[n_q][k_in][SS_RANK_N_FEATURES]*/);
int32_t ss_rerank_hits_by_model(ss_scorer* s, ss_rank_model* m, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/,
                                const int32_t* n_hits /*[n_q]*/, const ss_proximity* prox, const int32_t* vec_scores,
                                const int32_t* query_len, int32_t first, int32_t k,
                                ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/, double* scores_out /*[n_q][k], nullable*/);

/* Collapse by group ("host crowding"): at most g rows of one site on a result page, a "more from this site" count, and pages that
 * continue where the last one stopped.  The reference ranks pages, not sites (retrieval/main_retrieve.go:99-103 cuts the sorted list at 50).
 * The doc -> group table: group[d] is any 32-bit value (a site number, a hash of the host name); SS_NO_GROUP = doc d is never
 * collapsed with anything.  [n_docs] (the scorer's), host or device memory, copied; NULL clears.  Replaces the previous table after the
 * scorer's outstanding work (pipelined batches, tickets) has finished with it.  The table lives as long as the scorer: after an index
 * update (destroy scorers before, re-create after) register it again.  4 bytes per doc. */
#define SS_NO_GROUP 0xFFFFFFFFu
int32_t ss_scorer_set_doc_groups(ss_scorer* s, const uint32_t* group /*[n_docs], NULL clears*/);

/* ss_collapse_hits: collapse given rows.  Defined bit for bit:
 *   Window.     Row q's window is hits[q * k_in .. q * k_in + n_hits[q]), in the order given.  Nothing is re-sorted by score and only
 *               .doc of a row is read to decide anything: the rows may come from any scoring call or be made up by the caller.
 *   Group.      If doc < n_docs and group[doc] != SS_NO_GROUP the row's group is group[doc].  Otherwise the row is a group of its own:
 *               two such rows are never in the same group, even with equal docs.  Defined, not an error; no doc id makes the kernel
 *               read outside the table.
 *   Kept.       Row j is kept iff fewer than g rows i < j of the window are in j's group (the walk "keep a hit unless its site
 *               already has g").
 *   Output.     With the kept rows in window order K_0 .. K_{n_kept-1}: hits_out[q * k + r] = the 40 bytes of K_{first + r} (_pad included) for
 *               r < n_hits_out[q] = clamp(n_kept - first, 0, k) — page first / k of pages of k rows.  same_out[q * k + r]
 *               (nullable) = the number of rows of the WHOLE window in that row's group, the row itself included (1 for a row of its
 *               own): the number behind "3 more from this site".  n_kept_out[q] (nullable) = n_kept, so a pager knows how many pages
 *               the window holds.  Entries past n_hits_out[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle (or hits / n_hits / hits_out / n_hits_out with
 * n_q > 0), n_q < 0, k_in < 1, k < 1, g < 1, first < 0, hits_out overlapping hits as address ranges: SS_ERR_INVALID; k_in or k above
 * SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no group table registered: SS_ERR_STATE; n_hits[q] outside [0, k_in]: SS_ERR_INVALID when n_hits is
 * host memory, clamped by the kernel when it is device memory.  n_q == 0 is SS_OK and does nothing.
 * Every pointer may be host or device memory: when all given pointers are device memory the call only enqueues on the ctx stream and
 * NEVER waits, so it can sit right behind a scoring call whose outputs are device buffers (ss_score_topk_phrase, _constrained,
 * ss_similar_topk: there is no collapsed form of those, chain this call) and in front of ss_explain_hits; otherwise it
 * stages through blocks the scorer owns and returns when the outputs are written.  Serialised on the ctx like every scoring call; no
 * _submit / _collect form. */
int32_t ss_collapse_hits(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/,
                         const int32_t* n_hits /*[n_q]*/, int32_t g, int32_t first, int32_t k,
                         ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                         uint32_t* same_out /*[n_q][k], nullable*/, int32_t* n_kept_out /*[n_q], nullable*/);

/* Score and collapse in one call: row q = ss_collapse_hits applied to the row ss_score_topk_masked returns for query q with
 * k = k_window, this query_len, topic_probs[q] and mask_id[q] (mask_id NULL: the ss_score_topk row).  The window never leaves the
 * device: the scored rows stay inside the scorer and one kernel behind them writes the page.  With device outputs the call only
 * enqueues and never waits.  The window is the first k_window rows of the ranking: n_kept_out[q] counts kept rows of the window, and a
 * window that came back full (k_window rows) can mean the ranking, and the site's rows, continue past it — a caller who needs deeper
 * pages asks with a larger window; beyond SS_MAX_TOPK rows paging is not exact.  The query arrays are read on the host like every
 * scoring call's.  Checks as ss_collapse_hits (k_window for k_in) and as ss_score_topk_masked, plus topic_probs without a prior:
 * SS_ERR_STATE; all before anything is enqueued.  There is no phrase or constrained form: those callers score into device buffers
 * with their own call and chain ss_collapse_hits, which does not wait. */
int32_t ss_score_topk_collapsed(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                                const int32_t* query_len, const double* topic_probs, const int32_t* mask_id /*NULL = none*/,
                                int32_t k_window, int32_t g, int32_t first, int32_t k,
                                ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                                uint32_t* same_out /*[n_q][k], nullable*/, int32_t* n_kept_out /*[n_q], nullable*/);

/* Near-duplicate results: a MinHash signature per doc and a walk over one result window that drops the rows whose signature agrees
 * with an earlier kept row's ("some very similar results were omitted").  The reference ranks mirrors, print views and session-id
 * URLs as separate pages (retrieval/main_retrieve.go:99-103), and ss_collapse_hits only helps when the copies share a site key.
 * Integer arithmetic only, defined bit for bit:
 *   Hash.       With all arithmetic mod 2^32:   x = t + 0x9E3779B9 * (s + 1);
 *                                                x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16;
 *               h(t, s) = x.  h(0,0) = 0x92CA2F0E, h(1,0) = 0x96A0F96B, h(0,1) = 0x3CD6E3F3, h(12345,3) = 0x8EE55794,
 *               h(0xFFFFFFFE,31) = 0x26D56D90, h(70000,15) = 0x231FE950.
 *   Signature.  sig[d][s] = the minimum over the terms t of doc d's row of the doc view (ss_index_build_doc_view) of h(t, s), for
 *               s < n_slots.  Weights are not read.  A doc with an empty row has every slot = SS_SIG_EMPTY.  Row {3, 7, 70000} with
 *               4 slots gives 0x2316A329, 0x2C85567E, 0x41B9D641, 0x343B1A79.  A non-empty row is never all SS_SIG_EMPTY when
 *               n_slots >= 2: the mix is a bijection and the slots' offsets differ, so in one slot exactly one term value reaches
 *               0xFFFFFFFF and no term does so in two slots.
 * ss_index_build_signatures: n_slots in {4, 8, .., SS_MAX_SIG_SLOTS} (a row is then a multiple of 16 bytes); any other value up to
 * SS_MAX_SIG_SLOTS (zero and below included) is SS_ERR_INVALID, a larger one SS_ERR_UNSUPPORTED; a table without a doc view is
 * SS_ERR_STATE.  None of these touches signatures that exist.  The signatures are a snapshot and a pure function of the table: two
 * builds give identical bytes.  Resident size 4 * n_slots bytes per doc (640 MB at 10M docs and 16 slots).  Building where signatures
 * exist frees the old ones FIRST, and a build that fails (SS_ERR_OOM, SS_ERR_HIP) leaves the table WITHOUT signatures.
 * ss_tfidf_build, ss_index_apply_delta(_pos), ss_index_resize (and ss_index_destroy) free them; ss_index_drop_doc_view and a rebuild
 * of the view do not: the signatures are a snapshot of their own.  Without signatures ss_index_drop_signatures,
 * ss_index_read_signatures and ss_dedup_hits return SS_ERR_STATE.  The calls wait for their work.
 * ss_index_read_signatures: sig_out[i][0 .. n_slots) = sig[docs[i]]; *n_slots_out (nullable) = n_slots.  A doc id >= n_docs (or a
 * NULL docs / sig_out with n > 0) is SS_ERR_INVALID before anything is enqueued, sig_out untouched; a doc may appear more than once. */
#define SS_MAX_SIG_SLOTS 32
#define SS_SIG_EMPTY 0xFFFFFFFFu
int32_t ss_index_build_signatures(ss_index* idx, int32_t n_slots);
int32_t ss_index_drop_signatures(ss_index* idx);
int32_t ss_index_read_signatures(ss_index* idx, uint64_t n, const uint32_t* docs /*[n], host or device*/,
                                 uint32_t* sig_out /*[n][n_slots], host or device*/, int32_t* n_slots_out /*nullable*/);

/* ss_dedup_hits: drop the near-duplicate rows of given windows.  Reads the signatures of the scorer's BODY table.  Defined bit for bit:
 *   Window.     As in ss_collapse_hits: hits[q * k_in .. q * k_in + n_hits[q]), in the order given.  Only .doc of a row is read and
 *               nothing is re-sorted.
 *   Signature.  A row's signature is sig[doc] when doc < n_docs and sig[doc] is not all SS_SIG_EMPTY.  Otherwise the row is on its
 *               own: never a duplicate, and never the leader of any row but itself, even when another row has an equal doc.  No doc
 *               id makes the kernel read outside the table.
 *   match(i, j) = the number of slots s < n_slots in which the signatures of rows i and j are equal.
 *   Walk.       For j ascending: row j is a duplicate iff some KEPT row i < j has match(i, j) >= min_match; its leader is the smallest
 *               such i.  Otherwise j is kept and leads itself.  A dropped row shields nothing: with A ~ B and B ~ C but not A ~ C,
 *               B is dropped and C is kept.
 *   Output.     With the kept rows in window order K_0 .. K_{n_kept-1}: hits_out[q * k + r] = the 40 bytes of K_{first + r} for
 *               r < n_hits_out[q] = clamp(n_kept - first, 0, k), exactly as ss_collapse_hits copies them.  similar_out[q * k + r]
 *               (nullable) = the number of rows of the whole window led by that row, itself included.  n_kept_out[q] (nullable) =
 *               n_kept.  Entries past n_hits_out[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: those of ss_collapse_hits (NULL handle or array, n_q < 0,
 * k_in < 1, k < 1, first < 0, hits_out overlapping hits: SS_ERR_INVALID; k_in or k above SS_MAX_TOPK: SS_ERR_UNSUPPORTED; a host
 * n_hits[q] outside [0, k_in]: SS_ERR_INVALID, a device one is clamped by the kernel; n_q == 0 is SS_OK), with no signatures on the
 * body table: SS_ERR_STATE in place of the group table's, and min_match < 1 or min_match > n_slots: SS_ERR_INVALID in place of g's.
 * Pointers host or device: when all given pointers are device memory the call only enqueues on the ctx stream and NEVER waits, so
 * score -> dedup -> collapse -> explain -> passages chains on one stream; otherwise it stages through blocks the scorer owns and
 * returns when the outputs are written.  No fused scoring form and no _submit / _collect form. */
int32_t ss_dedup_hits(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/,
                      int32_t min_match, int32_t first, int32_t k,
                      ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                      uint32_t* similar_out /*[n_q][k], nullable*/, int32_t* n_kept_out /*[n_q], nullable*/);

/* Doc fields: a few signed 64-bit values per doc (a modification date as unix seconds, a page size in bytes), range filters over them,
 * a result window sorted by one of them, and their read-out per result row.  The reference's result card shows Mod_date and Page_size
 * (retrieval/util.go:28-29, filled from DocInfo, database/noschema_schema.go:34-38) and can neither restrict nor sort by them.
 * The table: values [n_fields][n_docs] field-major (n_docs = the scorer's), host or device memory, copied; n_fields = 0 / NULL clears.
 * Replaces the previous table after the scorer's outstanding work (pipelined batches, tickets) has finished with it.  The table lives as
 * long as the scorer: after an index update (destroy scorers before, re-create after) register it again.  8 bytes per doc and field.
 * n_fields < 0 is SS_ERR_INVALID, n_fields > SS_MAX_DOC_FIELDS is SS_ERR_UNSUPPORTED; a call that fails leaves the old table in place.
 * Every value is an ordinary value, SS_NO_FIELD_VALUE included: the read-outs write that one for a row whose doc is outside the table.
 * A range clause {field, lo, hi} MATCHES doc d iff lo <= value[field][d] <= hi as signed 64-bit integers; lo > hi matches nothing;
 * _pad is ignored. */
#define SS_MAX_DOC_FIELDS 4
#define SS_MAX_RANGE_CLAUSES 4            /* per query / per set */
#define SS_NO_FIELD_VALUE INT64_MIN
typedef struct ss_doc_range {
    int32_t field;     /* 0 .. n_fields-1 */
    int32_t _pad;
    int64_t lo, hi;    /* both inclusive */
} ss_doc_range;        /* 24 bytes */
int32_t ss_scorer_set_doc_fields(ss_scorer* s, int32_t n_fields, const int64_t* values /*[n_fields][n_docs], 0 / NULL clears*/);

/* Allow-lists from range clauses, built on the device ("past day / week / month / year", once per index refresh).  Defined bit for bit:
 * bit (d & 31) of word d >> 5 of set i of words_out [n_sets][(n_docs+31)/32] is 1 iff d < n_docs, d is in the REGISTERED allow-list
 * mask_id[i] (ss_scorer_set_doc_masks; -1 = every doc; mask_id NULL = all -1) and every clause of rng[rng_ptr[i] .. rng_ptr[i+1])
 * matches d.  Bits at and past n_docs in the last word are 0.  A set without clauses is its mask; with mask_id -1 it is all ones up to
 * n_docs.  Duplicate sets are sets like any other.  The layout is that of ss_scorer_set_doc_masks: the output can be registered as it is.
 * Checks, all before anything is enqueued and with words_out untouched: NULL handle, rng_ptr or words_out (or rng with a clause),
 * n_sets < 0, an rng_ptr that does not start at 0 or decreases, a clause field outside [0, n_fields), a mask_id below -1 or at / above
 * n_masks: SS_ERR_INVALID; more than SS_MAX_RANGE_CLAUSES clauses in one set: SS_ERR_UNSUPPORTED; a clause but no field table:
 * SS_ERR_STATE.  n_sets == 0 is SS_OK and does nothing.  rng_ptr / rng / mask_id are read on the host like the query arrays;
 * words_out may be host or device memory; the call waits for its work.  A host words_out goes through a device block of the same
 * size (SS_ERR_OOM if it cannot be had), kept by the scorer for the next call up to 64 MB and freed before the call returns beyond.
 * k_field_masks reads each field column once per group of 64 sets (80 MB per field at 10M docs), forms the words by wave ballot and
 * writes every word of every set exactly once: no atomics, no order dependence, no temporaries. */
int32_t ss_doc_field_masks(ss_scorer* s, int32_t n_sets, const uint32_t* rng_ptr /*[n_sets+1]*/, const ss_doc_range* rng,
                           const int32_t* mask_id /*[n_sets], -1 = every doc, NULL = all -1*/,
                           uint32_t* words_out /*[n_sets][(n_docs+31)/32], host or device*/);

/* ss_score_topk_constrained plus range clauses per query: "past week", "pages under 100 KB".  Doc d is allowed for query q iff it is
 * allowed by ss_score_topk_constrained's rule AND matches every clause of rng[rng_ptr[q] .. rng_ptr[q+1]).  Row q = byte for byte what
 * ss_score_topk_masked returns with that allowed set registered as the query's allow-list: NOT a post-filter of the unrestricted top-k.
 * The clauses only filter.  The allowed sets are built on the device for the call, one per distinct (mask, required, excluded, clauses)
 * combination (the clauses compared as sets: order and repeats do not matter), as in ss_score_topk_constrained: n_docs / 8 bytes each,
 * SS_ERR_OOM if that memory cannot be had.  rng_ptr [n_q+1] (NULL = none) starts at 0 and never decreases, a clause field lies in
 * [0, n_fields), else SS_ERR_INVALID; more than SS_MAX_RANGE_CLAUSES clauses in one query (as given, repeats counted) is
 * SS_ERR_UNSUPPORTED; a clause but no field table is SS_ERR_STATE; the other checks are ss_score_topk_constrained's.  Every check comes
 * before anything is enqueued and leaves the outputs untouched.  A call without a clause IS ss_score_topk_constrained (same kernels,
 * bit-identical rows).  rng_ptr / rng are read on the host like the constraint arrays (device pointers cost one blocking copy each);
 * outputs as ss_score_topk (device outputs: the call only enqueues, pipelined like any other batch).
 * There is no filtered form of ss_score_topk_submit / _collect. */
int32_t ss_score_topk_filtered(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                               const uint32_t* p_ptr, const uint32_t* p_terms, const int32_t* query_len,
                               const double* topic_probs, const int32_t* mask_id,
                               const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                               const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                               const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                               int32_t k, ss_hit* hits_out, int32_t* n_hits_out);

/* ss_sort_hits_by_field: a result window sorted by a field ("newest first").  Defined bit for bit:
 *   Window.     As in ss_collapse_hits: hits[q * k_in .. q * k_in + n_hits[q]), in the order given; only .doc of a row is read.
 *   Order.      Rows with doc < n_docs by value[field][doc], ascending (descending == 0) or descending (descending != 0) as signed
 *               64-bit integers, rows of equal value in window order (the sort is stable; the same doc twice is two rows).  Rows with
 *               doc >= n_docs come LAST in both directions, among themselves in window order.  No doc id makes the kernel read outside
 *               the table.
 *   Output.     With the sorted rows S_0 .. S_{n-1}: hits_out[q * k + r] = the 40 bytes of S_{first + r} (_pad included) for
 *               r < n_hits_out[q] = clamp(n - first, 0, k); values_out[q * k + r] (nullable) = that row's value, SS_NO_FIELD_VALUE
 *               for a row with doc >= n_docs.  Entries past n_hits_out[q] are left untouched.
 * ss_hit_fields: values_out[(q * k_in + j) * n_fields + f] = value[f][hits[q * k_in + j].doc] for j < n_hits[q] and every registered
 * field f; SS_NO_FIELD_VALUE in every field for a row with doc >= n_docs; rows past n_hits[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle (or hits / n_hits / hits_out / n_hits_out /
 * values_out of ss_hit_fields with n_q > 0), n_q < 0, k_in < 1, k < 1, first < 0, a field outside [0, n_fields), hits_out overlapping
 * hits as address ranges: SS_ERR_INVALID; k_in or k above SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no field table registered: SS_ERR_STATE;
 * n_hits[q] outside [0, k_in]: SS_ERR_INVALID when n_hits is host memory, clamped by the kernel when it is device memory.  n_q == 0
 * is SS_OK and does nothing.
 * Every pointer may be host or device memory: when all given pointers are device memory the calls only enqueue on the ctx stream and
 * NEVER wait, so score -> dedup -> collapse -> sort -> explain chains on one stream; otherwise they stage through blocks the scorer
 * owns and return when the outputs are written.  Serialised on the ctx like every scoring call; no _submit / _collect form. */
int32_t ss_sort_hits_by_field(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/,
                              const int32_t* n_hits /*[n_q]*/, int32_t field, int32_t descending, int32_t first, int32_t k,
                              ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/, int64_t* values_out /*[n_q][k], nullable*/);
int32_t ss_hit_fields(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/,
                      int64_t* values_out /*[n_q][k_in][n_fields]*/);

/* ss_facet_counts: how many docs a query matches -- "about 1,240,000 results" --, how many of them lie in every registered allow-list
 * -- "News (312) . Docs (4,881)" -- and how many in every bucket of a doc field -- "past day (14) . past week (230)".  No reference
 * counterpart.  A scoring call returns at most SS_MAX_TOPK rows and says nothing about the docs behind them.  Defined bit for bit; no
 * float is involved, counts are exact and no order of summation can show:
 *   C(q)        = the docs d < n_docs that CONTAIN (as in ss_score_topk_constrained: a posting in the title or the body table, of any
 *                 weight, zero included) at least one term t of q_terms[q_ptr[q] .. q_ptr[q+1]) with t < n_terms.  SS_UNKNOWN_TERM and
 *                 every other id >= n_terms contribute nothing; a repeated term changes nothing; a query without a usable term has an
 *                 empty C(q).
 *   A(q)        = the allowed set ss_score_topk_filtered builds for the same mask_id, req_*, exc_* and rng_* arguments (every doc when
 *                 all of them are NULL).
 *   M(q)        = C(q) AND A(q): exactly the docs ss_score_topk_filtered ranks for these arguments with p_ptr NULL.  That call's
 *                 candidates are the docs with a posting of a query term and nothing else: no score, NaN included, drops a doc, and
 *                 query_len / topic_probs only move scores.  So n_match_out[q] >= that call's n_hits_out[q], with equality whenever
 *                 |M(q)| <= k.
 *   n_match_out[q]                          = |M(q)|.
 *   mask_counts_out[q * n_masks + m]        = |M(q) AND mask_m| for every registered allow-list m (ss_scorer_set_doc_masks), bits at
 *                 and past n_docs ignored.  NULL: not counted.  With no masks registered the pointer is ignored.
 *   bucket_counts_out[q * n_buckets + b]    = the number of d in M(q) with buckets[b].lo <= value[buckets[b].field][d] <= buckets[b].hi
 *                 as signed 64-bit integers.  Buckets may overlap, nest ("past day" inside "past week"), repeat and name different
 *                 fields; a bucket with lo > hi counts 0; SS_NO_FIELD_VALUE is a value like any other; _pad is ignored.  The
 *                 buckets [n_buckets] are shared by the whole batch.
 * A known answer: 8 docs, 3 terms; the docs that contain t0 = {1, 2, 5} (doc 1 in both tables), t1 = {2, 3}, t2 = {6}; field 0 = 10, 20,
 * .. 80 for docs 0 .. 7; masks m0 = {0, 1, 2, 3}, m1 = {2, 5, 6}; buckets on field 0: [20, 30], [0, 100], [30, 60], [5, 4].  The query
 * (t0, t1, t0, SS_UNKNOWN_TERM) has C = {1, 2, 3, 5}.  Unconstrained: n_match 4, mask counts 3, 2, bucket counts 2, 4, 3, 0.  With t1
 * required: M = {2, 3}: 2; 2, 1; 1, 2, 2, 0.  With mask_id 1 and the clause field 0 in [25, 65]: A = {2, 5}, M = {2, 5}: 2; 1, 2; 1, 2, 2, 0.
 * Checks, all before anything is enqueued and with the outputs untouched: everything ss_score_topk_filtered checks about its query,
 * mask, constraint and range arrays, with its codes (more than SS_MAX_QUERY_TERMS distinct usable terms in a query included:
 * SS_ERR_UNSUPPORTED); NULL handle; n_q < 0; NULL q_ptr or n_match_out with n_q > 0; n_buckets < 0; NULL buckets or bucket_counts_out
 * with n_buckets > 0; a bucket field outside [0, n_fields): SS_ERR_INVALID; n_buckets > SS_MAX_FACET_BUCKETS: SS_ERR_UNSUPPORTED; a
 * bucket but no field table: SS_ERR_STATE.  n_q == 0 is SS_OK and does nothing.
 * The query, constraint and bucket arrays are read on the host like every scoring call's (device pointers cost one blocking copy
 * each).  The outputs may be host or device memory: when all given outputs are device memory the call only enqueues on the ctx stream
 * and NEVER waits, so it sits beside the scoring call of the same batch; otherwise it goes through a block the scorer owns and returns
 * when the outputs are written.  The allowed sets are built as in ss_score_topk_filtered (n_docs / 8 bytes per distinct set,
 * SS_ERR_OOM if that cannot be had); M(q) itself is never written out.  k_facet_counts gives a workgroup one block of 32768 docs of
 * one query: the runs of the query's lists in the block by binary search, ORed into an LDS image, ANDed with the allowed words and
 * d < n_docs, then one popcount for the total, one popcount of image & mask per registered mask, and for the buckets one gather of
 * value[field][d] per SET bit; the partial counts join the zeroed outputs by integer atomic adds.
 * Serialised on the ctx like every scoring call.  There is no phrase form (no p_ptr) and no _submit / _collect form. */
#define SS_MAX_FACET_BUCKETS 64
int32_t ss_facet_counts(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                        const int32_t* mask_id,
                        const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                        const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                        const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                        int32_t n_buckets, const ss_doc_range* buckets /*[n_buckets], shared by the whole batch*/,
                        uint32_t* n_match_out /*[n_q]*/,
                        uint32_t* mask_counts_out /*[n_q][n_masks], nullable*/,
                        uint32_t* bucket_counts_out /*[n_q][n_buckets], NULL iff n_buckets == 0*/);

/* ss_field_topk: the docs a query matches, ordered by a doc field, over ALL matches -- "newest first", "smallest pages first", "oldest
 * match".  No reference counterpart.  ss_sort_hits_by_field orders a window of at most SS_MAX_TOPK rows that relevance chose; this call
 * selects among every doc of M(q).  Defined bit for bit; no float is involved:
 *   M(q)        = exactly the set ss_facet_counts defines for the same q_*, mask_id, req_*, exc_* and rng_* arguments, which is the set
 *                 ss_score_topk_filtered ranks with p_ptr NULL.  Unknown term ids contribute nothing, a repeated term changes nothing,
 *                 docs at or above n_docs are never in it.
 *   Order.      By value[field][d] as signed 64-bit integers, ascending (descending == 0) or descending (descending != 0); docs of
 *               equal value in ascending doc id in BOTH directions.  SS_NO_FIELD_VALUE is a value like any other.  The order is total,
 *               so no summation or arrival order can show.
 *   Output.     With the ordered docs S_0 .. S_{n-1}, n = |M(q)|: n_out[q] = clamp(n - first, 0, k); docs_out[q * k + r] = S_{first + r}
 *               for r < n_out[q]; values_out[q * k + r] (nullable) = that doc's value; n_match_out[q] (nullable) = n, the number
 *               ss_facet_counts writes.  Entries past n_out[q] are left untouched.  A query without a usable term: n_out 0, n_match 0.
 * A known answer: the 8 docs of ss_facet_counts' comment (field 0 = 10, 20, .. 80; t0 = {1, 2, 5}, t1 = {2, 3}; m1 = {2, 5, 6}) and the
 * query (t0, t1, t0, SS_UNKNOWN_TERM), C = {1, 2, 3, 5}, n_match 4.  Field 0 ascending, first 0, k 4: docs 1, 2, 3, 5, values 20, 30, 40,
 * 60.  Descending, first 1, k 2: docs 3, 2, values 40, 30, n_out 2.  With t1 required (M = {2, 3}), ascending: docs 2, 3, values 30, 40,
 * n_match 2.  With mask_id 1 and the clause field 0 in [25, 65] (M = {2, 5}), descending: docs 5, 2, values 60, 30, n_match 2.  A second
 * field 5, 7, 7, 7, 0, 7, 0, 0: descending over C gives docs 1, 2, 3, 5 -- all tie at 7 and fall back to ascending doc id.
 * Checks, all before anything is enqueued and with the outputs untouched: everything ss_facet_counts checks about its query, mask,
 * constraint and range arrays, with its codes; NULL handle; n_q < 0; NULL q_ptr, docs_out or n_out with n_q > 0; k < 1; first < 0; a
 * field outside [0, n_fields): SS_ERR_INVALID; first + k > SS_MAX_TOPK (computed without overflow): SS_ERR_UNSUPPORTED -- a deeper page
 * is asked for with a range clause on the last value seen, as "value < last" (or "> last") plus the docs that tie with it; no field
 * table registered: SS_ERR_STATE.  n_q == 0 (with a handle) is SS_OK and does nothing, whatever the other arguments are: that rule comes
 * first, before k, first, field and the field table are looked at.
 * The query, constraint and range arrays are read on the host like every scoring call's.  The outputs may be host or device memory: when
 * all given outputs are device memory the call only enqueues on the ctx stream and NEVER waits; otherwise it goes through a block the
 * scorer owns and returns when the outputs are written.  docs_out and n_out are laid out as ss_score_docs takes docs and n_in with
 * k_in = k, so ss_field_topk -> ss_score_docs -> explain -> passages chains on one stream without a wait.
 * k_field_select gives a workgroup a run of consecutive 32768-doc blocks of one query: per block the match words as in k_facet_counts
 * (the bounds of the lists' runs searched from the previous block's ends), per set bit one gather of value[field][d], and a running
 * best first + k in LDS (a threshold and a buffer compacted by a bitonic sort when it fills); k_field_merge joins the runs' lists per
 * query.  Runs per query: option "ftopk.runs" (0 = from the device and the batch); the partial lists are bounded by option
 * "ftopk.scratch_bytes" (default 256 MB), the queries going in groups beyond it.  No atomics on any output.
 * Serialised on the ctx like every scoring call.  There is no phrase form (no p_ptr) and no _submit / _collect form. */
int32_t ss_field_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                      const int32_t* mask_id,
                      const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                      const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                      const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                      int32_t field, int32_t descending, int32_t first, int32_t k,
                      uint32_t* docs_out    /*[n_q][k]*/,
                      int32_t*  n_out       /*[n_q]*/,
                      int64_t*  values_out  /*[n_q][k], nullable*/,
                      uint32_t* n_match_out /*[n_q], nullable*/);

/* ss_top_groups: where a query's matches are -- "Results from 312 sites . example.org (4,881) . docs.example.com (1,902)", the languages
 * of the matches, the authors: the terms facet over the doc -> group table of ss_scorer_set_doc_groups.  No reference counterpart.
 * ss_collapse_hits sees the at most SS_MAX_TOPK rows relevance chose; this call counts every doc of M(q).  Defined bit for bit; no
 * float is involved:
 *   M(q)        = exactly the set ss_facet_counts defines for the same q_*, mask_id, req_*, exc_* and rng_* arguments.
 *   cnt(q, v)   = the number of d in M(q) with group[d] == v, for v != SS_NO_GROUP.
 *   Order.      The values v with cnt(q, v) > 0, by cnt descending, equal counts by value ascending as unsigned 32-bit.  The order is
 *               total, so no summation or arrival order can show.
 *   Output.     With that sequence G_0 .. G_{n-1}: n_out[q] = clamp(n - first, 0, m); groups_out[q * m + r] = {G_{first + r}, its cnt}
 *               for r < n_out[q]; entries past n_out[q] are left untouched; n_groups_out[q] (nullable) = n; n_ungrouped_out[q]
 *               (nullable) = the number of d in M(q) with group[d] == SS_NO_GROUP; n_match_out[q] (nullable) = |M(q)|, the number
 *               ss_facet_counts writes.  The counts of all n groups plus n_ungrouped add up to n_match.  A query without a usable
 *               term gets zeros everywhere.
 * A known answer: the 8 docs of ss_facet_counts' comment (t0 = {1, 2, 5}, t1 = {2, 3}, t2 = {6}; field 0 = 10, 20, .. 80; m1 = {2, 5, 6})
 * with the table group = 7, 7, 7, 3, 3, SS_NO_GROUP, 0xFFFFFFFE, 3, whose distinct values are 3, 7, 0xFFFFFFFE.  The query (t0, t1, t0,
 * SS_UNKNOWN_TERM), M = {1, 2, 3, 5}: first 0, m 4 gives (7, 2), (3, 1), n_out 2, n_groups 2, n_ungrouped 1, n_match 4; first 1, m 1
 * gives (3, 1), n_out 1, the counts as before.  With t1 required, M = {2, 3}: (3, 1), (7, 1) -- a tie, value ascending --, n_groups 2,
 * n_ungrouped 0, n_match 2.  With mask_id 1 and the clause field 0 in [25, 65], M = {2, 5}: (7, 1), n_out 1, n_groups 1, n_ungrouped 1,
 * n_match 2.  The query (t2), M = {6}: (0xFFFFFFFE, 1), n_groups 1, n_ungrouped 0, n_match 1.
 * Checks, all before anything is enqueued and with the outputs untouched: everything ss_facet_counts checks about its query, mask,
 * constraint and range arrays, with its codes; NULL handle; n_q < 0; NULL q_ptr, groups_out or n_out with n_q > 0; m < 1; first < 0:
 * SS_ERR_INVALID; first + m > SS_MAX_TOPK (computed without overflow): SS_ERR_UNSUPPORTED; no group table registered: SS_ERR_STATE.
 * n_q == 0 (with a handle) is SS_OK and does nothing, whatever the other arguments are: that rule comes first.
 * The group ranks: the first call that needs them after ss_scorer_set_doc_groups sorts a copy of the table, keeps its distinct values
 * != SS_NO_GROUP ascending and gives every doc the index of its value (4 bytes per doc + 4 per distinct value, SS_ERR_OOM if that cannot
 * be had).  That call waits once; registering a table again, or clearing it, drops the ranks.  ss_scorer_group_values reads them out
 * (and builds them if they are missing): *n_groups_out (nullable) = the number of distinct values, values_out (nullable, host or device
 * memory, [n_groups]) = the values ascending.  NULL handle: SS_ERR_INVALID; no group table: SS_ERR_STATE.
 * The query, constraint and range arrays are read on the host like every scoring call's.  The outputs may be host or device memory: when
 * all given outputs are device memory and the ranks are built, the call only enqueues on the ctx stream and NEVER waits; otherwise it
 * goes through a block the scorer owns and returns when the outputs are written.
 * k_group_count gives a workgroup a run of consecutive 32768-doc blocks of one query: per block the match words as in k_field_select,
 * per set bit one gather of the doc's rank, counted into the query's row of n_groups + 2 integer counters -- through a histogram in LDS
 * when the table has at most option "gtopk.lds_groups" (default 8192, at most 8192, 0 = never) distinct values, by global atomic adds
 * with consecutive equal ranks merged otherwise; both paths give the same bytes.  k_group_select, one workgroup per query, pushes the
 * row's non-zero counters through a running best first + m and writes the page.  Runs per query: option "gtopk.runs" (0 = from the
 * device and the batch); the counter rows are bounded by option "gtopk.scratch_bytes" (default 256 MB), the queries going in groups
 * beyond it, at least one query per group.  Integer atomics only.
 * Serialised on the ctx like every scoring call.  There is no phrase form (no p_ptr) and no _submit / _collect form. */
typedef struct ss_group_count { uint32_t group; uint32_t count; } ss_group_count;   /* 8 bytes */
int32_t ss_scorer_group_values(ss_scorer* s, uint32_t* n_groups_out /*nullable*/,
                               uint32_t* values_out /*[n_groups] ascending, nullable; host or device*/);
int32_t ss_top_groups(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                      const int32_t* mask_id,
                      const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                      const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                      const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                      int32_t first, int32_t m,
                      ss_group_count* groups_out /*[n_q][m]*/,
                      int32_t*  n_out           /*[n_q]*/,
                      uint32_t* n_groups_out    /*[n_q], nullable*/,
                      uint32_t* n_ungrouped_out /*[n_q], nullable*/,
                      uint32_t* n_match_out     /*[n_q], nullable*/);

/* ss_field_stats and ss_field_histogram: the range, the sum and a timeline of a doc field over ALL docs a query matches -- "pages from
 * 2009 to 2024", "sizes 2 KB to 14 MB, 61 KB on average" to size a date or size slider, "matches per month over twenty years" to draw
 * one.  No reference counterpart.  ss_field_topk gives the smallest or largest value only as the head of a selection and no sum;
 * ss_facet_counts stops at SS_MAX_FACET_BUCKETS nested buckets.  Both calls are defined bit for bit; no float is involved, every
 * operation is exact and associative, and no order of arrival can show:
 *   M(q)        = exactly the set ss_facet_counts defines for the same q_*, mask_id, req_*, exc_* and rng_* arguments.
 *   Missing.    In THESE TWO calls SS_NO_FIELD_VALUE means "no value": a doc of M(q) whose value in the field is SS_NO_FIELD_VALUE is
 *               counted in `missing` and takes part in nothing else -- not in min, max or sum, not in any bin, below or above, not even
 *               with origin == INT64_MIN.  Every other field call (range clauses, ss_facet_counts' buckets, ss_field_topk,
 *               ss_sort_hits_by_field) keeps treating it as the ordinary value INT64_MIN: a clause [INT64_MIN, x] still lets such docs
 *               into M(q), and they are then counted here as missing.
 *   ss_field_stats      stats_out[q * n_stat_fields + i], for field fields[i] (1 <= n_stat_fields <= SS_MAX_DOC_FIELDS; a repeated field
 *               is allowed and gives equal entries): count = the docs of M(q) with a value, missing = those without, count + missing =
 *               |M(q)|; min / max over the docs with a value as signed 64-bit, INT64_MAX / INT64_MIN when count == 0; sum_hi : sum_lo =
 *               their exact sum as a 128-bit two's complement integer.  A query with an empty M(q), one without a usable term included,
 *               gets the identity entry {INT64_MAX, INT64_MIN, 0, 0, 0, 0}.  n_match_out[q] (nullable) = |M(q)|, the number
 *               ss_facet_counts writes.  Every entry of every query is written.
 *   ss_field_histogram, fixed width (edges == NULL, width >= 1).  A doc with value v: v < origin as signed 64-bit counts in `below`;
 *               otherwise u = (uint64_t)v - (uint64_t)origin (exact: the difference of two int64 fits 64 unsigned bits), b = u / width;
 *               b >= n_bins counts in `above`, else counts_out[q * n_bins + b]++.  width may be any value up to 2^64 - 1;
 *               origin + n_bins * width is never formed in signed arithmetic.
 *   ss_field_histogram, explicit edges (edges != NULL; origin and width are ignored): calendar months, log-scale sizes.
 *               edges[0 .. n_bins] is strictly ascending as signed 64-bit; bin b is edges[b] <= v < edges[b + 1]; v < edges[0] counts
 *               in `below`, v >= edges[n_bins] in `above`.
 *   Histogram outputs.  1 <= n_bins <= SS_MAX_HIST_BINS.  All n_bins counters of every query are written, zeros included.  tails_out[q]
 *               (nullable) = {below, above, missing, n_match}; the counters plus below, above and missing add up to n_match, the number
 *               ss_facet_counts writes.  A query without a usable term gets zeros everywhere.
 * Known answers: the 8 docs of ss_facet_counts' comment (field 0 = 10, 20, .. 80 for docs 0 .. 7; t0 = {1, 2, 5}, t1 = {2, 3}; m1 = {2, 5,
 * 6}) and the query (t0, t1, t0, SS_UNKNOWN_TERM), M = {1, 2, 3, 5} with field-0 values 20, 30, 40, 60.  Stats of field 0: count 4,
 * missing 0, min 20, max 60, sum 150.  With t1 required, M = {2, 3}: 2, 0, 30, 40, 70.  With mask_id 1 and the clause field 0 in [25, 65],
 * M = {2, 5}: 2, 0, 30, 60, 90.  A second field that holds INT64_MAX for docs 1, 2, 3, SS_NO_FIELD_VALUE for doc 5 and 0 elsewhere, over
 * M = {1, 2, 3, 5}: count 3, missing 1, min = max = INT64_MAX, sum = 3 (2^63 - 1): sum_hi 1, sum_lo 0x7FFFFFFFFFFFFFFD.  Two values of
 * -1 sum to sum_lo 0xFFFFFFFFFFFFFFFE, sum_hi -1.  Histograms of field 0 over M = {1, 2, 3, 5}: origin 15, width 20, 2 bins: counts 2, 1,
 * below 0, above 1.  Origin 35, width 20, 2 bins: 1, 1, below 2, above 0.  Edges {20, 40, 61}: 2, 2, below 0, above 0.  Edges {25, 30,
 * 31}: 0, 1, below 1, above 2.
 * Checks, all before anything is enqueued and with the outputs untouched: everything ss_facet_counts checks about its query, mask,
 * constraint and range arrays, with its codes; NULL handle; n_q < 0; NULL q_ptr, stats_out or counts_out with n_q > 0; n_stat_fields < 1
 * or NULL fields; a field outside [0, n_fields); n_bins < 1; width == 0 with edges == NULL; edges that are not strictly ascending:
 * SS_ERR_INVALID; n_stat_fields > SS_MAX_DOC_FIELDS; n_bins > SS_MAX_HIST_BINS: SS_ERR_UNSUPPORTED; no field table registered:
 * SS_ERR_STATE.  n_q == 0 (with a handle) is SS_OK and does nothing, whatever the other arguments are: that rule comes first.
 * The query, constraint and range arrays, fields and edges are read on the host like every scoring call's (device pointers cost one
 * blocking copy each).  The outputs may be host or device memory: when all given outputs are device memory the calls only enqueue on the
 * ctx stream and NEVER wait; otherwise they go through a block the scorer owns and return when the outputs are written.
 * k_field_stats gives a workgroup a run of consecutive 32768-doc blocks of one query: per block the match words as in k_group_count, per
 * set bit one gather of value[field][d] per asked field; a thread keeps min, max, a 128-bit sum (a low word with carry, a high word) and
 * the missing count per field in registers, the workgroup reduces them by wave shuffles and through LDS and writes one partial
 * ss_field_stat per field; k_field_stats_merge folds the runs' partials per (query, field) and writes the identity entries of the
 * queries without a list.  No atomics touch any stats output.  k_field_hist has k_group_count's shape with the bin computed from the
 * gathered value: a shift for a width that is a power of two, else a multiply-high by a reciprocal computed on the host plus one fix-up
 * (exact for every 64-bit u), u >= n_bins * width decided before any of it; a binary search over the edges otherwise (an LDS copy of
 * up to 1025 edges, the staged array beyond).  A thread walks its docs in ascending order and merges consecutive equal bins into one
 * add; the adds go to an LDS histogram that joins the query's zeroed counter row at the end of the run when n_bins is at most option
 * "fstats.lds_bins" (default 8192, at most 8192, 0 = never), straight to the row by global atomic adds otherwise; both paths give the
 * same bytes.  The row has n_bins + 4 counters (below, above, missing, matches behind the bins); k_field_hist_out copies rows and tails
 * out.  Runs per query: option "fstats.runs" (0 = from the device and the batch); the partial entries or counter rows are bounded by
 * option "fstats.scratch_bytes" (default 256 MB), the queries going in groups beyond it, at least one query per group.
 * Serialised on the ctx like every scoring call.  There is no phrase form (no p_ptr) and no _submit / _collect form. */
#define SS_MAX_HIST_BINS 65536
typedef struct ss_field_stat {         /* 40 bytes */
    int64_t  min, max;                 /* over the docs that have a value; INT64_MAX / INT64_MIN when count == 0 */
    uint64_t sum_lo; int64_t sum_hi;   /* the exact sum as a 128-bit two's complement integer */
    uint32_t count, missing;           /* docs of M(q) with value != / == SS_NO_FIELD_VALUE; count + missing == |M(q)| */
} ss_field_stat;
typedef struct ss_hist_tail { uint32_t below, above, missing, n_match; } ss_hist_tail;   /* 16 bytes */
int32_t ss_field_stats(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                       const int32_t* mask_id,
                       const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                       const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                       const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                       int32_t n_stat_fields, const int32_t* fields /*[n_stat_fields], host*/,
                       ss_field_stat* stats_out /*[n_q][n_stat_fields]*/,
                       uint32_t* n_match_out    /*[n_q], nullable*/);
int32_t ss_field_histogram(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms,
                           const int32_t* mask_id,
                           const uint32_t* req_ptr /*[n_q+1], NULL = none*/, const uint32_t* req_terms,
                           const uint32_t* exc_ptr /*[n_q+1], NULL = none*/, const uint32_t* exc_terms,
                           const uint32_t* rng_ptr /*[n_q+1], NULL = none*/, const ss_doc_range* rng,
                           int32_t field, int64_t origin, uint64_t width,
                           const int64_t* edges /*[n_bins + 1] or NULL, host*/, int32_t n_bins,
                           uint32_t* counts_out    /*[n_q][n_bins]*/,
                           ss_hist_tail* tails_out /*[n_q], nullable*/);

/* Doc vectors: one signed 8-bit embedding per doc, the exact k nearest docs of a query vector, and a lexical result window re-ordered
 * by meaning.  No reference counterpart: every way the reference finds a page is a posting of a typed word.  Producing the embeddings
 * is the caller's work, as tokenising is; the caller brings [n_docs][dim] and [n_q][dim] int8.
 * The table: vec [n_docs][dim] doc-major (n_docs = the scorer's), host or device memory, copied; dim = 0 / NULL clears.  dim is a
 * multiple of 64 in [64, SS_MAX_VEC_DIM], anything else is SS_ERR_INVALID.  n_docs * dim bytes (1.28 GB at 10M docs and dim 128):
 * SS_ERR_OOM if that cannot be had.  Replaces the previous table after the scorer's outstanding work (pipelined batches, tickets) has
 * finished with it.  The table lives as long as the scorer: after an index update (destroy scorers before, re-create after) register
 * it again.  A call that fails leaves the old table in place.  Every int8 value is an ordinary value, -128 included; a doc whose vector
 * is all zero is a doc like any other.
 * Defined bit for bit:
 *   score(q, d) = the sum over i < dim of (int32)qvec[q][i] * (int32)vec[d][i], in exact 32-bit integer arithmetic (|score| <= 2^24).
 *               Nothing is normalised on the device: a caller who wants cosine quantises unit vectors. */
#define SS_MAX_VEC_DIM   1024          /* dim is a multiple of 64 in [64, 1024] */
#define SS_NO_VEC_SCORE  INT32_MIN     /* never a real score: |score| <= 1024*128*128 = 2^24 */
typedef struct ss_vec_hit { uint32_t doc; int32_t score; } ss_vec_hit;   /* 8 bytes */
int32_t ss_scorer_set_doc_vectors(ss_scorer* s, int32_t dim, const int8_t* vec /*[n_docs][dim] doc-major; 0 / NULL clears*/);

/* ss_vector_topk: exact nearest neighbours, not an approximate search and not a post-filter.  Defined bit for bit:
 *   Candidates. Every doc d < n_docs in the REGISTERED allow-list mask_id[q] (ss_scorer_set_doc_masks; -1 = every doc; mask_id NULL =
 *               all -1).  What ss_doc_field_masks writes can be registered as it is ("semantic search in the past week").
 *   Order.      score(q, d) descending, then d ascending.
 *   Output.     Row q = the first n_hits_out[q] = min(k, number of candidates) rows of that order; entries past that are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle (or qvec / hits_out / n_hits_out with n_q > 0),
 * n_q < 0, k < 1, a mask_id below -1 or at / above n_masks: SS_ERR_INVALID; k > SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no vector table
 * registered: SS_ERR_STATE.  n_q == 0 is SS_OK and does nothing.  mask_id is read on the host like the query arrays of the scoring
 * calls (a device pointer costs one blocking copy); qvec and the outputs may be host or device memory: with all of them on the device
 * the call only enqueues on the ctx stream and NEVER waits, otherwise it stages through blocks the scorer owns and returns when the
 * outputs are written.  The chunks' partial lists take n_q * chunks * k * 8 bytes of device memory (bounded by 256 MB unless option
 * "vec.chunk_docs" asks for more chunks): SS_ERR_OOM if that cannot be had.  More than 65535 blocks of queries: SS_ERR_UNSUPPORTED.
 * k_vec_topk multiplies tiles of 64 docs with blocks of up to 64 queries on the int8 matrix cores, reads every doc byte once per
 * block of queries and keeps, per query and chunk of docs, the k largest keys ((uint32)score ^ 0x80000000) << 32 | (0xFFFFFFFF - doc);
 * k_vec_merge merges the chunks.  A key names its doc, so the rows do not depend on the order in which tiles finish. */
int32_t ss_vector_topk(ss_scorer* s, int32_t n_q, const int8_t* qvec /*[n_q][dim]*/, const int32_t* mask_id /*[n_q], NULL = all -1*/,
                       int32_t k, ss_vec_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/);

/* ss_hit_vector_scores: scores_out[q * k_in + j] = score(q, hits[q * k_in + j].doc) for j < n_hits[q]; SS_NO_VEC_SCORE for a row with
 * doc >= n_docs; rows past n_hits[q] are left untouched; only .doc of a row is read.
 * ss_rerank_hits_by_vector: ss_sort_hits_by_field with the key score(q, doc), always descending.  Defined bit for bit:
 *   Window.     As in ss_collapse_hits: hits[q * k_in .. q * k_in + n_hits[q]), in the order given; only .doc of a row is read.
 *   Order.      Rows with doc < n_docs by score(q, doc) descending, rows of equal score in window order (the sort is stable; the
 *               same doc twice is two rows).  Rows with doc >= n_docs come LAST, among themselves in window order.  No doc id makes
 *               the kernel read outside the table.
 *   Output.     With the sorted rows S_0 .. S_{n-1}: hits_out[q * k + r] = the 40 bytes of S_{first + r} (_pad included) for
 *               r < n_hits_out[q] = clamp(n - first, 0, k); scores_out[q * k + r] (nullable) = that row's score, SS_NO_VEC_SCORE for
 *               a row with doc >= n_docs.  Entries past n_hits_out[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle (or qvec / hits / n_hits / hits_out /
 * n_hits_out / scores_out of ss_hit_vector_scores with n_q > 0), n_q < 0, k_in < 1, k < 1, first < 0, hits_out overlapping hits as
 * address ranges: SS_ERR_INVALID; k_in or k above SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no vector table registered: SS_ERR_STATE;
 * n_hits[q] outside [0, k_in]: SS_ERR_INVALID when n_hits is host memory, clamped by the kernel when it is device memory.  n_q == 0
 * is SS_OK and does nothing.
 * Every pointer may be host or device memory: when all given pointers are device memory the calls only enqueue on the ctx stream and
 * NEVER wait, so score (lexical window) -> dedup -> collapse -> rerank -> explain chains on one stream; otherwise they stage through
 * blocks the scorer owns and return when the outputs are written.  Serialised on the ctx like every scoring call; no _submit /
 * _collect form. */
int32_t ss_hit_vector_scores(ss_scorer* s, int32_t n_q, const int8_t* qvec /*[n_q][dim]*/, int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/,
                             const int32_t* n_hits /*[n_q]*/, int32_t* scores_out /*[n_q][k_in]*/);
int32_t ss_rerank_hits_by_vector(ss_scorer* s, int32_t n_q, const int8_t* qvec /*[n_q][dim]*/, int32_t k_in,
                                 const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/, int32_t first, int32_t k,
                                 ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/, int32_t* scores_out /*[n_q][k], nullable*/);

/* ss_diversify_hits: a window re-ranked greedily so that every next row is chosen for its relevance minus its similarity to the rows
 * already on the page (maximal marginal relevance).  No reference counterpart.  ss_rerank_hits_by_vector and ss_hybrid_topk can put five
 * paraphrases of one page at the top: ss_dedup_hits does not see them (they share no words) and ss_collapse_hits does not (they sit
 * on different hosts).  Defined bit for bit; no float is involved:
 *   Window.     As in ss_collapse_hits: hits[q * k_in .. q * k_in + n_hits[q]), in the order given; only .doc of a row is read.  n is
 *               its length.
 *   Classes.    A row with doc < n_docs is INSIDE, a row with doc >= n_docs OUTSIDE.  Outside rows come last, among themselves in
 *               window order, as in ss_rerank_hits_by_vector.  No doc id makes a kernel read outside the table.
 *   sim(i, j)   = the sum over t < dim of (int32)vec[doc_i][t] * (int32)vec[doc_j][t] of window rows i and j, exact (|sim| <= 2^24).
 *   rel(j)      = score(q, doc_j) exactly as ss_hit_vector_scores defines it when qvec is given; -(int32)j, the window position, when
 *               qvec is NULL: that diversifies a lexical window which keeps its own order as relevance.
 *   Walk.       S starts empty.  While an inside row is unchosen: for every unchosen inside row j, pen(j) = the max over the chosen i
 *               of sim(i, j), 0 while S is empty (a negative sim is a bonus), and value(j) = (int64)w_rel * rel(j) - (int64)w_div *
 *               pen(j) (|value| < 2^42); the row of the largest value is chosen, of equal values the smaller window index j.  The same
 *               doc twice is two rows.  Only the first min(n_inside, first + k) choices are made.
 *   Output.     With R_0 .. = the chosen rows in order of choice, then the outside rows: hits_out[q * k + r] = the 40 bytes of
 *               R_{first + r} (_pad included) for r < n_hits_out[q] = clamp(n - first, 0, k); info_out[q * k + r] (nullable) = {rel, pen
 *               at the moment of choice} of that row, sim = SS_NO_VEC_SCORE for the first chosen row, {SS_NO_VEC_SCORE,
 *               SS_NO_VEC_SCORE} for an outside row.  Entries past n_hits_out[q] are left untouched.
 *   Weights.    w_rel and w_div are 16.16 fixed point in [0, SS_DIV_WEIGHT_MAX]; only their ratio matters.
 * What follows from the definition: with w_div == 0, w_rel > 0 and a qvec the rows are byte for byte those of
 * ss_rerank_hits_by_vector; with qvec == NULL and w_div == 0 the output is the window with its inside rows first, in window order.
 * A known answer: dim 64, only coordinates 0 and 1 non-zero, docs A = (10, 0), B = (9, 1), C = (0, 8), D = (5, 5), window [A, B, C, D],
 * q = (1, 0): rel = 10, 9, 0, 5; sims AB = 90, AC = 0, AD = 50, BC = 8, BD = 50, CD = 40.  w_rel = 2, w_div = 1 chooses A, C, D, B with
 * info (10, NO), (0, 0), (5, 50), (9, 90); w_div = 0 chooses A, B, D, C; qvec == NULL, w_rel = 30, w_div = 1 chooses A, C, B, D.
 * Checks, all before anything is enqueued and with the outputs untouched: those of ss_rerank_hits_by_vector, except that qvec may be
 * NULL; w_rel or w_div outside [0, SS_DIV_WEIGHT_MAX]: SS_ERR_INVALID; no vector table registered: SS_ERR_STATE.  The Gram scratch or
 * the relevance row cannot be had: SS_ERR_OOM.  n_q == 0 is SS_OK and does nothing.
 * Every pointer may be host or device memory, as in ss_rerank_hits_by_vector: with every given array on the device the call only
 * enqueues on the ctx stream and NEVER waits.  k_div_gram computes the window's Gram matrix on the int8 matrix cores (a wave per tile
 * of 64 x 64 row pairs, both operands gathered from the table by doc id, only the tiles on and above the diagonal, both halves
 * written) into a scratch block [queries of a group][pitch][pitch] of int32, pitch = k_in rounded up to 64; k_div_select, one
 * workgroup per query, makes the choices: per choice one block arg-max over the 64-bit keys (value + 2^42) << 10 | (1023 - j) and one
 * read of the chosen row of the Gram matrix.  The queries of a call run in groups whose Gram matrices fit into option
 * "div.scratch_bytes" (default 256 MB; too small for one query: one query per group), one group after another on the ctx stream.
 * Serialised on the ctx like every scoring call; no fused scoring form and no _submit / _collect form. */
#define SS_DIV_WEIGHT_MAX 65536          /* weights are 16.16 fixed point in [0, 65536] */
typedef struct ss_div_info { int32_t rel; int32_t sim; } ss_div_info;   /* 8 bytes */
int32_t ss_diversify_hits(ss_scorer* s, int32_t n_q, const int8_t* qvec /*[n_q][dim], NULLABLE*/, int32_t k_in,
                          const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/,
                          int32_t w_rel, int32_t w_div, int32_t first, int32_t k,
                          ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/, ss_div_info* info_out /*[n_q][k], nullable*/);

/* Vector lists: the docs of the vector table cut into n_lists lists around centroids (an inverted-file partition), and the search over
 * the n_probe lists nearest to a query.  No reference counterpart.  ss_vector_topk reads every doc byte for every block of queries; a
 * probed search reads the centroids and the rows of the probed lists.  It is approximate only in WHICH docs it looks at: within them
 * the answer is exact and defined bit for bit.
 *   Lists.      ss_scorer_set_vector_lists registers a partition the caller brings, as they bring the embeddings: centroids
 *               [n_lists][dim] int8 (dim = the vector table's), list_of_doc [n_docs] with every entry below n_lists or SS_NO_LIST (a doc
 *               in no list: never found by a probed search); host or device memory, copied.  n_lists = 0 or centroids NULL clears.
 *               It needs a registered vector table (SS_ERR_STATE without one) and has ss_scorer_set_doc_vectors' lifecycle: it
 *               replaces the old lists behind the scorer's outstanding work, and a call that fails leaves the old lists in place.
 *               ss_scorer_set_doc_vectors, whether it replaces or clears, drops the lists: they describe the old table.  The call may
 *               wait; it reads every entry of list_of_doc on the host: one that is >= n_lists and not SS_NO_LIST, n_lists < 0 or above
 *               SS_MAX_VEC_LISTS, a NULL list_of_doc: SS_ERR_INVALID.  Empty lists are legal.  The device sorts the docs by list
 *               (stable: ascending doc inside a list) and keeps a SECOND, list-major copy of the vector rows with the doc of every row:
 *               n_docs * dim bytes plus 4 bytes per doc on top of the doc-major table, which stays (ss_hit_vector_scores gathers from
 *               it); SS_ERR_OOM if that cannot be had.
 *   Probes.     P(q) = the first min(n_probe, n_lists) lists in the order score(q, centroid[l]) descending, then l ascending; score is
 *               the 32-bit integer dot product of ss_vector_topk.  probes_out[q * min(n_probe, n_lists) + r] (nullable) = the r-th.
 *   Candidates. Every doc d with list_of_doc[d] in P(q) that mask_id[q] allows (as ss_vector_topk: -1 / NULL = every doc).
 *   Output.     Exactly as ss_vector_topk: score descending, then doc ascending; n_hits_out[q] = min(k, number of candidates); entries
 *               past the count are left untouched.  So with n_probe >= n_lists and no doc at SS_NO_LIST the rows and counts are
 *               ss_vector_topk's, byte for byte.
 *   Assign.     ss_vector_assign_lists: list_out[d] = the list l of the largest score(vec[d], centroid[l]), ties to the lower l;
 *               score_out[d] (nullable) = that score.  The expensive half of a k-means step and the natural way to produce
 *               list_of_doc; it registers nothing and needs no lists, only the vector table (SS_ERR_STATE without one).  n_lists
 *               outside [1, SS_MAX_VEC_LISTS], NULL centroids or list_out: SS_ERR_INVALID.  It is the exact top-1 search with the
 *               centroids as the table and batches of doc rows as the queries (option "vec.assign_batch"); with every array on the
 *               device it only enqueues.
 * Checks of ss_vector_topk_probed, all before anything is enqueued and with the outputs untouched: those of ss_vector_topk, and
 * n_probe < 1: SS_ERR_INVALID; n_probe > SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no lists registered: SS_ERR_STATE.  mask_id is read on the
 * host as in ss_vector_topk; with qvec and every output on the device the call only enqueues on the ctx stream and never waits.
 * It enqueues k_vec_topk / k_vec_merge over the centroids (the probes), three small kernels that turn probes per query into runs of
 * queries per list, k_vec_topk_lists (a work item is one segment of one list times one group of up to 64 queries that probe it; a list
 * of any length is cut into segments, option "vec.list_seg_rows", so one list holding nearly every doc neither serialises nor
 * overflows) and k_vec_merge_lists.  The partial lists are bounded as in ss_vector_topk (256 MB); a call whose queries need more is
 * split into query batches on the host, still without waiting.  Serialised on the ctx like every scoring call; no _submit / _collect
 * form. */
#define SS_MAX_VEC_LISTS 65536
#define SS_NO_LIST       0xFFFFFFFFu   /* a doc in no list: never found by a probed search */
int32_t ss_scorer_set_vector_lists(ss_scorer* s, int32_t n_lists, const int8_t* centroids /*[n_lists][dim]; n_lists 0 / NULL clears*/,
                                   const uint32_t* list_of_doc /*[n_docs]: < n_lists or SS_NO_LIST*/);
int32_t ss_vector_assign_lists(ss_scorer* s, int32_t n_lists, const int8_t* centroids /*[n_lists][dim]*/, uint32_t* list_out /*[n_docs]*/,
                               int32_t* score_out /*[n_docs], nullable*/);
int32_t ss_vector_topk_probed(ss_scorer* s, int32_t n_q, const int8_t* qvec /*[n_q][dim]*/, const int32_t* mask_id /*[n_q], NULL = all -1*/,
                              int32_t k, int32_t n_probe, ss_vec_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                              uint32_t* probes_out /*[n_q][min(n_probe, n_lists)], nullable*/);

/* Hybrid search: the lexical and the vector ranking of one query fused into one ranked, paged list, and the lexical row of ANY given
 * doc.  No reference counterpart.  Until here the two rankings could only be bridged by ss_rerank_hits_by_vector, which reorders docs
 * the lexical call found: a page that matches the meaning of a query but holds none of its words never stood beside the lexical hits.
 *
 * ss_score_docs: the row that query q's ranking holds for doc d, whether or not d would reach any top-k.  Defined bit for bit:
 *   Sums.       T = the sum of (double)title_w(t, d) and B = the sum of (double)body_w(t, d) over the query's tokens IN THE ORDER GIVEN,
 *               each starting from 0.0; a token that occurs twice is added twice; a token equal to SS_UNKNOWN_TERM or at / above
 *               n_terms adds nothing; a missing posting adds nothing.  (The order of oracle_np.score_topk's np.add.at.  The merge
 *               of ss_score_topk adds a repeated token's weight times its count, in first-occurrence order and through atomics: the
 *               same value wherever those sums are exact.)
 *   Row.        title, body and final are final_rank (get_metadata.go:53-69) of T, B, the magnitudes, qmag = sqrt((double)query_len[q])
 *               (query_len NULL: the token count) and sqd; a field in which the doc has no posting of any token takes magnitude 1.0, as
 *               in the merge, so a doc with no posting at all has title = body = 0.0 and final = (0.33 * sqd + 0.0 + 0.0) * 100.0.
 *               sqd = pagerank = topic_dot in topic order; 0.0 when topic_probs is NULL or no prior is registered.
 *   Output.     hits_out[q * k_in + j] for j < n_in[q] = that row of doc docs[q * k_in + j], _pad 0.  A doc at or above n_docs gives
 *               an all-zero row with .doc set to the given id, and no table is read.  Entries past n_in[q] are left untouched.
 *   No phrases, masks or operators: those decide WHICH docs rank, not a doc's row.
 * Checks, all before anything is enqueued and with the output untouched: NULL handle or q_ptr (or docs / n_in / hits_out, or q_terms
 * with tokens, with n_q > 0), n_q < 0, k_in < 1, a q_ptr that decreases: SS_ERR_INVALID; k_in > SS_MAX_TOPK, n_q * k_in >= 2^31:
 * SS_ERR_UNSUPPORTED; n_in[q] outside [0, k_in]: SS_ERR_INVALID when n_in is host memory, clamped by the kernel when it is device
 * memory.  n_q == 0 is SS_OK and does nothing.  The query arrays (q_ptr, q_terms, query_len, topic_probs) are read on the host like
 * every query array; docs, n_in and hits_out may be host or device memory: with all three on the device the call only enqueues on the
 * ctx stream and NEVER waits, otherwise it stages through blocks the scorer owns and returns when the output is written.
 * k_score_docs: 16 lanes per (query, doc); a lane searches one (token, field) list (the merge's interpolation search), then every lane
 * of the group adds the weights found in token order: no atomics. */
int32_t ss_score_docs(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                      const double* topic_probs, int32_t k_in, const uint32_t* docs /*[n_q][k_in]*/, const int32_t* n_in /*[n_q]*/,
                      ss_hit* hits_out /*[n_q][k_in]*/);

/* ss_fuse_hits: two ranked lists of one query fused into one.  Defined bit for bit, per query q:
 *   Lists.      The lexical list is lex[q * k_lex .. + n_lex[q]), the vector list vec[q * k_vec .. + n_vec[q]), each in the order given.
 *   Ranks.      A doc's rank in a list is 1 + the position of its FIRST occurrence; later occurrences are ignored.  Rows with doc at
 *               or above n_docs are ignored but keep their position: ranks are positions.  A doc absent from a list has rank 0.
 *   Candidates. The distinct valid docs of both lists; n_union_out[q] (nullable) = their number (at most k_lex + k_vec).
 *   Rows.       Every candidate gets a full row: its ss_hit is the 40 bytes given in lex (the first occurrence) if it has a lexical
 *               rank, else the row ss_score_docs returns for it; its vec_score is the .score given in vec (the first occurrence) if it
 *               has a vector rank, else score(q, d) as ss_hit_vector_scores defines it.  Given rows are trusted, not recomputed.
 *   Score.      Every operation rounded once, nothing contracted:
 *               SS_FUSE_RRF       (lex_rank ? w_lex / (double)(rrf_c + lex_rank) : 0.0) + (vec_rank ? w_vec / (double)(rrf_c + vec_rank) : 0.0)
 *                                 (the sum rrf_c + rank in 64-bit integers);
 *               SS_FUSE_WEIGHTED  w_lex * row.final + w_vec * (double)vec_score.  The caller scales w_vec to its embedding.
 *   Order.      Score descending by numeric comparison (-0.0 ties 0.0), then doc ascending; a NaN score comes last, NaN rows by doc
 *               ascending among themselves.
 *   Output.     With the ordered candidates S_0 .. S_{n-1}: hits_out[q * k + r] = the row of S_{first + r} for r < n_hits_out[q] =
 *               clamp(n - first, 0, k), as in ss_collapse_hits; fused_out[q * k + r] (nullable) = its score, vec_score and the two
 *               ranks.  A NaN score is stored as the quiet NaN 0x7FF8000000000000, whatever operation made it; every other score as
 *               computed (-0.0 stays -0.0).  Entries past n_hits_out[q] are left untouched.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle, q_ptr or fp, n_q < 0, (with n_q > 0) NULL qvec,
 * lex, n_lex, vec, n_vec, hits_out or n_hits_out, a mode other than the two, rrf_c < 1, a w_lex or w_vec that is not finite, k_lex,
 * k_vec or k below 1, first < 0, hits_out overlapping lex as address ranges, a q_ptr that decreases: SS_ERR_INVALID; k_lex, k_vec or k
 * above SS_MAX_TOPK: SS_ERR_UNSUPPORTED; no vector table registered: SS_ERR_STATE; n_lex[q] outside [0, k_lex] or n_vec[q] outside
 * [0, k_vec]: SS_ERR_INVALID when the count array is host memory, clamped by the kernel when it is device memory.  n_q == 0 is SS_OK
 * and does nothing.  The query arrays are read on the host; qvec, the lists, their counts and the outputs may each be host or device
 * memory: with all of them on the device the call only enqueues on the ctx stream and NEVER waits, so hybrid -> dedup -> collapse ->
 * explain -> passages chains on one stream; otherwise it stages through blocks the scorer owns and returns when the outputs are
 * written.  Four launches whose sizes depend on nothing read back: k_fuse_hits (one workgroup per query: (doc, list, position) keys
 * sorted in LDS, ranks and the docs that lack a side), k_score_docs and k_vec_hit_scores over those docs, k_fuse_page (scores, the sort
 * of up to 2048 keys, the page).  Serialised on the ctx like every scoring call; no _submit / _collect form.
 *
 * ss_hybrid_topk: row q = what ss_fuse_hits returns when lex is the row ss_score_topk_masked returns for q at k = k_window (no phrase,
 * this query_len, topic_probs and mask_id[q]) and vec the row ss_vector_topk returns for q at k = k_window under the same mask_id[q].
 * Both windows stay in memory the scorer owns, as in ss_score_topk_collapsed; only the page is written.  The checks are those of
 * ss_fuse_hits (k_window in the place of k_lex and k_vec) and, behind them, those of the two calls it makes; with qvec and the outputs
 * in device memory the call never waits. */
#define SS_FUSE_RRF      0   /* reciprocal rank fusion */
#define SS_FUSE_WEIGHTED 1   /* weighted sum of FinalRank and the vector score */
typedef struct ss_fuse_params { int32_t mode; int32_t rrf_c; double w_lex; double w_vec; } ss_fuse_params;   /* 24 bytes */
typedef struct ss_fused { double score; int32_t vec_score; uint16_t lex_rank; uint16_t vec_rank; } ss_fused;   /* 16 bytes; rank 0 = absent */
int32_t ss_fuse_hits(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                     const double* topic_probs, const int8_t* qvec /*[n_q][dim]*/,
                     int32_t k_lex, const ss_hit* lex /*[n_q][k_lex]*/, const int32_t* n_lex /*[n_q]*/,
                     int32_t k_vec, const ss_vec_hit* vec /*[n_q][k_vec]*/, const int32_t* n_vec /*[n_q]*/,
                     const ss_fuse_params* fp, int32_t first, int32_t k,
                     ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                     ss_fused* fused_out /*[n_q][k], nullable*/, int32_t* n_union_out /*[n_q], nullable*/);
int32_t ss_hybrid_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                       const double* topic_probs, const int8_t* qvec /*[n_q][dim]*/, const int32_t* mask_id /*[n_q], NULL = none*/,
                       int32_t k_window, const ss_fuse_params* fp, int32_t first, int32_t k,
                       ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/,
                       ss_fused* fused_out /*[n_q][k], nullable*/, int32_t* n_union_out /*[n_q], nullable*/);

/* ---- term lexicon: cmd/server/server.go:54-85 (/wordlist/{pre}), database/database.go:414-454 (IterateInv) -------------
 * The words of forw[0] keyed by dense term id, resident on the device.  The reference answers /wordlist/{pre} by walking every key
 * of inv[0] and inv[1], fetching each word from forw[0] and testing strings.HasPrefix: a scan of the whole vocabulary per request,
 * sorted afterwards (sort.StringSlice, server.go:83).  A lexicon answers the same question from a sorted order built once, one page
 * at a time, and adds what the reference lacks: the known words within a small edit distance of a query word ("did you mean").
 * Defined bit for bit:
 *   Lexicon.   Word t is bytes[word_ptr[t] .. word_ptr[t+1]): any bytes, any length, zero included; embedded NULs are data; duplicate
 *              words with different ids are allowed.  word_ptr must start at 0 and never decrease (SS_ERR_INVALID); 2^32 bytes or
 *              more, or 2^32 terms or more, is SS_ERR_UNSUPPORTED.  Inputs host or device memory, copied.  The lexicon is immutable
 *              apart from freq: after an index update that adds terms the caller destroys it and creates it again, as with scorers.
 *              freq[t] is whatever popularity the caller wants (the host mirror passes title list length + body list length,
 *              saturated at 2^32 - 1); NULL = all 0.
 *   Order.     The sort order is the permutation of 0 .. n_terms-1 that sorts the words as arrays of UNSIGNED bytes,
 *              lexicographically, a proper prefix first (Go's string <, what sort.StringSlice produces); equal words by ascending
 *              term id.  Built once at create, a pure function of the input; ss_lexicon_read_order returns it (host or device).
 *   Prefix.    Row q's matches are the terms whose word starts with prefix q = p_bytes[p_ptr[q] .. p_ptr[q+1]) (the empty prefix
 *              matches every term).  n_match_out[q] (nullable) = the number of matches; terms_out[q * k + r] = match number
 *              first + r in sort order for r < n_out[q] = clamp(n_match - first, 0, k).  Entries past n_out[q] are left untouched.
 *              The reference ships the whole sorted list; the paging is ours.
 *   Distance.  d(a, b) = the optimal-string-alignment distance over BYTES (not code points): unit-cost insert, delete, substitute
 *              and swap of two ADJACENT bytes.  D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1,
 *              D[i-1][j-1] + (a[i-1] != b[j-1]), and, if i, j >= 2 and a[i-1] == b[j-2] and a[i-2] == b[j-1], D[i-2][j-2] + 1).
 *              d("ab", "ba") = 1; d("ca", "abc") = 3 (not 2: this is not the unrestricted Damerau distance).
 *   Suggest.   The candidates of row q (query word w_bytes[w_ptr[q] .. w_ptr[q+1])) are the terms t with len(word t) <=
 *              SS_MAX_WORD_BYTES, freq[t] >= min_freq and d(query word, word t) <= max_dist; distance 0 is included, so the caller
 *              sees that a word is known.  A query word longer than SS_MAX_WORD_BYTES has no candidates: defined, not an error.
 *              Row q of terms_out [n_q][m] / dist_out [n_q][m] (nullable) holds the first n_out[q] = min(m, #candidates) candidates
 *              ordered by distance ascending, then freq descending, then term id ascending.  Entries past n_out[q] are left
 *              untouched.  The row does not depend on the order in which workgroups finish: there are no atomics.
 *   Complete.  "Of the words that start with what was typed, the most used" (no reference counterpart).  Row q's matches are exactly
 *              those of Prefix: the terms whose word starts with prefix q, a contiguous range [lb, ub) of positions in the sort
 *              order; n_match_out[q] (nullable) = ub - lb, whatever min_freq is.  The candidates are the matches with freq >=
 *              min_freq, ordered by freq descending, then by sort position ascending (the word in Go string order, equal words by
 *              term id): by the single 64-bit key (~freq << 32) | position, ascending.  No two candidates have the same key, so the
 *              row is a pure function of the input.  n_out[q] = min(m, #candidates); terms_out[q * m + r] = the term id of the
 *              r-th candidate and freq_out[q * m + r] (nullable) its freq, for r < n_out[q].  Entries past n_out[q] are left
 *              untouched.  No atomics, no dependence on the order in which workgroups finish.  By hand: the words (id 0 .. 5)
 *              "car", "cat", "ca", "dog", "cat", "cab" with freq 5, 9, 5, 100, 9, 0 sort as ca, cab, car, cat (1), cat (4), dog =
 *              ids 2, 5, 0, 1, 4, 3.  Prefix "ca", min_freq 1, m 3: range [0, 5), n_match 5, row ids 1, 4, 2 with freq 9, 9, 5
 *              ("ca" before "car": equal freq, earlier position), n_out 3; m 64: ids 1, 4, 2, 0, n_out 4 ("cab" has freq 0 < 1);
 *              min_freq 0: "cab" comes last, n_out 5; min_freq 10: n_out 0, n_match still 5; prefix "" with m 1: id 3 ("dog");
 *              prefix "cow": n_match 0, n_out 0.  With every freq equal the row is that of Prefix with first 0 and k = m.
 * Checks, all before anything is enqueued and with the outputs untouched: NULL handle or NULL required output (terms_out, n_out) or
 * pointer array, n_q < 0, a p_ptr / w_ptr that decreases (as q_ptr in ss_score_topk), k < 1, m < 1, first < 0, max_dist < 0:
 * SS_ERR_INVALID; k > SS_MAX_TOPK, m > SS_MAX_SUGGEST (SS_MAX_COMPLETE for Complete), max_dist > SS_MAX_EDIT_DIST:
 * SS_ERR_UNSUPPORTED.  n_q == 0 is SS_OK and does
 * nothing; every call on a lexicon of 0 terms is SS_OK: the rows come back empty and n_out is written as 0.
 * Query bytes and pointers are read on the host like every query array.  Outputs may each be host or device memory: when all given
 * outputs are device memory the call only enqueues on the ctx stream and NEVER waits (the queries go up through turns of pinned
 * blocks the lexicon owns); otherwise it stages through blocks the lexicon owns and returns when the outputs are written.
 * ss_lexicon_suggest compares every query word with every word of the length groups len - max_dist .. len + max_dist, one workgroup
 * per (query word, chunk of option "lexicon.chunk_terms" words, default 4096, 1 .. 2^20); its temporaries are sized by m * chunks,
 * never by the number of candidates.  ss_lexicon_complete cuts the range of every prefix into the same number P of near-equal parts,
 * one workgroup per (prefix, part), each streaming its part of the frequencies held in sort order (4 B per term); P comes from n_q
 * alone (about 4096 workgroups per call and at most 64 per prefix; option "lexicon.complete_parts" forces 1 .. 256), so its temporaries are
 * n_q * P * m keys, never sized by a range.  The rows are the same bytes for every P.
 * Calls are serialised on the ctx like the scoring calls; there is no _submit / _collect form. */
#define SS_MAX_WORD_BYTES 64   /* longest word that can be a suggestion candidate or a suggest query */
#define SS_MAX_EDIT_DIST  3
#define SS_MAX_SUGGEST    64
#define SS_MAX_COMPLETE   64
typedef struct ss_lexicon ss_lexicon;

int32_t ss_lexicon_create(ss_ctx* ctx, uint64_t n_terms, const uint64_t* word_ptr /*[n_terms+1]*/, const uint8_t* bytes,
                          const uint32_t* freq /*[n_terms], NULL = all 0*/, ss_lexicon** out);
int32_t ss_lexicon_set_freq(ss_lexicon* lx, const uint32_t* freq /*[n_terms], NULL = all 0*/);
int32_t ss_lexicon_get_info(const ss_lexicon* lx, uint64_t* n_terms, uint64_t* n_bytes);
int32_t ss_lexicon_read_order(ss_lexicon* lx, uint32_t* order_out /*[n_terms]*/);
int32_t ss_lexicon_destroy(ss_lexicon* lx);

int32_t ss_lexicon_prefix(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr /*[n_q+1]*/, const uint8_t* p_bytes,
                          int64_t first, int32_t k, uint32_t* terms_out /*[n_q][k]*/, int32_t* n_out /*[n_q]*/,
                          uint64_t* n_match_out /*[n_q] nullable*/);

int32_t ss_lexicon_suggest(ss_lexicon* lx, int32_t n_q, const uint32_t* w_ptr /*[n_q+1]*/, const uint8_t* w_bytes,
                           int32_t max_dist, uint32_t min_freq, int32_t m,
                           uint32_t* terms_out /*[n_q][m]*/, int32_t* dist_out /*[n_q][m] nullable*/, int32_t* n_out /*[n_q]*/);

int32_t ss_lexicon_complete(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr /*[n_q+1]*/, const uint8_t* p_bytes,
                            uint32_t min_freq, int32_t m,
                            uint32_t* terms_out /*[n_q][m]*/, uint32_t* freq_out /*[n_q][m] nullable*/,
                            int32_t* n_out /*[n_q]*/, uint64_t* n_match_out /*[n_q] nullable*/);

/* Doc-range-sharded scoring: every shard scores the same query batch against its own doc range
 * (ss_score_topk, local doc ids) and the host gathers the lists.  ss_merge_hits returns the k best
 * of the union per query in the order of appendSort (util.go:48-54) and the cut of
 * main_retrieve.go:99-103 — identical to scoring the unsharded index.
 * parts [n_parts][n_q][k], n_hits [n_parts][n_q] (the all-gathered outputs of ss_score_topk),
 * doc_base [n_parts] first corpus doc id of each shard (NULL = ids already global);
 * hits_out [n_q][k], n_hits_out [n_q].  All pointers host or device. */
#define SS_MAX_SHARDS 64
int32_t ss_merge_hits(ss_ctx* ctx, int32_t n_q, int32_t n_parts, int32_t k, const ss_hit* parts,
                      const int32_t* n_hits, const uint32_t* doc_base, ss_hit* hits_out, int32_t* n_hits_out);

/* Timing hook for bench.py: milliseconds between the start and end HIP events
 * recorded on the ctx stream around the LAST compute call of the given kind
 * (0 = ss_pr_step batch, 1 = ss_score_topk, 2 = ss_tfidf_build). */
int32_t ss_last_kernel_ms(ss_ctx* ctx, int32_t kind, float* ms_out);

/* Token vectors: late interaction (MaxSim).  Every call above sees a doc as one point (ss_scorer_set_doc_vectors); here a doc keeps one
 * signed 8-bit vector per token or passage, a query does too, and a doc's score is the sum, over the query's token vectors, of the
 * best dot product any of the doc's token vectors achieves.  It is a second stage: it scores or re-ranks a window that ss_score_topk*,
 * ss_vector_topk[_probed] + ss_score_docs or ss_hybrid_topk produced.  No reference counterpart.
 * The table: tok_ptr [n_docs + 1] (n_docs = the scorer's) and tok [tok_ptr[n_docs]][dim], the tokens of doc d at rows tok_ptr[d] ..
 * tok_ptr[d + 1]; host or device memory, both copied.  dim is a multiple of 64 in [64, SS_MAX_VEC_DIM]; dim = 0 or tok = NULL clears
 * the table.  It is independent of ss_scorer_set_doc_vectors' table (its own dim; neither call touches the other's table) and has that
 * call's lifecycle: a new table replaces the old one after the scorer's outstanding work has finished with it, it lives as long as
 * the scorer, and a call that fails leaves the old table in place.  tok_ptr is checked on the host, so the call may wait: NULL
 * tok_ptr (unless the call clears), tok_ptr[0] != 0, a decreasing entry or a bad dim: SS_ERR_INVALID; a doc of 2^31 or more tokens:
 * SS_ERR_UNSUPPORTED.  tok_ptr[n_docs] * dim bytes + 8 per doc: SS_ERR_OOM if that cannot be had.  Every int8 value is an ordinary
 * value, -128 included; a doc may have no token.
 * Defined bit for bit, with T_d = tok_ptr[d + 1] - tok_ptr[d] and m_q = qt_ptr[q + 1] - qt_ptr[q]:
 *   dot(q, i, d, t) = the sum over c < dim of (int32)qtok[qt_ptr[q] + i][c] * (int32)tok[tok_ptr[d] + t][c]
 *   maxsim(q, d)    = the sum over i < m_q of the max over t < T_d of dot(q, i, d, t), in exact 32-bit integer arithmetic
 *                     (|maxsim| <= SS_MAX_QUERY_TOKENS * 2^24 = 2^30).  m_q == 0 gives 0.  A doc with T_d == 0, or doc >= n_docs, has NO
 *                     score: SS_NO_VEC_SCORE (never a real score).  A token a doc does not have is never a zero vector: with every
 *                     dot product negative the score is negative.
 * ss_hit_maxsim_scores is ss_hit_vector_scores with that score: scores_out[q * k_in + j] = maxsim(q, hits[q * k_in + j].doc) for
 * j < n_hits[q], SS_NO_VEC_SCORE for a row without a score; rows past n_hits[q] are left untouched; only .doc of a row is read.
 * ss_rerank_hits_by_maxsim is ss_rerank_hits_by_vector with that score, its Window, Order and Output word for word: stable and paged
 * (first, k), rows of equal score in window order, the same doc twice is two rows, rows without a score LAST in window order, the 40
 * bytes of a row carried through (_pad included), scores_out[q * k + r] (nullable) the row's score, entries past n_hits_out[q] left
 * untouched.
 * Two consequences.  (1) With a token table of exactly one token per doc, equal to its doc vector, and one token per query, both
 * calls return the bytes of ss_hit_vector_scores / ss_rerank_hits_by_vector.  (2) By hand, dim 64 with only coordinates 0 and 1
 * non-zero: docs A = {(10,0), (0,3)}, B = {(4,4)}, C = {} and D = {(-5,-5), (-1,-9)}, query tokens {(1,0), (0,2)}: A = max(10, 0) +
 * max(0, 6) = 16, B = 4 + 8 = 12, D = max(-5, -1) + max(-10, -18) = -11 (not 0: no padded lane counts), C none.  The window [D, C, B,
 * A, doc 99] of that 4-doc table re-ranks to A, B, D, C, 99 with scores 16, 12, -11, SS_NO_VEC_SCORE, SS_NO_VEC_SCORE.
 * Checks of the two scoring calls, all before anything is enqueued and with the outputs untouched: those of ss_hit_vector_scores /
 * ss_rerank_hits_by_vector (with qt_ptr and qtok in qvec's place; qtok may be NULL when qt_ptr[n_q] == qt_ptr[0]); a decreasing qt_ptr:
 * SS_ERR_INVALID; an m_q above SS_MAX_QUERY_TOKENS: SS_ERR_UNSUPPORTED; no token table registered: SS_ERR_STATE.  n_q == 0 is SS_OK
 * and does nothing.
 * qt_ptr is read on the host like q_ptr of the scoring calls (a device pointer costs one blocking copy).  Every other pointer may be
 * host or device memory: when all of them are device memory the calls only enqueue on the ctx stream and NEVER wait (qt_ptr goes up
 * through a pinned block the scorer owns); otherwise they stage through blocks the scorer owns and return when the outputs are
 * written.  qtok that is host memory or not 16-byte aligned is copied into a block the scorer owns, as qvec is.
 * k_maxsim_scores<QT> (QT = 1, 2, 4 tiles of 16 query-token slots, from the call's largest m_q): a workgroup of four waves belongs to
 * one query and a run of its window rows and holds the query's token vectors in LDS; a wave takes a row at a time and multiplies the
 * doc's tokens, 64 per step straight from memory, with the query tiles on the int8 matrix cores
 * (__builtin_amdgcn_mfma_i32_16x16x64_i8), keeps a running max per query token with slots past T_d held at INT32_MIN, and sums the
 * maxima of the slots below m_q.  A row whose doc has at least option "maxsim.wide_tokens" tokens (default 1024) is shared by the four
 * waves, whose maxima are joined by integer max: the scores are the same bytes for every value.  No float, no atomics.  The re-rank
 * sorts with ss_rerank_hits_by_vector's kernel.  Serialised on the ctx like every scoring call; no _submit / _collect form. */
#define SS_MAX_QUERY_TOKENS 64
int32_t ss_scorer_set_doc_tokens(ss_scorer* s, int32_t dim, const uint64_t* tok_ptr /*[n_docs+1]*/, const int8_t* tok /*[tok_ptr[n_docs]][dim]; dim 0 / NULL clears*/);
int32_t ss_hit_maxsim_scores(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr /*[n_q+1]*/, const int8_t* qtok /*[qt_ptr[n_q]][dim]*/,
                             int32_t k_in, const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/, int32_t* scores_out /*[n_q][k_in]*/);
int32_t ss_rerank_hits_by_maxsim(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr /*[n_q+1]*/, const int8_t* qtok /*[qt_ptr[n_q]][dim]*/, int32_t k_in,
                                 const ss_hit* hits /*[n_q][k_in]*/, const int32_t* n_hits /*[n_q]*/, int32_t first, int32_t k,
                                 ss_hit* hits_out /*[n_q][k]*/, int32_t* n_hits_out /*[n_q]*/, int32_t* scores_out /*[n_q][k], nullable*/);

/* ss_maxsim_topk: a first stage of its own for token vectors: the exact top k of every query by maxsim(q, d) over ALL docs of the token
 * table, not a re-rank of a window and not an approximate search.  No reference counterpart.  Defined bit for bit, with maxsim(q, d),
 * T_d and m_q as above:
 *   Candidates. Every doc d < n_docs with T_d >= 1 in the REGISTERED allow-list mask_id[q] (ss_scorer_set_doc_masks; -1 = every doc;
 *               mask_id NULL = all -1).  A doc without tokens is never a candidate and never a row: no row carries SS_NO_VEC_SCORE.
 *   Order.      maxsim(q, d) descending, then d ascending.
 *   Output.     Row q = the first n_hits_out[q] = min(k, number of candidates) rows of that order as ss_vec_hit; entries past that are
 *               left untouched.
 *   Empty query. m_q == 0 scores every candidate 0: its row is the first k candidates by doc id.
 * Three consequences.  (1) Row q equals ss_hit_maxsim_scores over all docs of the mask, sorted by (score descending, doc ascending),
 * rows without a score dropped, cut at k.  (2) With a token table of exactly one token per doc, equal to its doc vector, and one token
 * per query, the call returns the bytes of ss_vector_topk under the same masks and k.  (3) The known world above (docs A, B, D, and C
 * without tokens) gives at k = 4 n_hits = 3 and the rows (A, 16), (B, 12), (D, -11).
 * Checks, all before anything is enqueued and with the outputs untouched: those of ss_vector_topk (NULL handle, hits_out / n_hits_out
 * NULL with n_q > 0, n_q < 0, k < 1, a mask_id below -1 or at / above n_masks: SS_ERR_INVALID) and NULL qt_ptr with n_q > 0, a decreasing
 * qt_ptr, qtok NULL when the call has a query token: SS_ERR_INVALID; k > SS_MAX_TOPK, an m_q above SS_MAX_QUERY_TOKENS, more blocks of
 * queries (65535) or chunks than one launch holds, a query whose token image, k + 64 candidate keys and the select's scratch exceed the
 * LDS of a workgroup: SS_ERR_UNSUPPORTED; no token table registered: SS_ERR_STATE; the chunks' partial lists (n_q * chunks * k * 8 bytes,
 * bounded by 256 MB unless option "maxsim.chunk_tokens" asks for more chunks) cannot be had: SS_ERR_OOM.  n_q == 0 is SS_OK and does
 * nothing — on a scorer that has a token table: as in ss_hit_maxsim_scores and ss_vector_topk the table is asked for first, so without
 * one n_q == 0 is SS_ERR_STATE too.  qtok may be NULL when the call has no query token.
 * qt_ptr and mask_id are read on the host, as in the sibling calls (a device pointer costs one blocking copy).  qtok and the outputs
 * may be host or device memory: with all of them on the device the call only enqueues on the ctx stream and NEVER waits — its plan
 * uses only what the host knew when the table was registered (a cut table: the first doc at or behind every 64th token) — otherwise
 * it stages through blocks the scorer owns and returns when the outputs are written.  The rows are what ss_score_docs takes:
 * ss_maxsim_topk -> ss_score_docs -> ss_dedup_hits -> ss_explain_hits stays on one stream.
 * k_maxsim_topk<QT> (maxsim_topk.hip; QT as in k_maxsim_scores): a workgroup of four waves owns a block of 16 / 8 / 4 / 2 / 1 queries —
 * the most whose token images, candidate lists and the select's scratch fit the LDS — and a chunk of consecutive docs cut at doc
 * boundaries by token count.  A wave takes a doc at a time, loads each 16-token tile of it once, as the doc has them, and multiplies
 * it on the int8 matrix cores with the token tiles of every query of the block that may take the doc: the table is read once per block
 * of queries.  A doc without tokens, or that no query of the block may take, costs no load.  A doc of at least "maxsim.wide_tokens"
 * tokens is shared by the four waves.  Keys, lists, select and merge are ss_vector_topk's: a key names its doc, so the rows do not
 * depend on which wave finishes first, nor on either option.  Serialised on the ctx like every scoring call; no _submit / _collect form. */
int32_t ss_maxsim_topk(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr /*[n_q+1]*/, const int8_t* qtok /*[qt_ptr[n_q]][dim]*/,
                       const int32_t* mask_id /*[n_q], NULL = all -1*/, int32_t k, ss_vec_hit* hits_out /*[n_q][k]*/,
                       int32_t* n_hits_out /*[n_q]*/);

#ifdef __cplusplus
}
#endif
#endif
