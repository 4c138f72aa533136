// score_call.hip — the host side of one scoring call (ss_score_topk and its variants, ss_score_topk_submit / _collect).
//
// A call runs under the context's lock as a row of steps, each with its own result struct:
//   fetch_filter_inputs / fetch_inputs   the caller's arrays copied to the host and checked          -> BatchInputs
//   resolve_constraints                  required / excluded terms, range clauses -> one allowed set per combination -> ConstraintPlan
//   plan_batch                           phrase parts, kernel per query, slices, launch order         -> BatchPlan
//   choose_route                         which kernels share which streams                            -> Route
//   stage_plan                           the plan into this turn's pinned buffer, workspaces, params  -> StagedBatch
//   enqueue                              upload, launches, the events between the streams
//   read_back                            host outputs only
// resolve_constraints and plan_batch are plain host arithmetic: no HIP call, no write to the scorer or the context; what they
// read of the scorer is a ScorerView, of the options a ScoreOptions, and an error comes back as a PlanError.  Everything up to and
// including plan_batch can fail on the caller's input, and nothing before stage_plan enqueues work, takes a turn or touches
// the outputs: a call that fails there leaves no trace.
// The kernels are in score.hip, score_wave.hip, score_small.hip, constraint.hip and field.hip, behind the launchers of scorer.hpp.
#include <chrono>
#include <tuple>
#include "scorer.hpp"

namespace {

using Clock = std::chrono::steady_clock;

struct CallArgs {
    int32_t n_q;
    const uint32_t *q_ptr, *q_terms, *p_ptr, *p_terms;
    const int32_t* query_len;
    const double* topic_probs;
    int32_t k;
    ss_hit* hits_out;
    int32_t* n_hits_out;
    const int32_t* mask_id;
    const QueryConstraints* cons;
    TurnRows* turn_rows;                        // ss::score_into_turn: the rows go to the plan turn's own block (hits_out / n_hits_out unused)
    const QueryRanges* ranges;                  // ss_score_topk_filtered
};

// the options a call reads, each looked up once per call, in one place (a look-up builds a std::string key)
constexpr int64_t OPT_UNSET = INT64_MIN;    // options whose default is computed from the batch
struct ScoreOptions {
    bool trace, timed, grade_slices, wave, pipeline_slices, separate_merge;
    int64_t pipeline, slice_target, wave_slice_target, wave_big_pct, wave_big_x100, wave_small_x100, wave_max_terms, wave_min_list,
        wave_share_pct, small, small_cap, small_batch, small_max_batch;
};
ScoreOptions read_options(const ss_ctx* ctx) {
    ScoreOptions o{};
    o.trace = ctx->opt("score.trace", 0) != 0;
    o.timed = ctx->opt("score.timing", 1) != 0;       // the two timing events of ss_last_kernel_ms(1) (each costs the stream a few us)
    o.grade_slices = ctx->opt("score.grade_slices", 0) != 0;
    o.wave = ctx->opt("score.wave", 1) != 0;
    o.pipeline = ctx->opt("score.pipeline", 2);
    o.pipeline_slices = ctx->opt("score.pipeline_slices", 1) != 0;
    o.separate_merge = ctx->opt("score.separate_merge", 0) != 0;
    o.slice_target = ctx->opt("score.slice_target", OPT_UNSET);             // experiments only
    o.wave_slice_target = ctx->opt("score.wave_slice_target", OPT_UNSET);
    // (85 / 115 / 40 suited one batch at a time; with consecutive batches overlapping the next batch's kernel fills this one's tail
    //  and fewer, larger tail slices pay: 0.334-0.338 ms per batch at config 3 against 0.341-0.345, `tools/score_wall.py` with OPTS)
    o.wave_big_pct = ctx->opt("score.wave_big_pct", 92);
    o.wave_big_x100 = ctx->opt("score.wave_big_x100", 115);
    o.wave_small_x100 = ctx->opt("score.wave_small_x100", 60);
    o.wave_max_terms = ctx->opt("score.wave_max_terms", 6);
    o.wave_min_list = ctx->opt("score.wave_min_list", 16);
    o.wave_share_pct = ctx->opt("score.wave_share_pct", 90);
    o.small = ctx->opt("score.small", 2);
    o.small_cap = ctx->opt("score.small_cap", ss::score_small_cap());
    o.small_batch = ctx->opt("score.small_batch", 0);
    o.small_max_batch = ctx->opt("score.small_max_batch", 64);
    return o;
}

// what the planning steps may see of the scorer and its context
struct ScorerView {
    uint64_t n_docs, n_terms;
    const std::vector<uint64_t>& tp;              // the title and body tables' term_ptr (host copies)
    const std::vector<uint64_t>& bp;
    const std::vector<double>& prior_max;
    const std::vector<double>& prior_min;
    bool has_combined, clean, prior_clean;
    int cu_count;
};

// an error of a planning step: the driver hands it to ss_ctx::fail
struct PlanError {
    char msg[256];
    __attribute__((format(printf, 3, 4))) int32_t set(int32_t code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        return code;
    }
};

struct BatchInputs {
    int32_t n_q = 0, k = 0;
    int K = 0;                                  // the prior's topics
    bool has_mask_arg = false, has_constraints = false, has_phrase_arg = false, has_probs = false;
    bool has_ranges = false;                    // a query of the call has a range clause (ss_score_topk_filtered)
    std::vector<uint32_t> rng_ptr;
    std::vector<ss_doc_range> rng;
    bool any_mask = false;                      // a query of the call has an allow-list (registered, or a set of resolve_constraints)
    bool dev_out = false;                       // both outputs live in device memory
    uint32_t n_tok = 0;
    std::vector<int32_t> mask;                  // [n_q] allow-list of the query, -1: none (empty without mask ids and constraints)
    std::vector<uint32_t> req_ptr, req_terms, exc_ptr, exc_terms;
    std::vector<uint32_t> qptr, terms, pptr, pterms;
    std::vector<int32_t> qlen;
    std::vector<double> probs;
};

struct ConstraintPlan {
    std::vector<ConstraintSet> sets;
    std::vector<ConstraintTerm> terms;
    // range clauses: the sets k_field_masks writes or narrows, in groups.  The last n_field_only sets have clauses and no terms:
    // k_constraint_masks leaves them out and k_field_masks builds them from the registered allow-list.
    std::vector<FieldSet> fsets;
    std::vector<ss_doc_range> fclauses;
    std::vector<uint32_t> fgroups;
    size_t n_field_only = 0;
};

struct SmallEnt { SmallHdr h; uint32_t loff; };
struct BatchPlan {
    bool exact_all = false, any_phrase = false, small_batch = false;
    int kth_j = 0, cb = 0, cb_flat = 0;
    std::vector<uint32_t> pdrv, xoff, pbase;
    std::vector<uint4> parts;                   // k_phrase_match work: {query, pass, first candidate, candidates}
    std::vector<uint8_t> fast;                  // [n_q] bit 0: k_score_wave, bit 1: k_score_small
    std::vector<SmallEnt> small_a, small_b;     // by table size: up to score_small_cap_a() postings, and beyond
    std::vector<SmallList> small_lists;
    uint32_t small_lmax = 0;
    std::vector<uint32_t> qoff, dterm, dmult, sbase, order, mergeq;
    std::vector<double> qmag, ub;
    std::vector<SliceDesc> slices;
    size_t n_small_a = 0, n_small_b = 0, n_small = 0, small_stride = 0, n_slices = 0, n_fast_slices = 0, n_d = 0;
};

// Filled in two steps: the flags by choose_route, from the plan alone, before anything is staged (stage_plan reads only the
// flags); the four streams by bind_streams inside enqueue, because taking a wave stream advances the scorer's wave_turn and
// a call that fails while staging must not have done that.  The streams are null until then.
struct Route {
    bool pipe, pipe_s, pipe_split, fused, small_staged, small_side, small_alone;
    hipStream_t st;          // the caller's stream: every kernel that writes hits
    hipStream_t wst;         // where k_wave_prep / k_score_wave go
    hipStream_t sst;         // ... and k_score_slices (with the phrase kernels in front of it)
    hipStream_t small_st;    // ... and k_score_small
};

struct StagedBatch {
    int turn = 0;
    size_t plan_bytes = 0, res_rows = 0, res_bytes = 0;
    uint64_t set_stride = 0;
    bool one_copy = false;
    ScoreParams p{};
    ConstraintParams cp{};
    FieldParams fp{};
};

struct Stamps { Clock::time_point begin, fetched, planned, staged, uploaded; };   // "score.trace"

// ---- 1. the caller's arrays ------------------------------------------------------------------------------------------------
// The first checks, the mask ids and the constraint arrays.  (Apart from the rest of the inputs: the constraints are resolved,
// and can be refused, before the queries are looked at.)
int32_t fetch_filter_inputs(ss_scorer* s, const CallArgs& a, BatchInputs& in) {
    ss_ctx* ctx = s->ctx;
    const int32_t n_q = a.n_q;
    if (n_q < 0 || !a.q_ptr || (!a.turn_rows && (!a.hits_out || !a.n_hits_out))) return ctx->fail(SS_ERR_INVALID, "ss_score_topk: NULL argument or n_q < 0");
    if (a.k < 1) return ctx->fail(SS_ERR_INVALID, "ss_score_topk: k < 1");
    if (a.k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_score_topk: k %d > SS_MAX_TOPK %d", a.k, SS_MAX_TOPK);
    if (a.topic_probs && s->k_topics == 0) return ctx->fail(SS_ERR_STATE, "ss_score_topk: topic_probs given but no prior set (ss_scorer_set_prior)");
    in.n_q = n_q;
    in.k = a.k;
    if (n_q == 0) return SS_OK;
    // allow-lists (ss_score_topk_masked): checked before anything is enqueued; a call without a masked query is the unmasked call
    in.has_mask_arg = a.mask_id != nullptr;
    if (a.mask_id) {
        in.mask.resize(n_q);
        SS_HIP(ctx, ss::copy_in(ctx->stream, in.mask.data(), a.mask_id, n_q * sizeof(int32_t)));
        for (int q = 0; q < n_q; q++) {
            if (in.mask[q] < -1 || in.mask[q] >= s->n_masks)
                return ctx->fail(SS_ERR_INVALID, "ss_score_topk_masked: query %d has mask id %d (the scorer has %d masks)", q, in.mask[q], s->n_masks);
            in.any_mask = in.any_mask || in.mask[q] >= 0;
        }
    }
    // query operators (ss_score_topk_constrained): required / excluded terms, checked here too
    // range clauses (ss_score_topk_filtered), checked here too; a call without a clause is the constrained call
    if (a.ranges && a.ranges->rng_ptr) {
        const char* const entry = "ss_score_topk_filtered";
        in.rng_ptr.resize(n_q + 1);
        SS_TRY(fetch_ptr_array(ctx, entry, "rng", a.ranges->rng_ptr, (size_t)n_q, in.rng_ptr.data()));
        if (in.rng_ptr[0] != 0) return ctx->fail(SS_ERR_INVALID, "%s: rng_ptr[0] is %u, not 0", entry, in.rng_ptr[0]);
        const size_t n_cl = in.rng_ptr[n_q];
        if (n_cl && !a.ranges->rng) return ctx->fail(SS_ERR_INVALID, "%s: rng is NULL", entry);
        for (int q = 0; q < n_q; q++)
            if (in.rng_ptr[q + 1] - in.rng_ptr[q] > SS_MAX_RANGE_CLAUSES)
                return ctx->fail(SS_ERR_UNSUPPORTED, "%s: query %d has %u range clauses (max %d)", entry, q, in.rng_ptr[q + 1] - in.rng_ptr[q], SS_MAX_RANGE_CLAUSES);
        if (n_cl && s->n_fields == 0) return ctx->fail(SS_ERR_STATE, "%s: no field table registered (ss_scorer_set_doc_fields)", entry);
        in.rng.resize(n_cl);
        if (n_cl) SS_HIP(ctx, ss::copy_in(ctx->stream, in.rng.data(), a.ranges->rng, n_cl * sizeof(ss_doc_range)));
        for (size_t c = 0; c < n_cl; c++)
            if (in.rng[c].field < 0 || in.rng[c].field >= s->n_fields)
                return ctx->fail(SS_ERR_INVALID, "%s: clause %zu names field %d (the scorer has %d fields)", entry, c, in.rng[c].field, s->n_fields);
        in.has_ranges = n_cl > 0;
    }
    in.has_constraints = a.cons && (a.cons->req_ptr || a.cons->exc_ptr);
    if (!in.has_constraints && !in.has_ranges) return SS_OK;
    in.req_ptr.assign(n_q + 1, 0);
    in.exc_ptr.assign(n_q + 1, 0);
    if (!in.has_constraints) return SS_OK;
    auto load = [&](const uint32_t* ptr, const uint32_t* terms, std::vector<uint32_t>& hp, std::vector<uint32_t>& ht, const char* what) -> int32_t {
        if (!ptr) return SS_OK;
        SS_TRY(fetch_ptr_array(ctx, "ss_score_topk_constrained", what, ptr, (size_t)n_q, hp.data()));
        if (hp[0] != 0) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_constrained: %s_ptr[0] is %u, not 0", what, hp[0]);
        ht.resize(hp[n_q]);
        if (hp[n_q] && !terms) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_constrained: %s_terms is NULL", what);
        if (hp[n_q]) SS_HIP(ctx, ss::copy_in(ctx->stream, ht.data(), terms, ht.size() * sizeof(uint32_t)));
        return SS_OK;
    };
    SS_TRY(load(a.cons->req_ptr, a.cons->req_terms, in.req_ptr, in.req_terms, "req"));
    return load(a.cons->exc_ptr, a.cons->exc_terms, in.exc_ptr, in.exc_terms, "exc");
}

// The queries, their phrase parts, lengths and topic probabilities.
int32_t fetch_inputs(ss_scorer* s, const CallArgs& a, BatchInputs& in) {
    ss_ctx* ctx = s->ctx;
    const int32_t n_q = a.n_q;
    in.qptr.resize(n_q + 1);
    SS_TRY(fetch_ptr_array(ctx, "ss_score_topk", "q", a.q_ptr, (size_t)n_q, in.qptr.data()));
    const uint32_t n_tok = in.n_tok = in.qptr[n_q];
    if (n_tok && !a.q_terms) return ctx->fail(SS_ERR_INVALID, "ss_score_topk: q_terms is NULL");
    in.terms.resize(n_tok);
    if (n_tok) SS_HIP(ctx, ss::copy_in(ctx->stream, in.terms.data(), a.q_terms, n_tok * sizeof(uint32_t)));
    // phrase part (retrieval/phrase.go): tokens of all quoted phrases of a query, concatenated
    in.has_phrase_arg = a.p_ptr != nullptr;
    in.pptr.assign(n_q + 1, 0);
    if (a.p_ptr) {
        if (!s->title->pos_ptr.p || !s->body->pos_ptr.p)
            return ctx->fail(SS_ERR_STATE, "ss_score_topk_phrase: positional postings not loaded (ss_index_set_positions on both tables)");
        SS_TRY(fetch_ptr_array(ctx, "ss_score_topk_phrase", "p", a.p_ptr, (size_t)n_q, in.pptr.data()));
        in.pterms.resize(in.pptr[n_q]);
        if (in.pptr[n_q]) {
            if (!a.p_terms) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_phrase: p_terms is NULL");
            SS_HIP(ctx, ss::copy_in(ctx->stream, in.pterms.data(), a.p_terms, in.pterms.size() * sizeof(uint32_t)));
        }
    }
    in.qlen.resize(n_q);
    if (a.query_len) SS_HIP(ctx, ss::copy_in(ctx->stream, in.qlen.data(), a.query_len, n_q * sizeof(int32_t)));
    else for (int q = 0; q < n_q; q++)     // len(queryTokenised)+len(phraseTokenised), main_retrieve.go:90
        in.qlen[q] = (int32_t)(in.qptr[q + 1] - in.qptr[q]) + (int32_t)(in.pptr[q + 1] - in.pptr[q]);
    in.K = s->k_topics;
    in.has_probs = a.topic_probs != nullptr;
    if (a.topic_probs) {
        in.probs.resize((size_t)n_q * in.K);
        SS_HIP(ctx, ss::copy_in(ctx->stream, in.probs.data(), a.topic_probs, in.probs.size() * sizeof(double)));
    }
    return SS_OK;
}

// results straight into the caller's buffers when both live in device memory (then the call does not wait either)
bool outputs_on_device(const CallArgs& a) {
    return ss::on_device(a.hits_out) && ss::on_device(a.n_hits_out);
}

// ---- 2. query operators ----------------------------------------------------------------------------------------------------
// Required / excluded terms (ss_score_topk_constrained) resolved to one allowed set per distinct (mask, required, excluded)
// combination, which k_constraint_masks builds on the device in the call's set buffer.  The scoring kernels take the sets as the
// masked call takes registered allow-lists: q_mask / SmallHdr carry the set's index, written here into in.mask.
// The sets with range clauses (ss_score_topk_filtered), for k_field_masks; set_cl[i]: the clauses of set i.  A set with clauses and no
// terms is built by k_field_masks alone, from the registered allow-list: those sets move to the end of the set buffer —
// k_constraint_masks builds the ones in front of them — and the queries' set indices follow.  A set with terms and clauses is narrowed
// in place behind k_constraint_masks.
void plan_field_sets(BatchInputs& in, const std::vector<std::vector<ss_doc_range>>& set_cl, ConstraintPlan& cp) {
    const size_t n = cp.sets.size();
    auto field_only = [&](size_t i) { return !set_cl[i].empty() && cp.sets[i].n_req + cp.sets[i].n_exc == 0; };
    std::vector<int32_t> new_of(n);
    std::vector<size_t> old_of;
    for (int pass = 0; pass < 2; pass++)
        for (size_t i = 0; i < n; i++)
            if (field_only(i) == (pass == 1)) {
                new_of[i] = (int32_t)old_of.size();
                old_of.push_back(i);
                cp.n_field_only += pass;
            }
    std::vector<ConstraintSet> sets(n);
    for (size_t j = 0; j < n; j++) sets[j] = cp.sets[old_of[j]];
    cp.sets.swap(sets);
    for (int32_t& m : in.mask)
        if (m >= 0) m = new_of[m];
    const uint32_t group = ss::field_mask_group();
    for (size_t j = 0; j < n; j++) {
        const std::vector<ss_doc_range>& cl = set_cl[old_of[j]];
        if (cl.empty()) continue;
        if (cp.fsets.size() % group == 0) cp.fgroups.push_back(0u);
        cp.fsets.push_back(FieldSet{(uint32_t)j, j >= n - cp.n_field_only ? cp.sets[j].mask1 : FS_IN_PLACE, (uint32_t)cp.fclauses.size(), (uint32_t)cl.size()});
        for (const ss_doc_range& c : cl) {
            cp.fclauses.push_back(c);
            cp.fgroups.back() |= 1u << c.field;
        }
    }
}

int32_t resolve_constraints(BatchInputs& in, const ScorerView& v, ConstraintPlan& cp, PlanError& err) {
    if (!in.has_constraints && !in.has_ranges) return SS_OK;
    const int32_t n_q = in.n_q;
    const std::vector<uint64_t>& tp = v.tp;
    const std::vector<uint64_t>& bp = v.bp;
    const std::vector<uint32_t>&rp = in.req_ptr, &rt = in.req_terms, &ep = in.exc_ptr, &et = in.exc_terms;
    auto df = [&](uint32_t t) -> uint64_t { return (uint64_t)t < v.n_terms ? (tp[t + 1] - tp[t]) + (bp[t + 1] - bp[t]) : 0; };
    // a query's set key: {CS_EMPTY} (no doc can be allowed), {mask + 1, n_req, n_exc, required ids, excluded ids, five words per range
    // clause: field, lo, hi}, or none at all
    std::vector<std::vector<uint32_t>> keys(n_q);
    bool constrained = false;
    std::vector<uint32_t> req, exc;
    using Clause = std::tuple<int32_t, int64_t, int64_t>;
    std::vector<Clause> cl;
    for (int q = 0; q < n_q; q++) {
        // the clauses as a set (sorted, repeats dropped); one with lo > hi matches no doc
        cl.clear();
        bool no_doc = false;
        for (uint32_t c = in.has_ranges ? in.rng_ptr[q] : 0u; c < (in.has_ranges ? in.rng_ptr[q + 1] : 0u); c++) {
            cl.emplace_back(in.rng[c].field, in.rng[c].lo, in.rng[c].hi);
            no_doc = no_doc || in.rng[c].lo > in.rng[c].hi;
        }
        std::sort(cl.begin(), cl.end());
        cl.erase(std::unique(cl.begin(), cl.end()), cl.end());
        req.assign(rt.begin() + rp[q], rt.begin() + rp[q + 1]);
        exc.assign(et.begin() + ep[q], et.begin() + ep[q + 1]);
        std::sort(req.begin(), req.end());
        req.erase(std::unique(req.begin(), req.end()), req.end());
        std::sort(exc.begin(), exc.end());
        exc.erase(std::unique(exc.begin(), exc.end()), exc.end());
        if (req.size() + exc.size() > SS_MAX_CONSTRAINT_TERMS)
            return err.set(SS_ERR_UNSUPPORTED, "ss_score_topk_constrained: query %d has %zu distinct required + excluded terms (max %d)", q,
                           req.size() + exc.size(), SS_MAX_CONSTRAINT_TERMS);
        // a term without postings (unknown ids included): required, no doc contains it; excluded, it excludes nothing
        bool empty = no_doc;
        for (uint32_t t : req) empty = empty || df(t) == 0 || std::binary_search(exc.begin(), exc.end(), t);
        exc.erase(std::remove_if(exc.begin(), exc.end(), [&](uint32_t t) { return df(t) == 0; }), exc.end());
        if (empty) keys[q] = {CS_EMPTY};
        else if (!req.empty() || !exc.empty() || !cl.empty()) {
            keys[q] = {(uint32_t)((in.has_mask_arg ? in.mask[q] : -1) + 1), (uint32_t)req.size(), (uint32_t)exc.size()};
            keys[q].insert(keys[q].end(), req.begin(), req.end());
            keys[q].insert(keys[q].end(), exc.begin(), exc.end());
            for (const Clause& c : cl) {
                const uint64_t lo = (uint64_t)std::get<1>(c), hi = (uint64_t)std::get<2>(c);
                const uint32_t w[5] = {(uint32_t)std::get<0>(c), (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
                keys[q].insert(keys[q].end(), w, w + 5);
            }
        }
        constrained = constrained || !keys[q].empty();
    }
    if (!constrained) return SS_OK;
    // every query with a set: the constrained ones and, since the sets replace the registered masks for the call, the ones
    // with an allow-list alone (a set without terms: the builder copies the list)
    in.mask.resize(n_q);
    std::map<std::vector<uint32_t>, int32_t> set_of;
    std::vector<std::vector<ss_doc_range>> set_cl;          // (has_ranges) the clauses of every set
    for (int q = 0; q < n_q; q++) {
        const int32_t m = in.has_mask_arg ? in.mask[q] : -1;
        if (keys[q].empty() && m >= 0) keys[q] = {(uint32_t)(m + 1), 0u, 0u};
        if (keys[q].empty()) { in.mask[q] = -1; continue; }
        auto it = set_of.find(keys[q]);
        if (it == set_of.end()) {
            const std::vector<uint32_t>& key = keys[q];
            ConstraintSet cs{CS_EMPTY, 0u, 0u, (uint32_t)cp.terms.size()};
            std::vector<ss_doc_range> ranges;
            if (key[0] != CS_EMPTY) {
                cs.mask1 = key[0];
                cs.n_req = key[1];
                cs.n_exc = key[2];
                const auto t_end = key.begin() + 3 + cs.n_req + cs.n_exc;
                // the required terms rarest first: a block that one of them empties skips the others
                std::vector<uint32_t> order(key.begin() + 3, t_end);
                std::stable_sort(order.begin(), order.begin() + cs.n_req, [&](uint32_t a, uint32_t b) { return df(a) < df(b); });
                for (uint32_t t : order) cp.terms.push_back(ConstraintTerm{tp[t], tp[t + 1], bp[t], bp[t + 1]});
                for (auto w = t_end; w != key.end(); w += 5)
                    ranges.push_back(ss_doc_range{(int32_t)w[0], 0, (int64_t)((uint64_t)w[2] << 32 | w[1]), (int64_t)((uint64_t)w[4] << 32 | w[3])});
            }
            it = set_of.emplace(key, (int32_t)cp.sets.size()).first;
            cp.sets.push_back(cs);
            if (in.has_ranges) set_cl.push_back(std::move(ranges));
        }
        in.mask[q] = it->second;
    }
    in.any_mask = true;
    if (in.has_ranges) plan_field_sets(in, set_cl, cp);
    return SS_OK;
}

// ---- 3. the plan (the host keeps df per term; queries are tiny) ------------------------------------------------------------
// what plan_batch decides for the batch before it walks the queries
struct KernelChoice {
    uint64_t slice_target = SLICE_TARGET, wave_target = 0, small_cap = 0;
    bool wave_ok = false, batch_wave = false, small_ok = false;
    std::vector<uint8_t> suits;                 // [n_q] the query suits k_score_wave
};

// phrase parts: the driver (rarest term) of every query's phrase, the capacity of its result lists, k_phrase_match's work list
int32_t plan_phrases(const BatchInputs& in, const ScorerView& v, BatchPlan& pl, PlanError& err) {
    const int32_t n_q = in.n_q;
    const std::vector<uint64_t>& tp = v.tp;
    const std::vector<uint64_t>& bp = v.bp;
    pl.pdrv.assign(n_q, 0xFFFFFFFFu);
    pl.xoff.assign(n_q + 1, 0);
    pl.pbase.assign(n_q + 1, 0);
    for (int q = 0; q < n_q && in.has_phrase_arg; q++) {
        const uint32_t m = in.pptr[q + 1] - in.pptr[q];
        pl.xoff[q + 1] = pl.xoff[q];
        pl.pbase[q + 1] = (uint32_t)pl.parts.size();
        if (m == 0) continue;
        pl.any_phrase = true;
        if (m > 16) return err.set(SS_ERR_UNSUPPORTED, "ss_score_topk_phrase: query %d has a phrase of %u terms (max 16)", q, m);
        uint64_t best = ~0ull;
        bool known = true;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t t = in.pterms[in.pptr[q] + i];
            if ((uint64_t)t >= v.n_terms) { known = false; break; }    // a doc must contain EVERY phrase term (phrase.go:63)
            const uint64_t df = (tp[t + 1] - tp[t]) + (bp[t + 1] - bp[t]);
            if (df < best) { best = df; pl.pdrv[q] = i; }
        }
        pl.pbase[q + 1] = (uint32_t)pl.parts.size();
        if (!known) { pl.pdrv[q] = 0xFFFFFFFFu; continue; }
        if ((uint64_t)pl.xoff[q] + best >= (1ull << 32))
            return err.set(SS_ERR_UNSUPPORTED, "ss_score_topk_phrase: the phrases of this batch have more than 2^32 candidate documents (split the batch)");
        pl.xoff[q + 1] = pl.xoff[q] + (uint32_t)best;   // matches <= docs of the rarest term
        // candidates = the rarest term's body postings (pass 0), then its title postings (pass 1), PH_PART per workgroup
        const uint32_t dt = in.pterms[in.pptr[q] + pl.pdrv[q]];
        const uint64_t nbody = bp[dt + 1] - bp[dt], ntitle = tp[dt + 1] - tp[dt];
        for (int pass = 0; pass < 2; pass++) {
            const uint64_t nc = pass == 0 ? nbody : ntitle;
            for (uint64_t c = 0; c < nc; c += PH_PART)
                pl.parts.push_back(make_uint4((uint32_t)q, (uint32_t)pass, (uint32_t)c, (uint32_t)std::min<uint64_t>(PH_PART, nc - c)));
        }
        pl.pbase[q + 1] = (uint32_t)pl.parts.size();
    }
    return SS_OK;
}

// slice sizes of the two scoring kernels for a batch of tok_tot postings
void slice_targets(const BatchInputs& in, const ScorerView& v, const ScoreOptions& opt, const BatchPlan& pl, uint64_t tok_tot, KernelChoice& kc) {
    // Slice size: SLICE_TARGET postings when the batch fills the chip several times over; smaller (down to
    // SLICE_MIN) for small batches, so that one query's lists are spread over many CUs instead of being
    // walked by a single workgroup (latency of a lone query: 0.72 ms -> see DESIGN.md K4).
    {
        const uint64_t slots = (uint64_t)std::max(v.cu_count, 1) * SS_WGS_PER_CU;
        // measured (10M docs, 3-term head queries, batches of 1..4096): one partial wave of slices is best — about
        // 1.5x the batch's postings per resident workgroup slot, never below SLICE_MIN (a slice costs ~45 us of
        // threshold warm-up whatever its size) nor above SLICE_TARGET
        uint64_t slice_target = std::min<uint64_t>(SLICE_TARGET, std::max<uint64_t>(SLICE_MIN, tok_tot * 3 / (2 * slots)));
        // (results in device memory: consecutive batches overlap — "score.pipeline_slices" —, the next batch's kernel fills this one's
        //  tail and larger slices pay: mixed batch 0.164 ms at 2.6x this target against 0.170)
        if (in.dev_out && opt.pipeline != 0 && opt.pipeline_slices) slice_target = std::min<uint64_t>(SLICE_TARGET, slice_target * 5 / 2);
        if (opt.slice_target != OPT_UNSET) slice_target = (uint64_t)opt.slice_target;
        kc.slice_target = (uint64_t)std::max<int64_t>(1024, (int64_t)slice_target);
    }
    // k_score_wave (one wave per slice) takes the plain OR queries: few lists, no phrase part, small k, inputs for which the
    // filter's assumptions hold, and a list long enough for the threshold floor (k'-th largest impact, k' >= k) to exist;
    // everything else runs k_score_slices.  Option "score.wave" = 0 switches the wave kernel off (tests, A/B).
    kc.wave_ok = opt.wave && v.has_combined && !pl.exact_all && in.k <= ss::score_wave_max_k();
    if (kc.wave_ok) {
        // about 5.5 slices per nine-wave-per-CU slot (four rounds of the 12 waves a CU holds), 8k .. 48k postings each
        const uint64_t slots = (uint64_t)std::max(v.cu_count, 1) * 9;
        uint64_t wave_target = std::min<uint64_t>(49152, std::max<uint64_t>(8192, tok_tot * 2 / (11 * slots)));          // (config 3, ms per batch at 6k / 8k / 10k / 12k / 14k / 17k / 21k postings: 0.661 / 0.635 / 0.616 / 0.623 / 0.655 / 0.649 / 0.639)
        if (opt.wave_slice_target != OPT_UNSET) wave_target = (uint64_t)opt.wave_slice_target;
        kc.wave_target = (uint64_t)std::max<int64_t>(1024, (int64_t)wave_target);
    }
}

// Which queries suit k_score_wave: no phrase part, few lists, a list long enough for the threshold floor (k'-th largest
// impact, k' = k rounded up to 2^j) to exist — and EVERY list long enough for that floor to be selective: the k'-th largest of
// n impacts lets k'/n of a list's records through until the real threshold has risen (measured: batches of term ranks
// U[1,100k] — long and short lists mixed — ran 3.5x slower here than in k_score_slices, with 100x the overflow events per
// slice).  Option "score.wave_min_list" x k' postings (default 16; 0 = no such demand: tests reach the kernel with small tables).
// The kernel is taken per BATCH: two scoring kernels one after the other each pay their ramp-up and tail (a batch split
// between them measured slower than either alone), so it runs only when the queries it suits carry 90 % of the batch.
// ... and few lists: a window is cut so that its blocks number 16 - 3 - (lists), every list adding a boundary block; with
// 12 dense lists a window is one driver block and most windows overflow into the slow path (soak on the config-3 index,
// wave / slices time: 0.4-0.9 at <= 5 terms, 1.0-1.1 at 9, 2-3 at 12).  Option "score.wave_max_terms", default 6.
void choose_wave_queries(const BatchInputs& in, const ScorerView& v, const ScoreOptions& opt, const BatchPlan& pl,
                         const std::vector<uint32_t>& tok_lt, const std::vector<uint32_t>& tok_lb, KernelChoice& kc) {
    const int32_t n_q = in.n_q, k = in.k;
    const uint32_t wave_max_terms = (uint32_t)std::min<int64_t>(ss::score_wave_max_lists(), std::max<int64_t>(1, opt.wave_max_terms));
    const int64_t wml = std::max<int64_t>(0, opt.wave_min_list);
    const uint64_t wave_min_list = (uint64_t)wml << pl.kth_j;
    kc.suits.assign(n_q, 0);
    if (!kc.wave_ok) return;
    uint64_t fit = 0, all = 0;
    for (int q = 0; q < n_q; q++) {
        uint64_t tot = 0, shortest = ~0ull, longest = 0;
        uint32_t n_known = 0;
        for (uint32_t i = in.qptr[q]; i < in.qptr[q + 1]; i++) {
            const uint32_t t = in.terms[i];
            if ((uint64_t)t >= v.n_terms) continue;
            n_known++;
            tot += (uint64_t)tok_lt[i] + tok_lb[i];
            const uint64_t len = std::max(tok_lt[i], tok_lb[i]);
            shortest = std::min(shortest, len);
            longest = std::max(longest, len);
        }
        all += tot;
        const bool phrase_q = in.has_phrase_arg && in.pptr[q + 1] > in.pptr[q];
        // (n_known counts duplicate tokens too: an upper bound of the distinct terms, good enough for the choice)
        if (n_known && n_known <= wave_max_terms && !phrase_q && longest >= (uint64_t)4 * (uint64_t)k && longest >= 1024 &&
            shortest >= wave_min_list) {
            kc.suits[q] = 1;
            fit += tot;
        }
    }
    // (a lone query or two — under ~400k postings — finish sooner in k_score_slices: 0.143 against 0.166 ms for two head queries,
    //  host in / host out; from four queries on the wave kernel leads, 0.21 against 0.31 ms)
    // "score.wave_share_pct": the share of the batch's postings the suited queries must carry (default 90; with device outputs
    // the two kernels of a split batch run side by side on two streams, so a split no longer pays two ramp-ups and tails one
    // after the other)
    const uint64_t share = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(100, opt.wave_share_pct));
    kc.batch_wave = wml == 0 ? fit > 0 : (fit * 100 >= all * share && fit >= 400000);
    // a query with an allow-list has no threshold floor, which the wave kernel's routing rests on: k_score_slices.  (After the
    // batch's choice: the unmasked queries of the batch go where they would without the masked ones.)
    for (int q = 0; q < n_q && in.any_mask; q++)
        if (in.mask[q] >= 0) kc.suits[q] = 0;
}

// k_score_small (one workgroup per query, every posting scored exactly, no slices and no merge: score_small.hip) takes queries without
// a phrase part whose lists hold at most score_small_cap() postings in all.  Bit-identical hits.  Round 5 measured both ways: a
// workgroup is a chain of short phases (list table, postings -> hash table, magnitudes -> scores, radix selection, placement, hits:
// ~20 us with nothing to overlap), so a 1024-query tail batch is SLOWER there than in the slices pipeline that runs batches side by
// side (0.14 against 0.09 ms), while a short call — where latency is all there is — is faster (1 .. 32 tail queries host to host
// 0.068-0.074 -> 0.050-0.058 ms): DESIGN K4c.
// "score.small": 1 = every query that fits (tests, A/B); 2 (default) = only a call that consists of such queries and is at most
// "score.small_max_batch" queries long: ONE launch that writes the hits, against a slices kernel and a merge — what a lone query or
// a handful gain in latency a 1024-query batch loses in overlap (the slices pipeline runs batches side by side); 0 = never.
void choose_small_kernel(const BatchInputs& in, const ScoreOptions& opt, const std::vector<uint32_t>& tok_lt, const std::vector<uint32_t>& tok_lb,
                         BatchPlan& pl, KernelChoice& kc) {
    const int32_t n_q = in.n_q, k = in.k;
    kc.small_cap = (uint64_t)std::min<int64_t>(ss::score_small_cap(), std::max<int64_t>(0, opt.small_cap));
    kc.small_ok = opt.small == 1 && k <= ss::score_small_max_k();
    // "score.small_batch" = 1 (with "score.small" = 2): in a LONGER call with device outputs every query that fits goes there too, the
    // kernel on an internal stream beside the neighbouring batches like the slices kernel, its rows staged and copied on the caller's stream
    pl.small_batch = opt.small == 2 && in.dev_out && k <= ss::score_small_max_k() && opt.pipeline != 0 && opt.small_batch != 0 &&
                     n_q > opt.small_max_batch;
    if (pl.small_batch) kc.small_ok = true;
    if (opt.small == 2 && k <= ss::score_small_max_k() && n_q <= opt.small_max_batch && !in.has_phrase_arg) {
        kc.small_ok = true;                                 // (tokens counted with their repeats: an upper bound of a query's postings)
        for (int q = 0; q < n_q && kc.small_ok; q++) {
            uint64_t tq = 0;
            for (uint32_t i = in.qptr[q]; i < in.qptr[q + 1]; i++) tq += (uint64_t)tok_lt[i] + tok_lb[i];
            kc.small_ok = tq <= kc.small_cap && in.qptr[q + 1] - in.qptr[q] <= (uint32_t)(ss::score_small_max_lists() / 2);
        }
    }
}

// per query: its distinct terms, constants, and either its entry of k_score_small's table or its slices; cost[q] = postings per slice
int32_t plan_queries(const BatchInputs& in, const ScorerView& v, const ScoreOptions& opt, const KernelChoice& kc,
                     const std::vector<uint32_t>& tok_lt, const std::vector<uint32_t>& tok_lb, uint64_t tok_tot, BatchPlan& pl,
                     std::vector<uint64_t>& cost, PlanError& err) {
    const int32_t n_q = in.n_q;
    const std::vector<uint64_t>& tp = v.tp;
    const std::vector<uint64_t>& bp = v.bp;
    const uint64_t grade_tot = tok_tot;
    uint64_t grade_seen = 0;
    pl.qoff.assign(n_q + 1, 0);
    pl.sbase.assign(n_q + 1, 0);
    pl.qmag.resize(n_q);
    pl.ub.assign(n_q, 0.0);
    pl.slices.reserve((size_t)n_q * 16);
    pl.dterm.reserve(in.n_tok);
    pl.dmult.reserve(in.n_tok);
    for (int q = 0; q < n_q; q++) {
        const size_t d0 = pl.dterm.size();
        uint64_t tot = 0;
        for (uint32_t i = in.qptr[q]; i < in.qptr[q + 1]; i++) {
            const uint32_t t = in.terms[i];
            if ((uint64_t)t >= v.n_terms) continue;             // unknown word: ErrKeyNotFound -> no postings (main_retrieve.go:193,218)
            size_t j = d0;
            while (j < pl.dterm.size() && pl.dterm[j] != t) j++;
            if (j < pl.dterm.size()) { pl.dmult[j]++; continue; } // duplicate token: counted again (Q8)
            pl.dterm.push_back(t);
            pl.dmult.push_back(1);
            tot += (uint64_t)tok_lt[i] + tok_lb[i];
        }
        if (pl.dterm.size() - d0 > SS_MAX_QUERY_TERMS)
            return err.set(SS_ERR_UNSUPPORTED, "ss_score_topk: query %d has more than %d distinct terms", q, SS_MAX_QUERY_TERMS);
        pl.qoff[q + 1] = (uint32_t)pl.dterm.size();
        pl.qmag[q] = std::sqrt((double)in.qlen[q]);             // get_metadata.go:53
        if (in.has_probs) {
            // upper bound of sqd over all docs, same operation order as topic_dot (monotone)
            double ub = 0.0;
            for (int t = 0; t < in.K; t++) {
                const double pt = in.probs[(size_t)q * in.K + t];
                ub += pt * (pt >= 0.0 ? v.prior_max[t] : v.prior_min[t]);
            }
            pl.ub[q] = ub != ub ? INFINITY : ub;
        }
        // the window plan holds (n_win + 1) * L cursors: keep a slice within what the plan can cut into regular windows
        const uint64_t n_lists = 2 * (pl.dterm.size() - d0) + 4;
        const uint64_t plan_cap = std::max<uint64_t>(TARGET, (uint64_t)(TBL_CAP / n_lists > 2 ? TBL_CAP / n_lists - 2 : 1) * TARGET * 7 / 8);
        uint64_t q_target = kc.slice_target;
        uint64_t max_slices = MAX_SLICES_PER_Q;
        if (kc.small_ok && tot <= kc.small_cap && !(in.has_phrase_arg && in.pptr[q + 1] > in.pptr[q])) {
            // no slices: k_score_small reads the lists whole and writes the hits.  Its list table is made here — the host holds
            // term_ptr, and the kernel's own walk (query -> terms -> term_ptr) was three dependent loads at the head of every workgroup
            SmallList tmp[SS_SMALL_MAX_LISTS];
            uint32_t nl = 0, run = 0;
            bool fits = true;
            for (size_t j = d0; j < pl.dterm.size() && fits; j++) {
                const uint32_t t = pl.dterm[j];
                for (uint32_t field = 0; field < 2; field++) {
                    const uint64_t* pp = field ? tp.data() : bp.data();
                    const uint64_t b = pp[t], e = pp[t + 1];
                    if (e == b) continue;
                    if (nl == SS_SMALL_MAX_LISTS) { fits = false; break; }
                    run += (uint32_t)(e - b);
                    tmp[nl++] = SmallList{b, run, pl.dmult[j] << 1 | field};
                }
            }
            if (fits) {
                SmallEnt en;
                en.h = SmallHdr{(uint32_t)q, nl, run, in.any_mask ? (uint32_t)(in.mask[q] + 1) : 0u, pl.qmag[q], 0.0};
                en.loff = (uint32_t)pl.small_lists.size();
                pl.small_lists.insert(pl.small_lists.end(), tmp, tmp + nl);
                pl.small_lmax = std::max(pl.small_lmax, nl);
                (run <= ss::score_small_cap_a() ? pl.small_a : pl.small_b).push_back(en);
                pl.fast[q] = 2;
                pl.sbase[q + 1] = (uint32_t)pl.slices.size();
                continue;
            }
        }
        const bool fast = kc.batch_wave && kc.suits[q] && pl.dterm.size() > d0 && (pl.dterm.size() - d0) <= (size_t)ss::score_wave_max_lists();
        if (fast) {
            pl.fast[q] = 1;
            q_target = kc.wave_target;
            max_slices = 4096;
        }
        // graded slices: the first part of the batch's postings in larger slices, the rest in smaller ones — launched
        // longest first, the small ones fill the kernel's tail (both kernels; see DESIGN K4b)
        if (opt.wave_big_pct > 0 && (fast || opt.grade_slices)) {
            q_target = grade_seen * 100 < grade_tot * (uint64_t)opt.wave_big_pct ? q_target * (uint64_t)opt.wave_big_x100 / 100
                                                                                 : q_target * (uint64_t)opt.wave_small_x100 / 100;
            q_target = std::max<uint64_t>(q_target, 1024);
            grade_seen += tot;
        }
        if (!fast) q_target = std::min<uint64_t>(q_target, plan_cap);
        uint64_t ns = std::max<uint64_t>(1, (tot + q_target - 1) / q_target);
        ns = std::min<uint64_t>(ns, std::min<uint64_t>(max_slices, v.n_docs));
        cost[q] = tot / ns;
        for (uint64_t j = 0; j < ns; j++) {
            SliceDesc sd;
            sd.q = (uint32_t)q;
            sd.dlo = (uint32_t)(v.n_docs * j / ns);
            sd.dhi = j + 1 == ns ? 0xFFFFFFFFu : (uint32_t)(v.n_docs * (j + 1) / ns);
            sd.pad = 0;
            pl.slices.push_back(sd);
        }
        pl.sbase[q + 1] = (uint32_t)pl.slices.size();
    }
    return SS_OK;
}

// launch order: the wave kernel's slices first, then k_score_slices' (each group longest first); merge list = the wave queries
// (the slices of a query are consecutive and cost the same, so the order is that of the QUERIES, stably sorted, with every
//  query's slices in a row: sorting 14.6k slice indices took two thirds of the 0.22 ms a config-3 batch is planned in)
void plan_launch_order(int32_t n_q, const std::vector<uint64_t>& cost, BatchPlan& pl) {
    pl.order.resize(pl.n_slices);
    // (a counting sort by a coarse cost class — the leading bit of the cost and the four bits behind it, 6 % steps — instead of
    //  std::stable_sort by the exact cost: the order only decides which slices are LAUNCHED first, and the comparison sort with its
    //  temporary buffer was most of the 35 us the plan of a 1024-query batch took (round 5); stable inside a class)
    std::vector<uint32_t> q_order(n_q);
    {
        constexpr int NCLS = 2048;
        auto cls_of = [&](uint32_t q) -> int {
            const uint64_t c = cost[q];
            int kc = 0;
            if (c) {
                const int msb = 63 - __builtin_clzll(c);
                const uint64_t frac = msb >= 4 ? (c >> (msb - 4)) & 15u : (c << (4 - msb)) & 15u;
                kc = (msb << 4 | (int)frac) + 1;                    // <= 64 * 16
            }
            return ((pl.fast[q] & 1) ? 1024 : 0) + std::min(kc, 1023);
        };
        uint32_t cnt[NCLS + 1] = {};
        for (int q = 0; q < n_q; q++) cnt[NCLS - 1 - cls_of((uint32_t)q)]++;      // descending classes
        uint32_t run = 0;
        for (int c = 0; c < NCLS; c++) { const uint32_t v = cnt[c]; cnt[c] = run; run += v; }
        for (int q = 0; q < n_q; q++) q_order[cnt[NCLS - 1 - cls_of((uint32_t)q)]++] = (uint32_t)q;
    }
    size_t o = 0;
    for (int i = 0; i < n_q; i++)
        for (uint32_t sl = pl.sbase[q_order[i]]; sl < pl.sbase[q_order[i] + 1]; sl++) pl.order[o++] = sl;
    for (size_t i = 0; i < pl.n_slices; i++) pl.n_fast_slices += pl.fast[pl.slices[i].q] & 1;
    for (int q = 0; q < n_q; q++)
        if (pl.fast[q] & 1) pl.mergeq.push_back((uint32_t)q);
}

// The filter of k_score_slices assumes non-negative finite addends (see there).  Anything else — tables or priors
// flagged at creation, a negative / non-finite topic probability, queryLength <= 0 — switches it off for this call:
// every record then goes through the exact stage, which restates the reference's arithmetic for any input.
// (The first part of the plan, apart from plan_batch: "score.trace" counts it with the checks of the inputs.)
void check_filter_assumptions(const BatchInputs& in, const ScorerView& v, BatchPlan& pl) {
    pl.exact_all = !v.clean || (in.has_probs && !v.prior_clean);
    for (int q = 0; q < in.n_q && !pl.exact_all; q++) pl.exact_all = in.qlen[q] <= 0;
    for (size_t i = 0; i < in.probs.size() && !pl.exact_all; i++) pl.exact_all = !(in.probs[i] >= 0.0) || !std::isfinite(in.probs[i]);
    while ((1 << pl.kth_j) < in.k) pl.kth_j++;
}

// needs check_filter_assumptions' exact_all and kth_j in `pl`
int32_t plan_batch(const BatchInputs& in, const ScorerView& v, const ScoreOptions& opt, BatchPlan& pl, PlanError& err) {
    const int32_t n_q = in.n_q, k = in.k;
    SS_TRY(plan_phrases(in, v, pl, err));
    // The tokens' list lengths, looked up ONCE: the two host copies of term_ptr are 8 MB each at config 3 and a batch's terms are
    // scattered over them, so every look-up is a cache miss — and the plan used to make them in three passes (batch total, the
    // wave kernel's suitability test, the per-query slicing): 37k misses per 1024-query batch, most of the 43 us the plan took for a
    // batch of tail queries (round 5: `score.trace`, tools/host_tail.py).  0 / 0 for unknown terms.
    static thread_local std::vector<uint32_t> tok_lt, tok_lb;
    tok_lt.resize(in.n_tok);
    tok_lb.resize(in.n_tok);
    uint64_t tok_tot = 0;
    for (uint32_t i = 0; i < in.n_tok; i++) {
        const uint32_t t = in.terms[i];
        const bool known = (uint64_t)t < v.n_terms;
        tok_lt[i] = known ? (uint32_t)(v.tp[t + 1] - v.tp[t]) : 0u;       // (a posting list is shorter than 2^32: ss_index_create)
        tok_lb[i] = known ? (uint32_t)(v.bp[t + 1] - v.bp[t]) : 0u;
        tok_tot += (uint64_t)tok_lt[i] + tok_lb[i];
    }
    KernelChoice kc;
    slice_targets(in, v, opt, pl, tok_tot, kc);
    choose_wave_queries(in, v, opt, pl, tok_lt, tok_lb, kc);
    pl.fast.assign(n_q, 0);
    choose_small_kernel(in, opt, tok_lt, tok_lb, pl, kc);
    std::vector<uint64_t> cost(n_q, 0);             // postings per slice of the query (all its slices cost the same)
    SS_TRY(plan_queries(in, v, opt, kc, tok_lt, tok_lb, tok_tot, pl, cost, err));
    if (opt.small == 2 && !(pl.small_batch && opt.small_batch == 2) && !pl.small_a.empty() && !pl.small_b.empty()) {      // one launch: the larger table takes them all
        pl.small_b.insert(pl.small_b.end(), pl.small_a.begin(), pl.small_a.end());
        pl.small_a.clear();
    }
    pl.n_small_a = pl.small_a.size();
    pl.n_small_b = pl.small_b.size();
    pl.n_small = pl.n_small_a + pl.n_small_b;
    pl.small_stride = sizeof(SmallHdr) + (size_t)pl.small_lmax * sizeof(SmallList);
    pl.n_slices = pl.slices.size();
    pl.n_d = pl.dterm.size();
    plan_launch_order(n_q, cost, pl);
    pl.cb = SS_CB_MIN;
    while (pl.cb < 2 * k) pl.cb <<= 1;
    // k_merge_flat gathers ALL of a query's candidates before it sorts once (config 3: ~300 per query at k = 100; with room for
    // 2k only it sorted 2.6 times per query, and the sorts' barriers were half of the merge)
    pl.cb_flat = std::max(pl.cb, 512);
    return SS_OK;
}

// ---- 4. which kernels share which streams (the streams themselves: bind_streams) -------------------------------------------
Route choose_route(const BatchPlan& pl, bool dev_out, const ScoreOptions& opt) {
    Route r{};
    const bool wave_part = pl.n_fast_slices > 0 && !pl.mergeq.empty();
    // "score.pipeline" (default): a batch that is all k_score_wave, results in device memory.  Its k_wave_prep and k_score_wave go
    // to the context's WAVE stream, its k_merge_flat to the caller's stream behind an event: the next batch's k_score_wave (which
    // needs nothing the caller's stream produces — queries arrive in host memory, the index is immutable while a scorer holds it,
    // candidate lists and counters exist once per turn) starts under this batch's merge, and since the merge — the kernel that
    // writes the hits — sits on the caller's stream, the results are complete in stream order like before.  [Round 3 had it the
    // other way round (merge on a side stream that the caller's stream did not wait for): faster by the same amount, but the hits
    // were only complete after ss_synchronize.]
    // A batch split between the two scoring kernels (queries that do not suit k_score_wave: short lists, phrases, many terms) is
    // pipelined too: its k_score_slices part — which writes its queries' hits itself — runs on the caller's stream BESIDE the wave
    // kernel, the wave queries' merge follows behind both.
    r.pipe = dev_out && wave_part && opt.pipeline != 0;
    // A batch that is all k_score_slices, results in device memory ("score.pipeline" != 0 and "score.pipeline_slices", default on):
    // pipelined like the wave batches — the slices kernel on an internal stream, the merge (k_merge_topk, the kernel that writes
    // the hits) as a launch of its own on the caller's stream behind an event.  Small slices leave the last third of their kernel
    // on a thinning machine; the next batch's kernel now starts under it.  (The fused merge — the last slice of a query merges it
    // inside k_score_slices — cannot move off the caller's stream: it writes the hits, and a consumer the caller enqueued between
    // two calls must see the first call's hits before the second call's kernel touches the buffer.)
    r.pipe_s = dev_out && pl.n_fast_slices == 0 && pl.n_slices > 0 && opt.pipeline != 0 &&
               opt.pipeline_slices;       // (phrase queries included: their match kernels go in front of the slices kernel)
    // ... and the k_score_slices part of a SPLIT batch (some queries on the wave kernel, the rest here): on a second internal stream
    // beside the wave kernel, unfused, its k_merge_topk on the caller's stream in front of the wave queries' k_merge_flat
    r.pipe_split = dev_out && wave_part && pl.n_slices > pl.n_fast_slices && opt.pipeline >= 2 && opt.pipeline_slices;
    r.fused = !opt.separate_merge && !r.pipe_s && !r.pipe_split;
    // k_score_small of a pipelined batch: on the slices kernel's stream if there is one, else on a side stream beside the wave kernel,
    // else (every query small) on a wave stream of its own
    r.small_staged = pl.small_batch && pl.n_small > 0;
    r.small_side = r.small_staged && !r.pipe_split && dev_out && wave_part && opt.pipeline >= 2;
    r.small_alone = r.small_staged && !r.pipe_s && !r.pipe_split && !r.small_side;
    return r;
}

// ---- 5. staging --------------------------------------------------------------------------------------------------------------
// Walks the plan's sections in buffer order.  Without buffers it only measures (`o` ends as the plan's size); with them it copies
// each section to the pinned buffer and points the kernel parameter at its place in the device copy.
struct PlanWriter {
    unsigned char* hp = nullptr;
    const unsigned char* dp = nullptr;
    size_t o = 0;
    // `count` elements from `src`; the parameter stays null where the kernels must not see the section
    template <typename T>
    void add(const T*& field, const T* src, size_t count, bool visible = true) {
        const size_t bytes = count * sizeof(T);
        if (hp) {
            if (bytes) std::memcpy(hp + o, src, bytes);
            field = visible ? reinterpret_cast<const T*>(dp + o) : nullptr;
        }
        o = align16(o + bytes);
    }
    // a section its owner writes record by record: where to write (null while measuring)
    unsigned char* reserve(const unsigned char*& field, size_t bytes) {
        unsigned char* const w = hp ? hp + o : nullptr;
        if (hp) field = dp + o;
        o = align16(o + bytes);
        return w;
    }
};

// the tables of the allowed sets' builders (the last sections of a scoring call's plan; all there is of ss::allowed_sets_into_turn's)
void constraint_sections(PlanWriter& w, const ConstraintPlan& cons, ConstraintParams& cp, FieldParams& fp) {
    w.add(cp.sets, cons.sets.data(), cons.sets.size());
    w.add(cp.terms, cons.terms.data(), cons.terms.size());
    w.add(fp.sets, cons.fsets.data(), cons.fsets.size());
    w.add(fp.clauses, cons.fclauses.data(), cons.fclauses.size());
    w.add(fp.group_fields, cons.fgroups.data(), cons.fgroups.size());
}

// THE list of the plan's sections: order, source, size, and whether the kernels see it.  Returns where k_score_small's table goes.
unsigned char* plan_sections(PlanWriter& w, const BatchInputs& in, const ConstraintPlan& cons, const BatchPlan& pl, ScoreParams& p,
                             ConstraintParams& cp, FieldParams& fp) {
    const size_t n_q = (size_t)in.n_q;
    const bool ph = pl.any_phrase;
    w.add(p.q_off, pl.qoff.data(), n_q + 1);
    w.add(p.dterm, pl.dterm.data(), pl.n_d);
    w.add(p.dmult, pl.dmult.data(), pl.n_d);
    w.add(p.slice_base, pl.sbase.data(), n_q + 1);
    w.add(p.order, pl.order.data(), pl.n_slices);
    w.add(p.qmag, pl.qmag.data(), n_q);
    w.add(p.sqd_ub, pl.ub.data(), n_q);
    w.add(p.slices, pl.slices.data(), pl.n_slices);
    w.add(p.ph_off, in.pptr.data(), n_q + 1, ph);
    w.add(p.ph_terms, in.pterms.data(), in.pterms.size(), ph);
    w.add(p.ph_drv, pl.pdrv.data(), n_q, ph);
    w.add(p.x_off, pl.xoff.data(), n_q + 1, ph);
    w.add(p.ph_pbase, pl.pbase.data(), n_q + 1, ph);
    w.add(p.ph_parts, pl.parts.data(), pl.parts.size(), ph);
    w.add(p.probs, in.probs.data(), in.probs.size(), in.has_probs);
    w.add(p.merge_q, pl.mergeq.data(), pl.mergeq.size());
    w.add(p.q_fast, pl.fast.data(), n_q);
    unsigned char* const small_tab = w.reserve(p.small_tab, pl.n_small * pl.small_stride);
    w.add(p.q_mask, in.mask.data(), in.any_mask ? n_q : 0, in.any_mask);
    constraint_sections(w, cons, cp, fp);
    return small_tab;
}

// Takes the next turn of per-batch buffers and waits until the batch that last used it is done with them; the pinned buffer,
// the device copy and the allowed sets are grown to this batch's size.
int32_t acquire_turn(ss_scorer* s, size_t plan_bytes, size_t n_csets, TurnRows* turn_rows, StagedBatch& sb) {
    ss_ctx* ctx = s->ctx;
    const int pb = sb.turn = s->plan_turn;
    s->plan_turn = (s->plan_turn + 1) % ss_scorer::TURNS;
    Turn& t = s->turn[pb];
    SS_HIP(ctx, t.h_plan.ensure(plan_bytes));
    // the batch two calls ago used this turn's device buffers (plan, prep, candidates) and may still be running — in pipelined mode its
    // merge certainly may: the host runs at most two batches ahead, and waits here BEFORE any of those buffers is grown or rewritten
    SS_HIP(ctx, t.batch_ev.wait());
    SS_HIP(ctx, ensure(t.d_plan, plan_bytes));
    if (turn_rows) {                             // ss_similar_topk's k + 1 rows: this turn's block, free since the wait above like the sets below
        SS_HIP(ctx, ensure(t.d_hits, turn_rows->rows));
        SS_HIP(ctx, ensure(t.d_n, turn_rows->n_q));
        turn_rows->hits = t.d_hits.p;
        turn_rows->n_hits = t.d_n.p;
        turn_rows->turn = pb;
    }
    // the call's allowed sets: this turn's buffer, free since the wait above (the batch that last read it is done); exactly the size
    // needed (1.25 MB per set at 10M docs), not grown by half like the other workspaces
    sb.set_stride = std::max<uint64_t>(4, ((s->n_docs + 31) / 32 + 3) & ~(uint64_t)3);
    if (n_csets && t.d_sets.n < n_csets * sb.set_stride) {
        const hipError_t e = t.d_sets.alloc(n_csets * sb.set_stride);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            t.d_sets.release();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "ss_score_topk_constrained: no device memory for %zu allowed sets of %llu bytes",
                             n_csets, (unsigned long long)(sb.set_stride * sizeof(uint32_t)));
        }
    }
    return SS_OK;
}

// the turn's device workspaces, grown to this batch's size (grow-only: no hipMalloc / hipFree on the steady-state query path)
int32_t grow_workspaces(ss_scorer* s, const BatchInputs& in, const BatchPlan& pl, const Route& r, StagedBatch& sb) {
    ss_ctx* ctx = s->ctx;
    Turn& t = s->turn[sb.turn];
    const size_t n_q = (size_t)in.n_q, k = (size_t)in.k;
    hipStream_t st = ctx->stream;
    if (pl.any_phrase) {
        for (int x = 0; x < 4; x++) {
            SS_HIP(ctx, ensure(t.d_x[x], (size_t)pl.xoff[n_q]));
            SS_HIP(ctx, ensure(t.d_xw[x], (size_t)pl.xoff[n_q]));
        }
        SS_HIP(ctx, ensure(t.d_xcnt, n_q * 4));
        SS_HIP(ctx, ensure(t.d_pcnt, std::max<size_t>(pl.parts.size(), 1) * 2));
    }
    SS_HIP(ctx, ensure(t.d_so_key, pl.n_slices * k));
    SS_HIP(ctx, ensure(t.d_so_doc, pl.n_slices * k));
    SS_HIP(ctx, ensure(t.d_so_cnt, pl.n_slices));
    if (r.small_staged) {
        SS_HIP(ctx, ensure(t.d_small_stage, pl.n_small * k));
        SS_HIP(ctx, ensure(t.d_small_stage_n, pl.n_small));
    }
    if (r.fused && s->qticket_zeroed < n_q) {
        SS_HIP(ctx, ensure(s->d_qticket, n_q));
        SS_HIP(ctx, hipMemsetAsync(s->d_qticket.p, 0, n_q * sizeof(uint32_t), st));
        s->qticket_zeroed = n_q;
    }
    if (!pl.mergeq.empty() && t.qcnt_zeroed < n_q) {    // k_merge_flat hands every counter back at zero
        SS_HIP(ctx, ensure(t.d_qcnt, n_q));
        SS_HIP(ctx, hipMemsetAsync(t.d_qcnt.p, 0, t.d_qcnt.bytes(), st));
        SS_HIP(ctx, hipStreamSynchronize(st));                        // (first use or growth only) k_score_wave may run on another stream
        t.qcnt_zeroed = t.d_qcnt.n;
    }
    // Small results that go back to the host (a lone query, a handful): hits and counts in ONE device block, one copy into the context's
    // pinned scratch, two host memcpys — a second device-to-host copy costs a lone query ~8 us of its ~0.12 ms (round 5)
    sb.res_rows = n_q * k;
    sb.res_bytes = sb.res_rows * sizeof(ss_hit) + n_q * sizeof(int32_t);
    // (up to 128 KB — 32 queries at k = 100 —: beyond that the extra host copy costs more than the second transfer; a 4 MB batch through
    //  a pinned block measured 0.79 against 0.655 ms in round 4)
    sb.one_copy = !in.dev_out && sb.res_bytes <= ss_scorer::H_RES_BYTES;
    if (sb.one_copy && !s->h_res.p && s->h_res.alloc(ss_scorer::H_RES_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        sb.one_copy = false;
    }
    SS_HIP(ctx, ensure(s->d_hits, sb.res_rows + (sb.one_copy ? (n_q * sizeof(int32_t) + sizeof(ss_hit) - 1) / sizeof(ss_hit) : 0)));
    SS_HIP(ctx, ensure(s->d_nhits, n_q));
    if (pl.n_fast_slices) SS_HIP(ctx, ensure(t.d_wprep, ss::score_wave_prep_bytes((unsigned)pl.n_fast_slices)));
    return SS_OK;
}

// the parameters of the allowed sets' builders that are not sections of the plan: the tables' docs, the registered masks, this turn's sets
void fill_constraint_params(ss_scorer* s, const ConstraintPlan& cons, StagedBatch& sb) {
    const Turn& t = s->turn[sb.turn];
    const size_t n_csets = cons.sets.size();
    if (n_csets) {
        ConstraintParams& cp = sb.cp;
        cp.t_doc = s->title->post_doc.p; cp.b_doc = s->body->post_doc.p;
        cp.reg_masks = s->masks.p; cp.reg_words = s->mask_words;
        cp.out = t.d_sets.p;
        cp.stride = sb.set_stride;
        cp.n_words = (s->n_docs + 31) / 32;
        cp.n_blocks = ss::constraint_blocks(sb.set_stride);
    }
    if (!cons.fsets.empty()) {
        FieldParams& fp = sb.fp;
        fp.values = s->fields.p;
        fp.n_docs = s->n_docs;
        fp.n_sets = (uint32_t)cons.fsets.size();
        fp.reg_masks = s->masks.p; fp.reg_words = s->mask_words;
        fp.out = t.d_sets.p;
        fp.stride = sb.set_stride;
        fp.n_words = (s->n_docs + 31) / 32;
    }
}

// everything of the kernel parameters that is not a section of the plan: the index, this turn's workspaces, the outputs
void fill_params(ss_scorer* s, const CallArgs& a, const BatchInputs& in, const ConstraintPlan& cons, const BatchPlan& pl, const Route& r,
                 StagedBatch& sb) {
    const Turn& t = s->turn[sb.turn];
    const size_t n_csets = cons.sets.size();
    ScoreParams& p = sb.p;
    p.t_ptr = s->title->term_ptr.p; p.t_rec = s->t_rec.p; p.t_w = s->title->post_w.p; p.t_mag = s->title->mag.p; p.t_kth = s->t_kth.p;
    p.b_ptr = s->body->term_ptr.p; p.b_rec = s->b_rec.p; p.b_w = s->body->post_w.p; p.b_mag = s->body->mag.p; p.b_kth = s->b_kth.p;
    p.c_ptr = s->c_ptr.p; p.c_rec = s->c_rec.p; p.c_w = s->c_w.p; p.c_skip = s->c_skip.p;
    p.c_pad_block = (uint32_t)s->c_pad_block;
    p.t_pos_ptr = s->title->pos_ptr.p; p.t_pos = s->title->pos.p;
    p.b_pos_ptr = s->body->pos_ptr.p; p.b_pos = s->body->pos.p;
    if (pl.any_phrase) {
        for (int x = 0; x < 4; x++) { p.x_rec[x] = t.d_x[x].p; p.x_w[x] = t.d_xw[x].p; }
        p.x_cnt = t.d_xcnt.p;
        p.ph_pcnt = t.d_pcnt.p;
    }
    p.prior = in.K ? s->prior.p : nullptr;
    p.k_topics = in.K;
    p.k = in.k;
    p.cb = pl.cb;
    p.cb_flat = pl.cb_flat;
    p.kth_j = pl.kth_j;
    p.exact_all = pl.exact_all ? 1 : 0;
    p.so_key = t.d_so_key.p; p.so_doc = t.d_so_doc.p; p.so_cnt = t.d_so_cnt.p;
    p.q_ticket = r.fused ? s->d_qticket.p : nullptr;
    p.qc_cnt = t.d_qcnt.p;
    p.small_q = nullptr;
    p.small_stride = (uint32_t)pl.small_stride;
    p.small_stage = r.small_staged ? t.d_small_stage.p : nullptr;
    p.small_stage_n = r.small_staged ? t.d_small_stage_n.p : nullptr;
    p.hits = a.turn_rows ? a.turn_rows->hits : in.dev_out ? a.hits_out : s->d_hits.p;
    p.n_hits = a.turn_rows ? a.turn_rows->n_hits : in.dev_out ? a.n_hits_out : sb.one_copy ? reinterpret_cast<int32_t*>(s->d_hits.p + sb.res_rows) : s->d_nhits.p;
    p.masks = n_csets ? t.d_sets.p : in.any_mask ? s->masks.p : nullptr;
    p.mask_words = n_csets ? sb.set_stride : s->mask_words;
    fill_constraint_params(s, cons, sb);
}

// one pinned staging buffer (one H2D copy: enqueue), the workspaces, the kernel parameters
int32_t stage_plan(ss_scorer* s, const CallArgs& a, const BatchInputs& in, const ConstraintPlan& cons, const BatchPlan& pl, const Route& r,
                   StagedBatch& sb, Stamps& t) {
    PlanWriter measure;
    plan_sections(measure, in, cons, pl, sb.p, sb.cp, sb.fp);
    sb.plan_bytes = measure.o;
    SS_TRY(acquire_turn(s, sb.plan_bytes, cons.sets.size(), a.turn_rows, sb));
    PlanWriter w{s->turn[sb.turn].h_plan.p, s->turn[sb.turn].d_plan.p, 0};
    unsigned char* tab = plan_sections(w, in, cons, pl, sb.p, sb.cp, sb.fp);
    // k_score_small's table: the 1024-slot queries first, then the larger ones (launch_score_small)
    for (const std::vector<SmallEnt>* v : {&pl.small_a, &pl.small_b})
        for (const SmallEnt& en : *v) {
            std::memcpy(tab, &en.h, sizeof(SmallHdr));
            std::memcpy(tab + sizeof(SmallHdr), pl.small_lists.data() + en.loff, (size_t)en.h.n_lists * sizeof(SmallList));
            tab += pl.small_stride;
        }
    t.staged = Clock::now();
    SS_TRY(grow_workspaces(s, in, pl, r, sb));
    fill_params(s, a, in, cons, pl, r, sb);
    return SS_OK;
}

// ---- 6. upload and launches ------------------------------------------------------------------------------------------------
// The plan's upload.  *prep_done: k_wave_prep went out with it.
int32_t upload_plan(ss_scorer* s, const BatchInputs& in, const BatchPlan& pl, const Route& r, const StagedBatch& sb, bool* prep_done) {
    ss_ctx* ctx = s->ctx;
    const Turn& t = s->turn[sb.turn];
    // The upload goes out on the context's SECOND stream as soon as the plan is staged — beside the kernels of the previous
    // batch, which read the other device buffer.  (On the one stream the copy sat
    // between two batches: 39 us per batch in the kernel trace with the counter memset, 6 % of the wall time at config 3.)
    *prep_done = false;
    if (!in.dev_out) {
        // results go back to the host: the call waits for them anyway, and a second wait in the middle would only add to a lone
        // query's latency (0.15 ms, of which 0.08 are kernels): copy, kernels and read-back follow each other on the one stream
        SS_HIP(ctx, hipMemcpyAsync(t.d_plan.p, t.h_plan.p, sb.plan_bytes, hipMemcpyHostToDevice, ctx->stream));
        return SS_OK;
    }
    SS_HIP(ctx, hipMemcpyAsync(t.d_plan.p, t.h_plan.p, sb.plan_bytes, hipMemcpyHostToDevice, ctx->comm_stream));
    // k_wave_prep reads the plan and the index, nothing of an earlier batch.  Unpipelined it follows the copy on the second
    // stream and so runs beside the previous batch's kernels (12 us of kernel and one launch gap per batch off the caller's
    // stream); pipelined it is enqueued on the wave stream in front of its k_score_wave (it finds no room beside the previous
    // batch's k_score_wave anyway: 3 x 168 VGPRs per SIMD).
    if (pl.n_fast_slices && !r.pipe) {
        ss::launch_wave_prep(&sb.p, (unsigned)pl.n_fast_slices, t.d_wprep.p, ctx->comm_stream);
        *prep_done = true;
    }
    // ... and the HOST waits for the second stream (~30 us; it has 0.4 ms to spare per batch): the kernels then go out with no
    // cross-stream dependency in front of them (a hipStreamWaitEvent there left 21 us between two batches, and two of
    // them per batch ran the runtime out of signals every ~80 batches: an 8 ms stall)
    SS_HIP(ctx, hipStreamSynchronize(ctx->comm_stream));
    return SS_OK;
}

// the route's streams: a pipelined batch takes the next wave stream (and the one after it for its second kernel)
int32_t bind_streams(ss_scorer* s, const ScoreOptions& opt, Route& r) {
    ss_ctx* ctx = s->ctx;
    r.st = r.wst = r.sst = ctx->stream;
    if (r.pipe || r.pipe_s || r.small_alone) {
        const int n_ws = (int)std::min<int64_t>(ss_ctx::N_WAVE_STREAMS, std::max<int64_t>(1, opt.pipeline));
        const int wi = (int)(s->wave_turn++ % (unsigned)n_ws);
        if (!ctx->wave_stream[wi]) SS_HIP(ctx, hipStreamCreateWithFlags(&ctx->wave_stream[wi], hipStreamNonBlocking));
        r.wst = ctx->wave_stream[wi];
        if (r.pipe_split || r.small_side) {
            const int si = (wi + 1) % n_ws;                        // (n_ws >= 2: "score.pipeline" >= 2)
            if (!ctx->wave_stream[si]) SS_HIP(ctx, hipStreamCreateWithFlags(&ctx->wave_stream[si], hipStreamNonBlocking));
            r.sst = ctx->wave_stream[si];
        }
    }
    if (r.pipe_s) r.sst = r.wst;
    r.small_st = !r.small_staged ? r.st : r.small_alone ? r.wst : r.sst;
    return SS_OK;
}

int32_t enqueue(ss_scorer* s, const BatchInputs& in, const ConstraintPlan& cons, const BatchPlan& pl, const ScoreOptions& opt, Route& r,
                const StagedBatch& sb, Stamps& t) {
    ss_ctx* ctx = s->ctx;
    Turn& turn = s->turn[sb.turn];
    const ScoreParams& p = sb.p;
    const size_t n_csets = cons.sets.size();
    const unsigned n_fast = (unsigned)pl.n_fast_slices;
    bool prep_done = false;
    SS_TRY(upload_plan(s, in, pl, r, sb, &prep_done));
    t.uploaded = Clock::now();
    if (opt.timed) SS_HIP(ctx, hipEventRecord(ctx->ev[1][0], ctx->stream));
    SS_TRY(bind_streams(s, opt, r));
    if (n_csets) {                               // the allowed sets, in front of the kernels that read them (never k_score_wave)
        ss::launch_constraint_masks(&sb.cp, (uint32_t)(n_csets - cons.n_field_only), r.sst);
        if (!cons.fsets.empty()) ss::launch_field_masks(&sb.fp, r.sst);     // range clauses: the sets of clauses alone, and the others in place
        if (pl.n_small && r.small_st != r.sst) SS_HIP(ctx, turn.set_ev.wait_behind(r.sst, r.small_st));
    }
    if (pl.n_small) {                  // writes its queries' hits itself: the caller's stream, like every kernel that does — or stages them
        const int32_t rc_s = ss::launch_score_small(&p, (unsigned)pl.n_small_a, (unsigned)pl.n_small_b, r.small_st);
        if (rc_s != 0) return ctx->fail(SS_ERR_HIP, "k_score_small: %s", hipGetErrorString((hipError_t)rc_s));
    }
    // the phrase matches, in front of the kernel that merges them in (k_score_slices)
    if (pl.any_phrase) ss::launch_phrase(&p, (unsigned)pl.parts.size(), (unsigned)in.n_q, r.sst);
    if (n_fast) {
        if (!prep_done) ss::launch_wave_prep(&p, n_fast, turn.d_wprep.p, r.wst);
        ss::launch_score_wave(&p, n_fast, turn.d_wprep.p, r.wst);
    }
    if (pl.n_slices > n_fast)
        SS_HIP(ctx, ss::launch_score_slices(&p, n_fast, (unsigned)(pl.n_slices - n_fast), in.any_mask, &s->lds_attr, &s->lds_attr_masked, r.sst));
    // the merge, on the caller's stream, behind this batch's k_score_slices
    if (r.pipe_s) SS_HIP(ctx, turn.wave_ev.wait_behind(r.wst, r.st));
    if (r.pipe_split || r.small_side) SS_HIP(ctx, turn.slice_ev.wait_behind(r.sst, r.st));
    if (r.small_alone) SS_HIP(ctx, turn.wave_ev.wait_behind(r.wst, r.st));
    if (r.small_staged) ss::launch_small_copy(&p, (unsigned)pl.n_small, r.st);
    if (!r.fused && pl.n_slices > n_fast) ss::launch_merge_topk(&p, (unsigned)in.n_q, r.st);
    // the merge, on the caller's stream, behind this batch's k_score_wave
    if (r.pipe) SS_HIP(ctx, turn.wave_ev.wait_behind(r.wst, r.st));
    if (!pl.mergeq.empty()) ss::launch_merge_flat(&p, (unsigned)pl.mergeq.size(), r.st);
    if (opt.timed) {                             // (pipelined: from the end of the previous batch's merge to the end of this one's)
        SS_HIP(ctx, hipEventRecord(ctx->ev[1][1], r.st));
        ctx->ev_valid[1] = true;
    }
    SS_HIP(ctx, turn.batch_ev.record(r.st));       // until here the batch reads the turn's buffers; a later reader of its rows records again
    SS_HIP(ctx, hipGetLastError());
    return SS_OK;
}

// ---- 7. host outputs -------------------------------------------------------------------------------------------------------
int32_t read_back(ss_scorer* s, const CallArgs& a, const StagedBatch& sb) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t n_q = (size_t)a.n_q;
    if (sb.one_copy) {
        unsigned char* const hp1 = s->h_res.p;
        SS_HIP(ctx, hipMemcpyAsync(hp1, s->d_hits.p, sb.res_bytes, hipMemcpyDeviceToHost, st));
        SS_HIP(ctx, hipStreamSynchronize(st));
        std::memcpy(a.hits_out, hp1, sb.res_rows * sizeof(ss_hit));
        std::memcpy(a.n_hits_out, hp1 + sb.res_rows * sizeof(ss_hit), n_q * sizeof(int32_t));
        return SS_OK;
    }
    SS_HIP(ctx, hipMemcpyAsync(a.hits_out, s->d_hits.p, sb.res_rows * sizeof(ss_hit), hipMemcpyDefault, st));
    // (the counts through the context's pinned scratch: a small copy into pageable memory is staged and waited for by the runtime on its
    //  own, ~20 us that a copy into pinned memory does not cost)
    const size_t nh_bytes = n_q * sizeof(int32_t);
    if (nh_bytes <= ss_ctx::PIN_SCRATCH) {
        ctx->pin_used = 0;
        int32_t* const hn = ctx->pin<int32_t>(n_q);
        SS_HIP(ctx, hipMemcpyAsync(hn, s->d_nhits.p, nh_bytes, hipMemcpyDeviceToHost, st));
        SS_HIP(ctx, hipStreamSynchronize(st));
        std::memcpy(a.n_hits_out, hn, nh_bytes);
        return SS_OK;
    }
    SS_HIP(ctx, hipMemcpyAsync(a.n_hits_out, s->d_nhits.p, nh_bytes, hipMemcpyDefault, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

// ---- the call --------------------------------------------------------------------------------------------------------------
int32_t score_impl_inner(ss_scorer* s, const CallArgs& a) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    BatchInputs in;
    SS_TRY(fetch_filter_inputs(s, a, in));
    if (a.n_q == 0) return SS_OK;
    const ScorerView view{s->n_docs, s->n_terms, s->title->h_term_ptr, s->body->h_term_ptr, s->prior_max, s->prior_min,
                          s->has_combined, s->clean, s->prior_clean, ctx->cu_count};
    PlanError err;
    ConstraintPlan cons;
    if (const int32_t rc = resolve_constraints(in, view, cons, err)) return ctx->fail(rc, "%s", err.msg);
    Stamps t;
    t.begin = Clock::now();
    SS_TRY(fetch_inputs(s, a, in));
    BatchPlan plan;
    check_filter_assumptions(in, view, plan);
    t.fetched = Clock::now();
    // (the options and the outputs' whereabouts here, not at the top: "score.trace" has always counted them with the plan)
    const ScoreOptions opt = read_options(ctx);
    in.dev_out = a.turn_rows || outputs_on_device(a);
    if (const int32_t rc = plan_batch(in, view, opt, plan, err)) return ctx->fail(rc, "%s", err.msg);
    t.planned = Clock::now();
    Route route = choose_route(plan, in.dev_out, opt);
    StagedBatch sb;
    SS_TRY(stage_plan(s, a, in, cons, plan, route, sb, t));
    SS_TRY(enqueue(s, in, cons, plan, opt, route, sb, t));
    if (opt.trace) {
        auto us = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[score trace] copies in + checks %.0f us, plan (%zu slices) %.0f us, staging %.0f us, H2D + allocs + params %.0f us, launches %.0f us%s\n",
                us(t.begin, t.fetched), plan.n_slices, us(t.fetched, t.planned), us(t.planned, t.staged), us(t.staged, t.uploaded),
                us(t.uploaded, Clock::now()), route.pipe ? " (k_score_wave on the wave stream)" : "");
    }
    if (in.dev_out) return SS_OK;                // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    return read_back(s, a, sb);
}

// no C++ exception may cross the C ABI: host allocation failures come back as SS_ERR_OOM
int32_t score_impl(ss_scorer* s, const CallArgs& a) {
    if (!s) return SS_ERR_INVALID;
    try {
        return score_impl_inner(s, a);
    } catch (const std::bad_alloc&) {
        return s->ctx->fail(SS_ERR_OOM, "ss_score_topk: host allocation failed");
    } catch (const std::exception& e) {
        return s->ctx->fail(SS_ERR_INVALID, "ss_score_topk: %s", e.what());
    }
}

}  // namespace

// ss_similar_topk (similar.hip), ss_related_terms (related.hip): ss_score_topk_masked without phrases, the rows left in the plan
// turn's own device block
int32_t ss::score_into_turn(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const double* topic_probs,
                            const int32_t* mask_id, int32_t k, TurnRows* out, const int32_t* query_len) {
    out->rows = (size_t)n_q * (size_t)k;
    out->n_q = (size_t)n_q;
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, nullptr, nullptr, query_len, topic_probs, k, nullptr, nullptr, mask_id, nullptr, out});
}

// ss_facet_counts (facet.hip): steps 1 and 2 of a scoring call for the mask ids, constraint arrays and range clauses alone, then the
// sets' tables through the plan turn's buffers and the builders on the context's stream.  The caller holds the context's lock and
// has set the device.
int32_t ss::allowed_sets_into_turn(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const int32_t* mask_id, const QueryConstraints* cons,
                                   const QueryRanges* ranges, AllowedSets* out) {
    ss_ctx* ctx = s->ctx;
    TurnRows no_rows;                            // (stands for the outputs fetch_filter_inputs would check: this call writes no rows)
    const CallArgs a{n_q, q_ptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, mask_id, cons, &no_rows, ranges};
    BatchInputs in;
    SS_TRY(fetch_filter_inputs(s, a, in));
    const ScorerView view{s->n_docs, s->n_terms, s->title->h_term_ptr, s->body->h_term_ptr, s->prior_max, s->prior_min,
                          s->has_combined, s->clean, s->prior_clean, ctx->cu_count};
    PlanError err;
    ConstraintPlan cp;
    if (const int32_t rc = resolve_constraints(in, view, cp, err)) return ctx->fail(rc, "%s", err.msg);
    // ---- the last check has passed
    StagedBatch sb;
    PlanWriter measure;
    constraint_sections(measure, cp, sb.cp, sb.fp);
    sb.plan_bytes = measure.o;
    const size_t n_csets = cp.sets.size();
    SS_TRY(acquire_turn(s, sb.plan_bytes, n_csets, nullptr, sb));
    Turn& t = s->turn[sb.turn];
    if (n_csets) {
        PlanWriter w{t.h_plan.p, t.d_plan.p, 0};
        constraint_sections(w, cp, sb.cp, sb.fp);
        fill_constraint_params(s, cp, sb);
        hipStream_t st = ctx->stream;
        SS_HIP(ctx, hipMemcpyAsync(t.d_plan.p, t.h_plan.p, sb.plan_bytes, hipMemcpyHostToDevice, st));
        ss::launch_constraint_masks(&sb.cp, (uint32_t)(n_csets - cp.n_field_only), st);
        if (!cp.fsets.empty()) ss::launch_field_masks(&sb.fp, st);
        SS_HIP(ctx, hipGetLastError());
        SS_HIP(ctx, t.batch_ev.record(st));      // (the caller records again behind its own reader of the sets)
    }
    out->set_of.assign((size_t)n_q, -1);
    if (in.any_mask) out->set_of = in.mask;
    out->words = n_csets ? t.d_sets.p : in.any_mask ? s->masks.p : nullptr;
    out->stride = n_csets ? sb.set_stride : s->mask_words;
    out->turn = sb.turn;
    return SS_OK;
}

extern "C" {

int32_t ss_score_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                      const double* topic_probs, int32_t k, ss_hit* hits_out, int32_t* n_hits_out) {
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, nullptr, nullptr, query_len, topic_probs, k, hits_out, n_hits_out, nullptr, nullptr});
}

int32_t ss_score_topk_phrase(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const uint32_t* p_ptr,
                             const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, int32_t k,
                             ss_hit* hits_out, int32_t* n_hits_out) {
    if (s && !p_ptr) return s->ctx->fail(SS_ERR_INVALID, "ss_score_topk_phrase: p_ptr is NULL");
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs, k, hits_out, n_hits_out, nullptr, nullptr});
}

int32_t ss_score_topk_masked(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const uint32_t* p_ptr,
                             const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, const int32_t* mask_id,
                             int32_t k, ss_hit* hits_out, int32_t* n_hits_out) {
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs, k, hits_out, n_hits_out, mask_id, nullptr});
}

int32_t ss_score_topk_constrained(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const uint32_t* p_ptr,
                                  const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, const int32_t* mask_id,
                                  const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                                  int32_t k, ss_hit* hits_out, int32_t* n_hits_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs, k, hits_out, n_hits_out, mask_id, &cons});
}

int32_t ss_score_topk_filtered(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const uint32_t* p_ptr,
                               const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, const int32_t* mask_id,
                               const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                               const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t k, ss_hit* hits_out, int32_t* n_hits_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return score_impl(s, CallArgs{n_q, q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs, k, hits_out, n_hits_out, mask_id, &cons, nullptr, &ranges});
}

// Batches in flight with HOST results: submit runs the batch like a call with device outputs (nothing waits, consecutive batches
// overlap on the device) into the slot's own device buffers; collect waits for that batch alone and copies its rows to the caller.
// The host's plan for batch i+1 and the copy-out of batch i-1 then run under the kernels of batch i.
int32_t ss_score_topk_submit(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const uint32_t* p_ptr,
                             const uint32_t* p_terms, const int32_t* query_len, const double* topic_probs, int32_t k, uint64_t* ticket_out) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!ticket_out) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_submit: ticket_out is NULL");
    *ticket_out = 0;
    if (n_q < 0 || k < 1 || k > SS_MAX_TOPK) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_submit: n_q < 0 or k outside 1 .. %d", SS_MAX_TOPK);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    ss_scorer::AsyncSlot* a = nullptr;
    for (auto& c : s->aslot)
        if (!c.ticket) { a = &c; break; }
    if (!a) return ctx->fail(SS_ERR_STATE, "ss_score_topk_submit: %d batches in flight already (ss_score_topk_collect one first)", (int)ss_scorer::INFLIGHT);
    const size_t rows = (size_t)n_q * (size_t)k;
    if (a->hits.n < rows) SS_HIP(ctx, a->hits.alloc(rows + rows / 4));
    if (a->n_hits.n < (size_t)n_q) SS_HIP(ctx, a->n_hits.alloc((size_t)n_q + 64));
    a->pin_mode = ctx->opt("score.collect_pinned", 0) != 0;
    if (a->pin_mode) {
        const size_t bytes = rows * sizeof(ss_hit) + (size_t)n_q * sizeof(int32_t);
        if (a->pin_cap < bytes) {
            ctx->pin_free(a->pin, a->pin_cap);
            a->pin = ctx->pin_alloc(bytes, &a->pin_cap);
            if (!a->pin) { a->pin_cap = 0; return ctx->fail(SS_ERR_OOM, "ss_score_topk_submit: no pinned host memory for %zu bytes of results", bytes); }
        }
        if (!s->out_stream) SS_HIP(ctx, hipStreamCreateWithFlags(&s->out_stream, hipStreamNonBlocking));
    }
    if (a->pin_n_cap < (size_t)n_q * sizeof(int32_t)) {
        if (a->pin_n) ctx->pin_free(a->pin_n, a->pin_n_cap);
        a->pin_n = ctx->pin_alloc(std::max<size_t>((size_t)n_q * sizeof(int32_t), 4096), &a->pin_n_cap);
        if (!a->pin_n) a->pin_n_cap = 0;                                   // (no pinned memory: collect copies the counts straight out)
    }
    if (n_q) {
        const int32_t rc = score_impl(s, CallArgs{n_q, q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs, k, a->hits.p, a->n_hits.p, nullptr, nullptr});
        if (rc != SS_OK) return rc;
        // Only an event behind the batch's kernels is recorded here; the rows are copied when they are COLLECTED.  [Enqueued at
        // submit, the device-to-host copy waits in the copy engine's in-order queue for this batch's merge and holds up the NEXT
        // batch's plan upload behind it (submit then took 0.41 ms instead of 0.13); done by a kernel on the caller's stream it sat
        // between two merges that the wave kernel stretches (period 0.48 ms instead of 0.345), on a stream of its own it shared a
        // hardware queue with a wave stream (0.59).  At collect time the batch is finished, the copy takes its 85 us and blocks
        // nothing: the host spends 0.13 ms in submit and 0.09 in collect per batch, under the 0.345 ms the device needs.]
        SS_HIP(ctx, a->ev.record(ctx->stream));
    }
    a->n_q = n_q;
    a->k = k;
    a->ticket = s->next_ticket++;
    *ticket_out = a->ticket;
    return SS_OK;
}

int32_t ss_score_topk_collect(ss_scorer* s, uint64_t ticket, ss_hit* hits_out, int32_t* n_hits_out) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    ss_scorer::AsyncSlot* a = nullptr;
    // everything the unlocked part needs is read HERE, under the context's lock: the options map, the slot's fields and the scorer's
    // stream may be written by a thread that submits or sets an option meanwhile (ctx->opt() is an unlocked map lookup)
    bool trace = false, pin_mode = false;
    int32_t n_q = 0, k = 0;
    hipEvent_t ev = nullptr;
    hipStream_t out_stream = nullptr;
    const ss_hit* d_hits = nullptr;
    const int32_t* d_n = nullptr;
    void* pin = nullptr;
    void* pin_n = nullptr;
    {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        if (!hits_out || !n_hits_out) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_collect: NULL output");
        for (auto& c : s->aslot)
            if (ticket && c.ticket == ticket && !c.collecting) { a = &c; break; }
        if (!a) return ctx->fail(SS_ERR_INVALID, "ss_score_topk_collect: no batch in flight with ticket %llu", (unsigned long long)ticket);
        SS_HIP(ctx, hipSetDevice(ctx->device));
        a->collecting = true;                   // (a second collect of the same ticket from another thread is refused, not raced)
        trace = ctx->opt("score.trace", 0) != 0;
        pin_mode = a->pin_mode;
        n_q = a->n_q; k = a->k; ev = a->ev.h; out_stream = s->out_stream;
        d_hits = a->hits.p; d_n = a->n_hits.p; pin = a->pin; pin_n = a->pin_n;
    }
    // (the wait and the copies run outside the context's lock: another thread may submit the next batch meanwhile; the slot itself
    // stays this call's until its ticket is cleared below)
    if (n_q) {
        const auto tw0 = std::chrono::steady_clock::now();
        hipError_t e = hipEventSynchronize(ev);
        const auto tw1 = std::chrono::steady_clock::now();
        const size_t rows = (size_t)n_q * (size_t)k;
        const size_t hb = rows * sizeof(ss_hit), nb = (size_t)n_q * sizeof(int32_t);
        if (pin_mode) {
            // through the slot's pinned block on the copy engine, then a host memcpy
            if (e == hipSuccess) e = hipMemcpyAsync(pin, d_hits, hb, hipMemcpyDeviceToHost, out_stream);
            if (e == hipSuccess) e = hipMemcpyAsync(static_cast<unsigned char*>(pin) + hb, d_n, nb, hipMemcpyDeviceToHost, out_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(out_stream);
            if (e == hipSuccess) {
                std::memcpy(hits_out, pin, hb);
                std::memcpy(n_hits_out, static_cast<unsigned char*>(pin) + hb, nb);
            }
        } else {
            if (e == hipSuccess) e = hipMemcpy(hits_out, d_hits, hb, hipMemcpyDeviceToHost);
            if (pin_n) {                                                   // the counts: device -> the slot's pinned block -> the caller
                if (e == hipSuccess) e = hipMemcpy(pin_n, d_n, nb, hipMemcpyDeviceToHost);
                if (e == hipSuccess) std::memcpy(n_hits_out, pin_n, nb);
            } else if (e == hipSuccess) {
                e = hipMemcpy(n_hits_out, d_n, nb, hipMemcpyDeviceToHost);
            }
        }
        if (trace) fprintf(stderr, "[score trace] collect: waited %.0f us for the batch, copies %.0f us\n", std::chrono::duration<double, std::micro>(tw1 - tw0).count(),
                           std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw1).count());
        if (e != hipSuccess) {
            std::lock_guard<std::recursive_mutex> lk(ctx->mu);
            a->ticket = 0;
            a->collecting = false;
            return ctx->fail(SS_ERR_HIP, "ss_score_topk_collect: %s", hipGetErrorString(e));
        }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    a->ticket = 0;
    a->collecting = false;
    return SS_OK;
}

}  // extern "C"
