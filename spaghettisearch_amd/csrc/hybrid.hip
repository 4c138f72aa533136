// hybrid.hip — ss_score_docs, ss_fuse_hits and ss_hybrid_topk: the lexical row of any given doc, and a lexical and a vector list of one
// query fused into one ranked, paged list.  A step file beside collapse.hip and vector.hip: no scoring kernel and no
// vector kernel edited; ss_hybrid_topk makes its two windows with ss::score_into_turn and ss_vector_topk as they are.
//
//   checks               arguments, fusion parameters, q_ptr, host counts — all before anything is enqueued (hybrid_plan.hpp)
//   the queries' table   qmag [n_q] | probs [n_q][K] | ptr [n_q + 1] | tokens, through one of the TURNS hybrid turns (a QueryTurn, as
//                        ss_explain_hits' table; the doubles first, so that they are aligned)
//   k_score_docs         16 lanes per (query, doc).  Lane l of a group takes the (token, field) pairs l, l + 16, ...: pair 2 i is token
//                        i's title list, pair 2 i + 1 its body list, searched with the merge's lower_bound_interp over the scoring
//                        records; the weight comes from the table's float32 weights.  Behind every 16 pairs the group's weights go
//                        round by shuffle and EVERY lane adds them in pair order, i.e. token order per field — no atomics, one order.
//                        Lane 0 then calls final_rank / topic_dot and stores the 40-byte row.
//   k_fuse_hits          one workgroup per query.  Every valid row of both lists becomes the key doc << 11 | list << 10 | position;
//                        the keys are sorted in LDS over the next power of two (hitwin::bitonic_sort, the scheme of k_collapse_hits).
//                        A doc's rows then lie side by side, the lexical ones first, each list's in position order: a key whose
//                        neighbour below has another (doc, list) is a first occurrence, one whose neighbour has another doc starts a
//                        candidate.  A workgroup prefix sum over the starts numbers the candidates (in doc order); first occurrences
//                        write their rank to their candidate.  A candidate that lacks a side takes a slot of that side's gather list.
//   k_score_docs / k_vec_hit_scores over the gather lists (sized by n_q * k_vec and n_q * k_lex; they leave on the device counts)
//   k_fuse_page          one workgroup per query: the score of every candidate (hybrid_plan.hpp: fuse_score), the pairs (order key,
//                        candidate number) sorted in LDS — the candidate number ascends with the doc, so it breaks ties as the
//                        definition does — and the page copied out, five lanes to a row as hitwin::copy_page does, from whichever
//                        array holds a candidate's row.
// The lexical window in, the outputs' way back and the paging: hit_window.hpp.
#include "hit_window.hpp"
#include "hybrid_plan.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace hw = ss::hitwin;
namespace hy = ss::hybrid;

static_assert(SS_FUSE_RRF == hy::MODE_RRF && SS_FUSE_WEIGHTED == hy::MODE_WEIGHTED, "hybrid_plan.hpp states the ABI's modes");
static_assert(sizeof(ss_fuse_params) == 24 && sizeof(ss_fused) == 16 && alignof(ss_fused) == 8, "the ABI's layouts");

// ---- the row of a given doc --------------------------------------------------------------------------------------------------
constexpr int SD_TPB = 256;
constexpr uint32_t SD_GROUP = 16;                         // lanes per (query, doc)

struct ScoreDocsParams {
    const uint64_t *t_ptr, *b_ptr;
    const Rec *t_rec, *b_rec;
    const float *t_w, *b_w;
    const double *t_mag, *b_mag;
    uint64_t t_terms, b_terms, n_terms, n_docs;
    const double* prior;                                  // [n_docs][k_topics] or NULL
    int32_t k_topics;
    const double* qmag;                                   // [n_q]
    const double* probs;                                  // [n_q][k_topics] or NULL
    const uint32_t *q_ptr, *q_terms;                      // the call's table: [n_q + 1] offsets into the tokens
    const uint32_t* docs;                                 // [n_q][k_in]
    const int32_t* n_in;                                  // [n_q]
    ss_hit* out;                                          // [n_q][k_in]
    uint32_t k_in;
    uint64_t total;                                       // n_q * k_in
};

__global__ __launch_bounds__(SD_TPB) void k_score_docs(ScoreDocsParams p) {
    const uint64_t pair = ((uint64_t)blockIdx.x * SD_TPB + threadIdx.x) / SD_GROUP;
    const uint32_t sub = threadIdx.x & (SD_GROUP - 1u);
    if (pair >= p.total) return;                          // (a whole group)
    const uint64_t q = pair / p.k_in;
    const uint32_t j = (uint32_t)(pair - q * p.k_in);
    if (j >= hw::window_len(p.n_in[q], p.k_in)) return;
    const uint32_t d = p.docs[pair];
    ss_hit h;
    h.doc = d; h._pad = 0; h.title = 0.0; h.body = 0.0; h.pagerank = 0.0; h.final = 0.0;
    if ((uint64_t)d >= p.n_docs) {
        if (sub == 0) p.out[pair] = h;
        return;
    }
    const uint32_t q0 = p.q_ptr[q], n_pairs = 2u * (p.q_ptr[q + 1] - q0);      // (the host keeps a query below 2^31 tokens)
    const uint32_t g_shift = (threadIdx.x & 63u) & ~(SD_GROUP - 1u);            // the group's first lane inside its wave
    double T = 0.0, B = 0.0;
    uint32_t any = 0;                                     // bit 0: a title posting was found, bit 1: a body posting
    for (uint32_t base = 0; base < n_pairs; base += SD_GROUP) {                 // (the same trips in every lane of the group)
        const uint32_t pr = base + sub;
        float w = 0.0f;
        bool found = false;
        if (pr < n_pairs) {
            const uint32_t term = p.q_terms[q0 + (pr >> 1)];
            const bool body = pr & 1u;
            if (term != SS_UNKNOWN_TERM && (uint64_t)term < p.n_terms && (uint64_t)term < (body ? p.b_terms : p.t_terms)) {
                const uint64_t* const ptr = body ? p.b_ptr : p.t_ptr;
                const uint64_t lo = ptr[term], hi = ptr[term + 1];
                const uint64_t addr = (uint64_t)((body ? p.b_rec : p.t_rec) + lo);
                const uint32_t len = (uint32_t)(hi - lo);                       // (one posting list: shorter than 2^32, as in the merge)
                const uint32_t pos = lower_bound_interp(addr, 0u, len, d);
                if (pos < len && load_doc(addr, pos) == d) {
                    w = (body ? p.b_w : p.t_w)[lo + pos];
                    found = true;
                }
            }
        }
        const uint32_t fm = (uint32_t)(__ballot(found) >> g_shift) & 0xFFFFu;  // the group's lanes are all here
#pragma unroll
        for (uint32_t i = 0; i < SD_GROUP; i++) {
            const float wi = __shfl(w, (int)i, (int)SD_GROUP);
            if ((fm >> i) & 1u) {
                if (i & 1u) B += (double)wi;
                else T += (double)wi;
            }
        }
        any |= ((fm & 0x5555u) ? 1u : 0u) | ((fm & 0xAAAAu) ? 2u : 0u);
    }
    if (sub != 0) return;
    const double mt = (any & 1u) ? p.t_mag[d] : 1.0, mb = (any & 2u) ? p.b_mag[d] : 1.0;
    const double sqd = (p.probs && p.prior) ? topic_dot(p.prior, p.probs + q * (uint64_t)p.k_topics, p.k_topics, d) : 0.0;
    final_rank(T, B, mt, mb, p.qmag[q], sqd, h.title, h.body, h.final);
    h.pagerank = sqd;
    p.out[pair] = h;
}

// ---- the union of two lists ----------------------------------------------------------------------------------------------------
constexpr uint64_t FZ_DEAD = ~0ull;                       // the key of a slot without a valid row: behind every live key
constexpr uint32_t FZ_POS_BITS = 10;                      // position < SS_MAX_TOPK = 2^10; bit 10: the list (1 = vector)
static_assert(SS_MAX_TOPK == (1 << FZ_POS_BITS), "a window index takes FZ_POS_BITS bits of a key");

struct FuseParams {
    const ss_hit* lex;                                    // [n_q][k_lex]
    const int32_t* n_lex;
    const ss_vec_hit* vec;                                // [n_q][k_vec]
    const int32_t* n_vec;
    uint64_t n_docs;
    uint32_t k_lex, k_vec, n_q;
    uint32_t* cand;                                       // [n_q][3][k_lex + k_vec]: doc | lex_rank + (vec_rank << 16) | slot
    int32_t* counts;                                      // [3][n_q]: candidates | docs without a lexical row | docs without a vector score
    uint32_t* miss_docs;                                  // [n_q][k_vec] the docs without a lexical row
    ss_hit* miss_vec_rows;                                // [n_q][k_lex] .doc = the docs without a vector score
    // k_fuse_page
    const ss_hit* miss_rows;                              // [n_q][k_vec] from k_score_docs
    const int32_t* miss_scores;                           // [n_q][k_lex] from k_vec_hit_scores
    ss_fuse_params fp;
    uint32_t first, k;
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;
    ss_fused* fused_out;                                  // nullable
    int32_t* n_union_out;                                 // nullable
};

// the workgroup's exclusive prefix sum of `mine` (one value per thread) and the total; s_wsum: BLOCK / 64 words.  Ends behind a barrier.
template <int BLOCK>
__device__ __forceinline__ uint32_t block_scan(uint32_t mine, uint32_t* s_wsum, uint32_t* total) {
    constexpr uint32_t WAVES = BLOCK / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, sum = 0;
#pragma unroll
    for (uint32_t v = 0; v < WAVES; v++) {
        const uint32_t w = s_wsum[v];
        if (v < wave) before += w;
        sum += w;
    }
    *total = sum;
    __syncthreads();
    return before;
}

// One workgroup of BLOCK threads per query; both lists together hold up to CAP = PER * BLOCK rows (the launcher picks the instance).
template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_fuse_hits(FuseParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    __shared__ uint64_t s_key[CAP];                       // sorted keys
    __shared__ uint32_t s_doc[CAP];                       // by candidate: its doc
    __shared__ uint16_t s_lr[CAP], s_vr[CAP];             // by candidate: its ranks, 0 = absent
    __shared__ uint32_t s_wsum[BLOCK / 64];
    __shared__ uint32_t s_cnt[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n_l = hw::window_len(p.n_lex[q], p.k_lex), n_v = hw::window_len(p.n_vec[q], p.k_vec);
    const uint32_t n = n_l + n_v;                         // <= k_lex + k_vec <= CAP: checked by the launcher
    const uint32_t np = hw::pow2_at_least(n);
    const ss_hit* const lex = p.lex + (size_t)q * p.k_lex;
    const ss_vec_hit* const vec = p.vec + (size_t)q * p.k_vec;
    // ---- the keys
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint64_t key = FZ_DEAD;
        if (j < n) {
            const bool v = j >= n_l;
            const uint32_t pos = v ? j - n_l : j;
            const uint32_t d = v ? vec[pos].doc : lex[pos].doc;
            if ((uint64_t)d < p.n_docs) key = (uint64_t)d << (FZ_POS_BITS + 1) | (uint64_t)(v ? 1u : 0u) << FZ_POS_BITS | pos;
        }
        s_key[j] = key;
    }
    for (uint32_t c = tid; c < CAP; c += BLOCK) { s_lr[c] = 0; s_vr[c] = 0; }
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t a = s_key[i], b = s_key[o];
        if ((a > b) == up) {
            s_key[i] = b;
            s_key[o] = a;
        }
    });
    // ---- number the candidates: thread t owns sorted slots [t * PER, (t + 1) * PER)
    uint32_t mine = 0;
#pragma unroll
    for (int c = 0; c < PER; c++) {
        const uint32_t i = tid * PER + c;
        if (i < np && s_key[i] != FZ_DEAD && (i == 0 || (s_key[i - 1] >> (FZ_POS_BITS + 1)) != (s_key[i] >> (FZ_POS_BITS + 1)))) mine++;
    }
    uint32_t n_u = 0;
    uint32_t run = block_scan<BLOCK>(mine, s_wsum, &n_u); // candidates that start before this thread's slots
#pragma unroll
    for (int c = 0; c < PER; c++) {
        const uint32_t i = tid * PER + c;
        if (i >= np) break;
        const uint64_t key = s_key[i];
        if (key == FZ_DEAD) break;                        // (the live keys are the first)
        const uint64_t below = i ? s_key[i - 1] : FZ_DEAD;
        const bool starts = !i || (below >> (FZ_POS_BITS + 1)) != (key >> (FZ_POS_BITS + 1));
        const bool first_in_list = !i || (below >> FZ_POS_BITS) != (key >> FZ_POS_BITS);
        if (starts) run++;
        const uint32_t cand = run - 1;                    // < n_u <= n <= CAP
        if (starts) s_doc[cand] = (uint32_t)(key >> (FZ_POS_BITS + 1));
        if (first_in_list) {
            const uint16_t rank = (uint16_t)(((uint32_t)key & ((1u << FZ_POS_BITS) - 1u)) + 1u);
            if ((key >> FZ_POS_BITS) & 1u) s_vr[cand] = rank;
            else s_lr[cand] = rank;
        }
    }
    __syncthreads();
    // ---- the candidates and the gather lists of the docs that lack a side
    const size_t U = (size_t)p.k_lex + p.k_vec;
    uint32_t* const c_doc = p.cand + (size_t)q * 3 * U;
    uint32_t* const c_rk = c_doc + U;
    uint32_t* const c_slot = c_rk + U;
    for (uint32_t c = tid; c < n_u; c += BLOCK) {
        const uint32_t d = s_doc[c], lr = s_lr[c], vr = s_vr[c];
        uint32_t slot = 0;
        if (!lr) {                                        // in the vector list only: at most n_v <= k_vec of them
            slot = atomicAdd(&s_cnt[0], 1u);
            p.miss_docs[(size_t)q * p.k_vec + slot] = d;
        } else if (!vr) {                                 // in the lexical list only: at most n_l <= k_lex of them
            slot = atomicAdd(&s_cnt[1], 1u);
            p.miss_vec_rows[(size_t)q * p.k_lex + slot].doc = d;
        }
        c_doc[c] = d;
        c_rk[c] = lr | vr << 16;
        c_slot[c] = slot;
    }
    __syncthreads();
    if (tid == 0) {
        p.counts[q] = (int32_t)n_u;
        p.counts[(size_t)p.n_q + q] = (int32_t)s_cnt[0];
        p.counts[2 * (size_t)p.n_q + q] = (int32_t)s_cnt[1];
    }
}

// what a candidate's completed row holds
struct Completed {
    const ss_hit* row;
    int32_t vec_score;
    uint32_t lex_rank, vec_rank;
};
__device__ __forceinline__ Completed completed(const FuseParams& p, uint32_t q, uint32_t c) {
    const size_t U = (size_t)p.k_lex + p.k_vec;
    const uint32_t* const c_rk = p.cand + (size_t)q * 3 * U + U;
    const uint32_t rk = c_rk[c], slot = c_rk[U + c];
    Completed r;
    r.lex_rank = rk & 0xFFFFu;
    r.vec_rank = rk >> 16;
    r.row = r.lex_rank ? p.lex + (size_t)q * p.k_lex + (r.lex_rank - 1u) : p.miss_rows + (size_t)q * p.k_vec + slot;
    r.vec_score = r.vec_rank ? p.vec[(size_t)q * p.k_vec + (r.vec_rank - 1u)].score : p.miss_scores[(size_t)q * p.k_lex + slot];
    return r;
}
__device__ __forceinline__ double completed_score(const FuseParams& p, const Completed& r) {
    return hy::fuse_score(p.fp.mode, p.fp.rrf_c, p.fp.w_lex, p.fp.w_vec, r.lex_rank, r.vec_rank, r.row->final, r.vec_score);
}

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_fuse_page(FuseParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    constexpr uint32_t PAGE = CAP < SS_MAX_TOPK ? CAP : SS_MAX_TOPK;
    __shared__ uint64_t s_key[CAP];                       // the order keys
    __shared__ uint32_t s_tag[CAP];                       // the candidate of a key; ~0 in a slot behind the candidates
    __shared__ uint64_t s_src[PAGE];                      // by output slot: the address of its row
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t n_u = (uint32_t)p.counts[q];
    n_u = n_u > CAP ? CAP : n_u;                          // (k_fuse_hits wrote it: <= k_lex + k_vec <= CAP)
    const uint32_t np = hw::pow2_at_least(n_u);
    for (uint32_t c = tid; c < np; c += BLOCK) {
        uint64_t key = hy::KEY_NAN;
        uint32_t tag = 0xFFFFFFFFu;
        if (c < n_u) {
            key = hy::order_key(completed_score(p, completed(p, q, c)));
            tag = c;
        }
        s_key[c] = key;
        s_tag[c] = tag;
    }
    __syncthreads();
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t ka = s_key[i], kb = s_key[o];
        const uint32_t ta = s_tag[i], tb = s_tag[o];
        if ((ka != kb ? ka > kb : ta > tb) == up) {
            s_key[i] = kb; s_tag[i] = tb;
            s_key[o] = ka; s_tag[o] = ta;
        }
    });
    // ---- the page: sorted positions [first, first + n_out), all below n_u
    const uint32_t n_out = hw::page_len(n_u, p.first, p.k);                   // <= k <= PAGE (the launcher), <= n_u <= CAP
    for (uint32_t r = tid; r < n_out; r += BLOCK) {
        const Completed cr = completed(p, q, s_tag[p.first + r]);
        s_src[r] = (uint64_t)cr.row;
        if (p.fused_out) {
            ss_fused f;
            const uint64_t bits = hy::stored_bits(completed_score(p, cr));
            f.score = __longlong_as_double((long long)bits);
            f.vec_score = cr.vec_score;
            f.lex_rank = (uint16_t)cr.lex_rank;
            f.vec_rank = (uint16_t)cr.vec_rank;
            p.fused_out[(size_t)q * p.k + r] = f;
        }
    }
    __syncthreads();
    // the rows as 8-byte words, lane x word x % 5 of output slot x / 5 (hitwin::copy_page's layout, a source address per slot)
    uint64_t* const out_w = reinterpret_cast<uint64_t*>(p.hits_out + (size_t)q * p.k);
    for (uint32_t x = tid; x < n_out * hw::ROW_WORDS; x += BLOCK) {
        const uint32_t r = x / hw::ROW_WORDS, w = x - r * hw::ROW_WORDS;
        out_w[x] = reinterpret_cast<const uint64_t*>(s_src[r])[w];
    }
    if (tid == 0) {
        p.n_hits_out[q] = (int32_t)n_out;
        if (p.n_union_out) p.n_union_out[q] = (int32_t)n_u;
    }
}

// both lists together up to 256 rows: one wave, four rows a lane; longer ones: four waves, up to eight rows a lane
constexpr int FZ_SMALL = 64, FZ_SMALL_PER = 4, FZ_LARGE = 256, FZ_LARGE_PER = 8;
static_assert(FZ_LARGE * FZ_LARGE_PER >= 2 * SS_MAX_TOPK, "the fuse kernels hold both windows in LDS");

// ---- host side -------------------------------------------------------------------------------------------------------------
// The query arrays of a call on the host, checked, and their table in the pinned block of the next hybrid turn.
struct QueryArrays {
    std::vector<uint32_t> ptr;
    std::vector<int32_t> qlen;
    std::vector<double> probs;
    const uint32_t* q_terms = nullptr;
    bool has_probs = false;
};
int32_t query_arrays_fetch(ss_scorer* s, const char* entry, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                           const double* topic_probs, QueryArrays* qa) {
    ss_ctx* ctx = s->ctx;
    const size_t nq = (size_t)n_q;
    qa->ptr.resize(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, entry, "q", q_ptr, nq, qa->ptr.data()));
    if (qa->ptr[nq] - qa->ptr[0] && !q_terms) return ctx->fail(SS_ERR_INVALID, "%s: q_terms is NULL", entry);
    for (size_t q = 0; q < nq; q++)
        if (qa->ptr[q + 1] - qa->ptr[q] >= (1u << 30)) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: query %zu has 2^30 tokens or more", entry, q);
    qa->q_terms = q_terms;
    qa->qlen.resize(nq);
    if (query_len) SS_HIP(ctx, ss::copy_in(ctx->stream, qa->qlen.data(), query_len, nq * sizeof(int32_t)));
    else for (size_t q = 0; q < nq; q++) qa->qlen[q] = (int32_t)(qa->ptr[q + 1] - qa->ptr[q]);
    qa->has_probs = topic_probs && s->k_topics > 0;
    if (qa->has_probs) {
        qa->probs.resize(nq * (size_t)s->k_topics);
        SS_HIP(ctx, ss::copy_in(ctx->stream, qa->probs.data(), topic_probs, qa->probs.size() * sizeof(double)));
    }
    return SS_OK;
}

// Waits for the turn's last reader, fills its pinned block and enqueues the upload; sets the table's pointers in p.  The caller records
// turn.ev behind the last kernel that reads the table.
int32_t query_table_up(ss_scorer* s, QueryTurn& turn, const QueryArrays& qa, ScoreDocsParams* p) {
    ss_ctx* ctx = s->ctx;
    SS_HIP(ctx, turn.ev.wait());
    const size_t nq = qa.ptr.size() - 1, tok0 = qa.ptr[0], n_tok = qa.ptr[nq] - tok0;
    const size_t n_dbl = nq + qa.probs.size();
    const size_t words = 2 * n_dbl + nq + 1 + n_tok;
    SS_HIP(ctx, turn.h_q.ensure(words * sizeof(uint32_t)));
    SS_HIP(ctx, ensure(turn.d_q, words));
    double* const h_d = turn.h_q.as<double>();
    for (size_t q = 0; q < nq; q++) h_d[q] = std::sqrt((double)qa.qlen[q]);       // get_metadata.go:53, as the scoring call's plan
    if (!qa.probs.empty()) std::memcpy(h_d + nq, qa.probs.data(), qa.probs.size() * sizeof(double));
    uint32_t* const h_w = turn.h_q.as<uint32_t>() + 2 * n_dbl;
    for (size_t q = 0; q <= nq; q++) h_w[q] = qa.ptr[q] - (uint32_t)tok0;
    SS_HIP(ctx, ss::copy_in(ctx->stream, h_w + nq + 1, qa.q_terms ? qa.q_terms + tok0 : nullptr, n_tok * sizeof(uint32_t)));
    SS_HIP(ctx, hipMemcpyAsync(turn.d_q.p, turn.h_q.p, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const double* const d_d = reinterpret_cast<const double*>(turn.d_q.p);
    p->qmag = d_d;
    p->probs = qa.has_probs ? d_d + nq : nullptr;
    p->q_ptr = turn.d_q.p + 2 * n_dbl;
    p->q_terms = p->q_ptr + nq + 1;
    return SS_OK;
}

void tables_of(const ss_scorer* s, ScoreDocsParams* p) {
    p->t_ptr = s->title->term_ptr.p; p->t_rec = s->t_rec.p; p->t_w = s->title->post_w.p; p->t_mag = s->title->mag.p; p->t_terms = s->title->n_terms;
    p->b_ptr = s->body->term_ptr.p; p->b_rec = s->b_rec.p; p->b_w = s->body->post_w.p; p->b_mag = s->body->mag.p; p->b_terms = s->body->n_terms;
    p->n_terms = s->n_terms;
    p->n_docs = s->n_docs;
    p->prior = s->k_topics ? s->prior.p : nullptr;
    p->k_topics = s->k_topics;
}

// k_score_docs over docs / counts in device memory; p holds the tables and the queries' table
hipError_t launch_score_docs(ScoreDocsParams p, const uint32_t* docs, const int32_t* n_in, ss_hit* out, size_t n_q, uint32_t k_in, hipStream_t st) {
    p.docs = docs;
    p.n_in = n_in;
    p.out = out;
    p.k_in = k_in;
    p.total = (uint64_t)n_q * k_in;
    hipLaunchKernelGGL(k_score_docs, dim3(ss::div_up(p.total * SD_GROUP, SD_TPB)), dim3(SD_TPB), 0, st, p);   // (total < 2^31: below 2^27 blocks)
    return hipGetLastError();
}

int32_t score_docs_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                        const double* topic_probs, int32_t k_in, const uint32_t* docs, const int32_t* n_in, ss_hit* hits_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and the output is not touched before the last of them has passed
    if (n_q < 0 || !q_ptr) return ctx->fail(SS_ERR_INVALID, "ss_score_docs: q_ptr is NULL or n_q < 0");
    if (k_in < 1) return ctx->fail(SS_ERR_INVALID, "ss_score_docs: k_in = %d must be >= 1", k_in);
    if (k_in > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_score_docs: k_in = %d exceeds SS_MAX_TOPK = %d", k_in, SS_MAX_TOPK);
    if ((uint64_t)n_q * (uint64_t)k_in >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_score_docs: n_q * k_in = %llu rows, must be below 2^31", (unsigned long long)((uint64_t)n_q * (uint64_t)k_in));
    if (n_q == 0) return SS_OK;
    if (!docs || !n_in || !hits_out) return ctx->fail(SS_ERR_INVALID, "ss_score_docs: docs, n_in or hits_out is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q, n_rows = nq * (size_t)k_in;
    QueryArrays qa;
    SS_TRY(query_arrays_fetch(s, "ss_score_docs", n_q, q_ptr, q_terms, query_len, topic_probs, &qa));
    hw::WindowIn w;                                       // the window's counts; its rows are doc ids, staged below
    w.n_hits = n_in;
    w.n_q = nq;
    w.k_in = (size_t)k_in;
    w.dev_n = ss::on_device(n_in);
    const bool dev_d = ss::on_device(docs);
    if (!w.dev_n) {
        w.h_n.assign(n_in, n_in + nq);
        const size_t bad = hw::first_bad_count(w.h_n.data(), nq, k_in);
        if (bad != hw::NONE) return ctx->fail(SS_ERR_INVALID, "ss_score_docs: n_in[%zu] = %d outside 0 .. k_in = %d", bad, w.h_n[bad], k_in);
    }
    // ---- the queries' table, the blocks of host arrays; then the pipeline
    QueryTurn& turn = s->hyb[s->hyb_turn];
    ScoreDocsParams p{};
    tables_of(s, &p);
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, hits_out, n_rows * sizeof(ss_hit), &o));
    if (!dev_d) SS_HIP(ctx, ensure(s->d_hyb_docs_in, n_rows));
    if (!w.dev_n) SS_HIP(ctx, ensure(s->win.n_in, nq));
    SS_TRY(query_table_up(s, turn, qa, &p));
    s->hyb_turn = (s->hyb_turn + 1) % ss_scorer::TURNS;
    if (!dev_d) {
        SS_HIP(ctx, hipMemcpyAsync(s->d_hyb_docs_in.p, docs, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        docs = s->d_hyb_docs_in.p;
    }
    if (!w.dev_n) {
        SS_HIP(ctx, hipMemcpyAsync(s->win.n_in.p, w.h_n.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
        w.n_hits = s->win.n_in.p;
    }
    w.staged = !dev_d || !w.dev_n;
    SS_HIP(ctx, launch_score_docs(p, docs, w.n_hits, static_cast<ss_hit*>(o.dev), nq, (uint32_t)k_in, st));
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    return hw::entries_out_finish(s, o, w, sizeof(ss_hit));
}

// the hybrid_plan.hpp check with the ABI's codes and the context's error text
int32_t check_fuse(ss_ctx* ctx, const char* entry, const ss_fuse_params* fp, int32_t n_q, const char* lex_name, int32_t k_lex, const char* vec_name,
                   int32_t k_vec, int32_t k, int32_t first) {
    char msg[256];
    const int rc = hy::check_fuse(msg, sizeof(msg), entry, SS_MAX_TOPK, fp != nullptr, fp ? fp->mode : 0, fp ? fp->rrf_c : 0, fp ? fp->w_lex : 0.0,
                                  fp ? fp->w_vec : 0.0, n_q, lex_name, k_lex, vec_name, k_vec, k, first);
    return rc == hy::OK ? SS_OK : ctx->fail(rc == hy::INVALID ? SS_ERR_INVALID : SS_ERR_UNSUPPORTED, "%s", msg);
}

struct FuseArgs {
    int32_t n_q, k_lex, k_vec, first, k;
    const ss_hit* lex;                                    // device memory ...
    const int32_t* n_lex;
    const ss_vec_hit* vec;
    const int32_t* n_vec;
    const int8_t* qvec;                                   // ... all five, qvec 16-byte aligned
    ss_fuse_params fp;
    ss_hit* hits_out;                                     // host or device, the caller's
    int32_t* n_hits_out;
    ss_fused* fused_out;                                  // nullable
    int32_t* n_union_out;                                 // nullable
};

// The four kernels behind lists that are in device memory, and the way back of host outputs.  `last_reader` (nullable) is recorded
// behind the last kernel.  Returns without waiting when every output is device memory and `staged` is false.
int32_t fuse_run(ss_scorer* s, const char* entry, const FuseArgs& a, const QueryArrays& qa, ss::Event* last_reader, bool staged) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)a.n_q, U = (size_t)a.k_lex + (size_t)a.k_vec;
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, nq, (size_t)a.k, a.hits_out, a.n_hits_out, a.n_union_out, a.fused_out, sizeof(ss_fused), &o));
    SS_HIP(ctx, ensure(s->d_hyb_cand, nq * 3 * U));
    SS_HIP(ctx, ensure(s->d_hyb_counts, 3 * nq));
    SS_HIP(ctx, ensure(s->d_hyb_miss_docs, nq * (size_t)a.k_vec));
    SS_HIP(ctx, ensure(s->d_hyb_miss_rows, nq * (size_t)a.k_vec));
    SS_HIP(ctx, ensure(s->d_hyb_miss_vec_rows, nq * (size_t)a.k_lex));
    SS_HIP(ctx, ensure(s->d_hyb_miss_scores, nq * (size_t)a.k_lex));
    QueryTurn& turn = s->hyb[s->hyb_turn];
    ScoreDocsParams sp{};
    tables_of(s, &sp);
    SS_TRY(query_table_up(s, turn, qa, &sp));
    s->hyb_turn = (s->hyb_turn + 1) % ss_scorer::TURNS;
    FuseParams p{};
    p.lex = a.lex; p.n_lex = a.n_lex; p.vec = a.vec; p.n_vec = a.n_vec;
    p.n_docs = s->n_docs;
    p.k_lex = (uint32_t)a.k_lex; p.k_vec = (uint32_t)a.k_vec; p.n_q = (uint32_t)a.n_q;
    p.cand = s->d_hyb_cand.p;
    p.counts = s->d_hyb_counts.p;
    p.miss_docs = s->d_hyb_miss_docs.p;
    p.miss_vec_rows = s->d_hyb_miss_vec_rows.p;
    p.miss_rows = s->d_hyb_miss_rows.p;
    p.miss_scores = s->d_hyb_miss_scores.p;
    p.fp = a.fp;
    p.first = (uint32_t)a.first; p.k = (uint32_t)a.k;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.fused_out = static_cast<ss_fused*>(o.extra);
    p.n_union_out = o.n_kept;
    const bool small = U <= (size_t)FZ_SMALL * FZ_SMALL_PER && a.k <= FZ_SMALL * FZ_SMALL_PER;
    if (small) hipLaunchKernelGGL((k_fuse_hits<FZ_SMALL, FZ_SMALL_PER>), dim3((unsigned)a.n_q), dim3(FZ_SMALL), 0, st, p);
    else hipLaunchKernelGGL((k_fuse_hits<FZ_LARGE, FZ_LARGE_PER>), dim3((unsigned)a.n_q), dim3(FZ_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    // the two gathers: sized by the windows, they leave on the counts k_fuse_hits wrote
    SS_HIP(ctx, launch_score_docs(sp, p.miss_docs, p.counts + nq, s->d_hyb_miss_rows.p, nq, (uint32_t)a.k_vec, st));
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    ss::launch_vec_hit_scores(s, a.qvec, p.miss_vec_rows, p.counts + 2 * nq, a.n_q, a.k_lex, s->d_hyb_miss_scores.p, st);
    SS_HIP(ctx, hipGetLastError());
    if (small) hipLaunchKernelGGL((k_fuse_page<FZ_SMALL, FZ_SMALL_PER>), dim3((unsigned)a.n_q), dim3(FZ_SMALL), 0, st, p);
    else hipLaunchKernelGGL((k_fuse_page<FZ_LARGE, FZ_LARGE_PER>), dim3((unsigned)a.n_q), dim3(FZ_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    if (last_reader) SS_HIP(ctx, last_reader->record(st));
    (void)entry;
    return hw::rows_out_finish(s, o, staged);
}

int32_t fuse_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len, const double* topic_probs,
                  const int8_t* qvec, int32_t k_lex, const ss_hit* lex, const int32_t* n_lex, int32_t k_vec, const ss_vec_hit* vec,
                  const int32_t* n_vec, const ss_fuse_params* fp, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out,
                  ss_fused* fused_out, int32_t* n_union_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(check_fuse(ctx, "ss_fuse_hits", fp, n_q, "k_lex", k_lex, "k_vec", k_vec, k, first));
    if (!q_ptr) return ctx->fail(SS_ERR_INVALID, "ss_fuse_hits: q_ptr is NULL");
    if (n_q > 0 && (!qvec || !vec || !n_vec)) return ctx->fail(SS_ERR_INVALID, "ss_fuse_hits: qvec, vec or n_vec is NULL");
    SS_TRY(hw::check_page_arrays(ctx, "ss_fuse_hits", n_q, k_lex, k, lex, n_lex, hits_out, n_hits_out));
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_fuse_hits: no vector table registered (ss_scorer_set_doc_vectors)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    QueryArrays qa;
    SS_TRY(query_arrays_fetch(s, "ss_fuse_hits", n_q, q_ptr, q_terms, query_len, topic_probs, &qa));
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_fuse_hits", "k_lex", n_q, k_lex, lex, n_lex, &w));
    const bool dev_v = ss::on_device(vec), dev_nv = ss::on_device(n_vec);
    std::vector<int32_t> h_nv;                            // host counts: the snapshot that was checked and is uploaded
    if (!dev_nv) {
        h_nv.assign(n_vec, n_vec + nq);
        const size_t bad = hw::first_bad_count(h_nv.data(), nq, k_vec);
        if (bad != hw::NONE) return ctx->fail(SS_ERR_INVALID, "ss_fuse_hits: n_vec[%zu] = %d outside 0 .. k_vec = %d", bad, h_nv[bad], k_vec);
    }
    // ---- host arrays into the scorer's blocks (the call then waits before it returns)
    SS_TRY(hw::window_stage(s, &w));
    if (!dev_v) {
        SS_HIP(ctx, ensure(s->d_hyb_vec_in, nq * (size_t)k_vec));
        SS_HIP(ctx, hipMemcpyAsync(s->d_hyb_vec_in.p, vec, nq * (size_t)k_vec * sizeof(ss_vec_hit), hipMemcpyHostToDevice, st));
        vec = s->d_hyb_vec_in.p;
    }
    if (!dev_nv) {
        SS_HIP(ctx, ensure(s->d_hyb_nvec_in, nq));
        SS_HIP(ctx, hipMemcpyAsync(s->d_hyb_nvec_in.p, h_nv.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
        n_vec = s->d_hyb_nvec_in.p;
    }
    w.staged = w.staged || !dev_v || !dev_nv;
    const int8_t* d_q = nullptr;
    SS_TRY(ss::vec_queries_to_device(s, qvec, nq * (size_t)s->vec_dim, &d_q, &w.staged));
    const FuseArgs a{n_q, k_lex, k_vec, first, k, w.hits, w.n_hits, vec, n_vec, d_q, *fp, hits_out, n_hits_out, fused_out, n_union_out};
    return fuse_run(s, "ss_fuse_hits", a, qa, nullptr, w.staged);
}

int32_t hybrid_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len, const double* topic_probs,
                    const int8_t* qvec, const int32_t* mask_id, int32_t k_window, const ss_fuse_params* fp, int32_t first, int32_t k,
                    ss_hit* hits_out, int32_t* n_hits_out, ss_fused* fused_out, int32_t* n_union_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks of this call; the two calls below make their own (mask ids, the prior, the queries) before they enqueue anything
    SS_TRY(check_fuse(ctx, "ss_hybrid_topk", fp, n_q, "k_window", k_window, "k_window", k_window, k, first));
    if (!q_ptr || (n_q > 0 && (!qvec || !hits_out || !n_hits_out)))
        return ctx->fail(SS_ERR_INVALID, "ss_hybrid_topk: q_ptr, qvec, hits_out or n_hits_out is NULL");
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_hybrid_topk: no vector table registered (ss_scorer_set_doc_vectors)");
    if (topic_probs && s->k_topics == 0)
        return ctx->fail(SS_ERR_STATE, "ss_hybrid_topk: topic_probs given but no prior set (ss_scorer_set_prior)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    QueryArrays qa;
    SS_TRY(query_arrays_fetch(s, "ss_hybrid_topk", n_q, q_ptr, q_terms, query_len, topic_probs, &qa));
    // ---- the lexical window: the scoring call with k_window, rows in the turn's block
    TurnRows tr;
    if (const int32_t rc = ss::score_into_turn(s, n_q, q_ptr, q_terms, topic_probs, mask_id, k_window, &tr, query_len)) {
        const std::string why = ctx->last_error;          // (the shared steps name ss_score_topk; nothing has touched the outputs)
        return ctx->fail(rc, "ss_hybrid_topk: scoring the queries at k_window failed: %s", why.c_str());
    }
    if (tr.turn < 0) return ctx->fail(SS_ERR_STATE, "ss_hybrid_topk: internal: the scoring call took no turn");
    // ---- the vector window, in a block of the scorer's
    bool staged = false;
    const int8_t* d_q = nullptr;
    SS_TRY(ss::vec_queries_to_device(s, qvec, nq * (size_t)s->vec_dim, &d_q, &staged));
    SS_HIP(ctx, ensure(s->d_hyb_vec_win, nq * (size_t)k_window));
    SS_HIP(ctx, ensure(s->d_hyb_nvec_win, nq));
    if (const int32_t rc = ss_vector_topk(s, n_q, d_q, mask_id, k_window, s->d_hyb_vec_win.p, s->d_hyb_nvec_win.p)) {
        const std::string why = ctx->last_error;
        return ctx->fail(rc, "ss_hybrid_topk: the vector search at k_window failed: %s", why.c_str());
    }
    // k_fuse_page is the last reader of the turn's rows: the turn's batch_ev is recorded again behind it
    const FuseArgs a{n_q, k_window, k_window, first, k, tr.hits, tr.n_hits, s->d_hyb_vec_win.p, s->d_hyb_nvec_win.p, d_q, *fp,
                     hits_out, n_hits_out, fused_out, n_union_out};
    return fuse_run(s, "ss_hybrid_topk", a, qa, &s->turn[tr.turn].batch_ev, staged);
}

}  // namespace

extern "C" {

int32_t ss_score_docs(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                      const double* topic_probs, int32_t k_in, const uint32_t* docs, const int32_t* n_in, ss_hit* hits_out) {
    return hw::guarded(s, "ss_score_docs", [&] { return score_docs_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, k_in, docs, n_in, hits_out); });
}

int32_t ss_fuse_hits(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                     const double* topic_probs, const int8_t* qvec, int32_t k_lex, const ss_hit* lex, const int32_t* n_lex, int32_t k_vec,
                     const ss_vec_hit* vec, const int32_t* n_vec, const ss_fuse_params* fp, int32_t first, int32_t k, ss_hit* hits_out,
                     int32_t* n_hits_out, ss_fused* fused_out, int32_t* n_union_out) {
    return hw::guarded(s, "ss_fuse_hits", [&] {
        return fuse_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, qvec, k_lex, lex, n_lex, k_vec, vec, n_vec, fp, first, k, hits_out,
                         n_hits_out, fused_out, n_union_out);
    });
}

int32_t ss_hybrid_topk(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                       const double* topic_probs, const int8_t* qvec, const int32_t* mask_id, int32_t k_window, const ss_fuse_params* fp,
                       int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, ss_fused* fused_out, int32_t* n_union_out) {
    return hw::guarded(s, "ss_hybrid_topk", [&] {
        return hybrid_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, qvec, mask_id, k_window, fp, first, k, hits_out, n_hits_out,
                           fused_out, n_union_out);
    });
}

}  // extern "C"
