// proximity.hip — ss_hit_proximity, ss_rerank_hits_by_proximity and ss_score_topk_proximity: per result row the smallest body span that
// holds every query term the doc has at all, and a window re-ranked by it.  A step file beside passage.hip and
// vector.hip: two kernels behind whatever made the rows, no scoring kernel edited.
//
//   checks                     arguments, q_ptr, the weights, host n_hits, the scratch of a re-rank — all before anything is enqueued
//   the queries' table         ptr [n_q + 1] | tokens | first, through one of the TURNS proximity turns, exactly as passage.hip's: a
//                              term's SLOT is the index of its first token.
//   k_hit_proximity            one wave (a workgroup of 64) per (query, hit), the frame of k_best_passages: lane i < n_tok owns token i,
//                              the first lane of a term searches the body list for the doc and takes the posting's position list.
//                              N = the lists' lengths together; P = the slots with a value that is an occurrence (0 <= v < +inf).
//     N <= cap ("proximity.lds_events")   every value goes into the LDS as (pos_key << 6) | slot (no occurrence: the all-ones
//                              sentinel), the events are sorted (bitonic, padded to a power of two), and every lane walks from its
//                              candidate starts (the first event of a run of equal keys) forward until the slots seen equal P: the
//                              span's smallest end for that start.
//     N > cap                  the same answer from global memory for any N: 64 candidate starts at a time, one per lane; per term of
//                              P one pass over its list, 64 values per load handed round with shuffles, for the smallest value >= the
//                              start; the end is the largest of those.  Quadratic in N and meant to be, as k_best_passages' long path.
//                              The lanes' best spans (smallest float64 difference of the VALUES, then the smallest start key) are
//                              reduced with shuffles; the occurrences of the winning span are then counted by all lanes (over the
//                              sorted events, or in one more pass over the lists); the token mask is one ballot; lanes 0 .. 5
//                              store one dword each.
//   k_prox_sort_hits           one workgroup per query, the frame of k_vec_sort_hits: the score of every window row from its entry
//                              (every operation rounded once: the Makefile switches contraction off), then (class, score key, window
//                              index) sorted in the LDS and the page copied out.
// The window in and the way back of host outputs: hit_window.hpp; the re-rank's two per-row outputs come back through a block of its own.
#include "hit_window.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace hw = ss::hitwin;

constexpr int PX_TPB = 64;                                // one wave
constexpr uint32_t PX_NONE = 0xFFFFFFFFu;                 // position key of a value that is no occurrence
constexpr uint32_t PX_INF = 0x7F800000u;                  // the bits of +inf: keys are below it
constexpr uint64_t PX_PAD = ~0ull;                        // LDS event of a value that is no occurrence, and of the padding
constexpr int64_t PX_CAP_DEFAULT = 512, PX_CAP_MAX = 4096;
constexpr size_t PX_LDS_LISTS = 2 * 64 * sizeof(uint64_t);   // the lists' [begin, end) in front of the events
constexpr size_t PX_ENTRY_WORDS = sizeof(ss_proximity) / 4;
static_assert(sizeof(ss_proximity) == 24, "an entry is six dwords");

struct ProxParams {
    const uint64_t* b_ptr;                                // term_ptr of the body table
    const uint32_t* b_doc;
    const uint64_t* b_pos_ptr;                            // NULL: the body table has no positional postings
    const float* b_pos;
    uint64_t b_terms, n_docs;
    const uint32_t *q_ptr, *q_terms, *q_first;            // the call's table: [n_q + 1] offsets | tokens | first index of the token's term
    const ss_hit* hits;                                   // [n_q][k]
    const int32_t* n_hits;                                // [n_q]
    uint32_t* out;                                        // [n_q][k] ss_proximity as six dwords each
    uint32_t k, cap;
};

// the float's bits (ascending with the value for v >= 0), both zeros -> 0; PX_NONE for a negative value, a NaN or +inf
__device__ __forceinline__ uint32_t px_key(float v) {
    return v >= 0.0f && v < __uint_as_float(PX_INF) ? (v == 0.0f ? 0u : __float_as_uint(v)) : PX_NONE;
}
__device__ __forceinline__ double px_diff(uint32_t a, uint32_t b) { return (double)__uint_as_float(b) - (double)__uint_as_float(a); }

// a lane's best span so far; ok == 0: none
struct Span {
    double diff;
    uint32_t key, last, ok;
};
__device__ __forceinline__ bool px_better(double diff, uint32_t key, const Span& b) {
    return !b.ok || (diff != b.diff ? diff < b.diff : key < b.key);
}

__global__ __launch_bounds__(PX_TPB) void k_hit_proximity(ProxParams p) {
    extern __shared__ __attribute__((aligned(16))) uint64_t px_lds[];
    uint64_t* const s_pb = px_lds;                        // [64] per slot: the position list [pb, pe) (empty for a lane that owns none)
    uint64_t* const s_pe = px_lds + 64;
    uint64_t* const ev = px_lds + 128;                    // [pow2 >= cap] events
    const uint32_t q = blockIdx.x / p.k, j = blockIdx.x - q * p.k;
    if (j >= hw::window_len(p.n_hits[q], p.k)) return;    // (the whole wave)
    const uint32_t lane = threadIdx.x;
    const uint32_t q0 = p.q_ptr[q];
    uint32_t n_tok = p.q_ptr[q + 1] - q0;
    n_tok = n_tok > 64u ? 64u : n_tok;                    // (the host has refused longer queries; the table is the call's own)
    const uint32_t d = p.hits[(size_t)blockIdx.x].doc;
    // ---- the lists: lane i < n_tok owns token i, the first lane of a term searches
    uint32_t first = lane;
    uint64_t pb = 0, pe = 0;
    if (lane < n_tok) {
        first = p.q_first[q0 + lane];
        const uint32_t term = p.q_terms[q0 + lane];
        if (first == lane && p.b_pos_ptr && (uint64_t)d < p.n_docs && (uint64_t)term < p.b_terms) {
            uint64_t lo = p.b_ptr[term], hi = p.b_ptr[term + 1];
            const uint64_t end = hi;
            while (lo < hi) {
                const uint64_t m = lo + ((hi - lo) >> 1);
                if (p.b_doc[m] < d) lo = m + 1; else hi = m;
            }
            if (lo < end && p.b_doc[lo] == d) {
                pb = p.b_pos_ptr[lo];
                pe = p.b_pos_ptr[lo + 1];
            }
        }
    }
    s_pb[lane] = pb;
    s_pe[lane] = pe;
    const uint64_t len = pe - pb;
    uint64_t incl = len;                                  // inclusive prefix of the lengths over the lanes
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += up;
    }
    const uint64_t n_all = __shfl(incl, 63, 64);
    const uint64_t owners = __ballot(len != 0);
    __syncthreads();                                      // (one wave: orders the LDS writes above before the reads below)
    const bool in_lds = n_all <= (uint64_t)p.cap;         // (the same in every lane)
    Span best{0.0, PX_NONE, 0u, 0u};
    uint64_t pmask = 0;                                   // P as a mask of slots; per lane until the reduction below
    if (in_lds) {
        // ---- LDS path: load, pad, sort, walk
        const uint32_t n = (uint32_t)n_all;
        uint32_t pw = 1;
        while (pw < n) pw <<= 1;                          // (<= the power of two the launch sized the LDS for)
        uint64_t todo = owners;
        while (todo) {
            const int o = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t ob = s_pb[o], on = s_pe[o] - ob;
            const uint32_t base = (uint32_t)(__shfl(incl, o, 64) - on);
            for (uint32_t x = lane; x < (uint32_t)on; x += 64) {
                const uint32_t key = px_key(p.b_pos[ob + x]);
                ev[base + x] = key == PX_NONE ? PX_PAD : ((uint64_t)key << 6) | (uint64_t)o;
                if (key != PX_NONE) pmask |= 1ull << o;
            }
        }
        for (uint32_t x = n + lane; x < pw; x += 64) ev[x] = PX_PAD;
        for (int off = 32; off > 0; off >>= 1) pmask |= __shfl_xor(pmask, off, 64);
        __syncthreads();
        for (uint32_t kk = 2; kk <= pw; kk <<= 1)
            for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                for (uint32_t x = lane; x < pw; x += 64) {
                    const uint32_t y = x ^ jj;
                    if (y > x) {
                        const uint64_t a = ev[x], b = ev[y];
                        if ((a > b) == ((x & kk) == 0)) { ev[x] = b; ev[y] = a; }
                    }
                }
                __syncthreads();
            }
        for (uint32_t x = lane; x < n; x += 64) {
            const uint64_t e = ev[x];
            if (e == PX_PAD) break;                       // (ascending: nothing but padding from here on)
            const uint32_t key = (uint32_t)(e >> 6);
            if (x > 0 && (uint32_t)(ev[x - 1] >> 6) == key) continue;     // the span of this value starts at the first of the run
            uint64_t slots = 0;
            uint32_t last = 0;
            bool covered = false;
            for (uint32_t y = x; y < n && !covered; y++) {
                const uint64_t f = ev[y];
                if (f == PX_PAD) break;
                slots |= 1ull << (f & 63u);
                covered = slots == pmask;
                last = (uint32_t)(f >> 6);
            }
            if (!covered) break;                          // (no later start of this lane covers P either)
            const double diff = px_diff(key, last);
            if (px_better(diff, key, best)) best = Span{diff, key, last, 1u};
        }
    } else {
        // ---- long path (all loops wave-uniform).  P first: one pass over every list
        uint64_t todo = owners;
        while (todo) {
            const int o = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t ob = s_pb[o], oe = s_pe[o];
            bool any = false;
            for (uint64_t xb = ob + lane; xb < oe; xb += 64) any |= px_key(p.b_pos[xb]) != PX_NONE;
            if (__any(any)) pmask |= 1ull << o;
        }
        // 64 candidate starts per batch, one per lane; per term of P the smallest value >= the start
        uint64_t cand = pmask;
        while (cand) {
            const int o = __ffsll((unsigned long long)cand) - 1;
            cand &= cand - 1;
            const uint64_t ob = s_pb[o], oe = s_pe[o];
            for (uint64_t xb = ob; xb < oe; xb += 64) {
                const uint32_t key = xb + lane < oe ? px_key(p.b_pos[xb + lane]) : PX_NONE;
                if (!__any(key != PX_NONE)) continue;
                uint32_t last = 0;
                bool covered = true;
                uint64_t scan = pmask;
                while (scan) {
                    const int o2 = __ffsll((unsigned long long)scan) - 1;
                    scan &= scan - 1;
                    const uint64_t sb = s_pb[o2], se = s_pe[o2];
                    uint32_t least = PX_NONE;
                    for (uint64_t yb = sb; yb < se; yb += 64) {
                        const float mine = yb + lane < se ? p.b_pos[yb + lane] : -1.0f;      // (-1: no occurrence)
                        const int cnt = se - yb < 64 ? (int)(se - yb) : 64;
                        for (int l = 0; l < cnt; l++) {
                            const uint32_t vk = px_key(__shfl(mine, l, 64));
                            if (vk != PX_NONE && vk >= key && vk < least) least = vk;
                        }
                    }
                    if (least == PX_NONE) covered = false;
                    else last = least > last ? least : last;
                }
                if (key != PX_NONE && covered) {
                    const double diff = px_diff(key, last);
                    if (px_better(diff, key, best)) best = Span{diff, key, last, 1u};
                }
            }
        }
    }
    // ---- the wave's best span (every lane gets here)
    for (int off = 32; off > 0; off >>= 1) {
        Span o;
        o.diff = __shfl_xor(best.diff, off, 64);
        o.key = __shfl_xor(best.key, off, 64);
        o.last = __shfl_xor(best.last, off, 64);
        o.ok = __shfl_xor(best.ok, off, 64);
        if (o.ok && px_better(o.diff, o.key, best)) best = o;                     // (equal pairs are the same span)
    }
    // ---- the occurrences of the span, a lane its share: of the sorted events, or in one more pass over every list
    uint32_t nocc = 0;
    if (in_lds) {
        for (uint32_t x = lane; x < (uint32_t)n_all; x += 64) {
            const uint64_t e = ev[x];
            const uint32_t vk = (uint32_t)(e >> 6);
            nocc += best.ok && e != PX_PAD && vk >= best.key && vk <= best.last ? 1u : 0u;
        }
    } else {
        uint64_t todo = best.ok ? pmask : 0ull;
        while (todo) {
            const int o = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t ob = s_pb[o], oe = s_pe[o];
            for (uint64_t xb = ob + lane; xb < oe; xb += 64) {
                const uint32_t vk = px_key(p.b_pos[xb]);
                nocc += vk != PX_NONE && vk >= best.key && vk <= best.last ? 1u : 0u;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) nocc += __shfl_xor(nocc, off, 64);
    const uint64_t token_mask = __ballot(lane < n_tok && best.ok && ((pmask >> first) & 1ull));
    if (lane < 6) {
        const bool any = best.ok != 0;
        const uint32_t w = lane == 0 ? (any ? best.key : 0u) : lane == 1 ? (any ? best.last : 0u)
                           : lane == 2 ? (any ? (uint32_t)__popcll((unsigned long long)pmask) : 0u) : lane == 3 ? (any ? nocc : 0u)
                           : lane == 4 ? (uint32_t)token_mask : (uint32_t)(token_mask >> 32);
        p.out[(size_t)blockIdx.x * PX_ENTRY_WORDS + lane] = w;                    // (a caller's array need only be aligned to 4 bytes)
    }
}

// ---- a window sorted by its proximity scores ------------------------------------------------------------------------------------
constexpr uint32_t PS_CLASS_SHIFT = 16;                   // tag = class << 16 | window index (< SS_MAX_TOPK = 2^10)
constexpr uint32_t PS_NAN = 1, PS_OUTSIDE = 2, PS_DEAD = 3;
constexpr uint64_t PS_NAN_BITS = 0x7FF8000000000000ull;

struct ProxSortParams {
    const uint32_t* entries;                              // [n_q][k_in] six dwords each, from k_hit_proximity
    const uint32_t *q_ptr, *q_first;                      // the call's table
    uint64_t n_docs;
    const ss_hit* hits;
    const int32_t* n_hits;
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;
    uint64_t* scores_out;                                 // [n_q][k] the bits of a double, nullable
    uint32_t* prox_out;                                   // [n_q][k] six dwords each, nullable
    double w_rank, w_prox;
    uint32_t k_in, first, k;
};

// (class, key, window index) of a behind that of b; the key: the score's bits turned so that the larger score has the smaller key
__device__ __forceinline__ bool ps_after(uint64_t ka, uint32_t ta, uint64_t kb, uint32_t tb) {
    const uint32_t ca = ta >> PS_CLASS_SHIFT, cb = tb >> PS_CLASS_SHIFT;
    return ca != cb ? ca > cb : ka != kb ? ka > kb : ta > tb;
}

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_prox_sort_hits(ProxSortParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    __shared__ uint64_t s_key[CAP];
    __shared__ uint64_t s_score[CAP];                     // by window index: the bits that scores_out gets
    __shared__ uint32_t s_tag[CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t* const ent = p.entries + (size_t)q * p.k_in * PX_ENTRY_WORDS;
    const uint32_t np = hw::pow2_at_least(n);
    // T: the distinct term ids of the query's tokens = the tokens that are the first of their term (the same in every thread)
    const uint32_t q0 = p.q_ptr[q];
    uint32_t n_tok = p.q_ptr[q + 1] - q0;
    n_tok = n_tok > 64u ? 64u : n_tok;
    uint32_t n_terms = 0;
    for (uint32_t i = 0; i < n_tok; i++) n_terms += p.q_first[q0 + i] == i ? 1u : 0u;
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint64_t key = 0;
        uint32_t tag = PS_DEAD << PS_CLASS_SHIFT | j;
        if (j < n) {
            uint64_t bits = PS_NAN_BITS;
            tag = PS_OUTSIDE << PS_CLASS_SHIFT | j;
            if ((uint64_t)rows[j].doc < p.n_docs) {
                const uint32_t* const e = ent + (size_t)j * PX_ENTRY_WORDS;
                const uint32_t n_present = e[2];
                const double sp = (double)__uint_as_float(e[1]) - (double)__uint_as_float(e[0]);
                const double gaps = (double)(n_present - 1u);
                const double prox = n_present < 2u ? 0.0 : gaps / (sp > gaps ? sp : gaps);
                const double cover = n_terms ? (double)n_present / (double)n_terms : 0.0;
                const double bonus = prox * cover;
                const double a = p.w_rank * rows[j].final, b = p.w_prox * bonus;
                const double score = a + b;
                if (score != score) {
                    tag = PS_NAN << PS_CLASS_SHIFT | j;
                } else {
                    bits = (uint64_t)__double_as_longlong(score);
                    const uint64_t ob = score == 0.0 ? 0ull : bits;               // -0.0 ties 0.0
                    const uint64_t asc = ob >> 63 ? ~ob : ob | (1ull << 63);      // ascending with the value
                    key = ~asc;
                    tag = j;
                }
            }
            s_score[j] = bits;
        }
        s_key[j] = key;
        s_tag[j] = tag;
    }
    __syncthreads();
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t ka = s_key[i], kb = s_key[o];
        const uint32_t ta = s_tag[i], tb = s_tag[o];
        if (ps_after(ka, ta, kb, tb) == up) {
            s_key[i] = kb; s_tag[i] = tb;
            s_key[o] = ka; s_tag[o] = ta;
        }
    });
    // ---- the page: sorted positions [first, first + n_out), all below n
    const uint32_t n_out = hw::page_len(n, p.first, p.k);
    constexpr uint32_t J_MASK = (1u << PS_CLASS_SHIFT) - 1u;
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_tag[p.first + r] & J_MASK; });
    if (p.scores_out)
        for (uint32_t r = tid; r < n_out; r += BLOCK) p.scores_out[(size_t)q * p.k + r] = s_score[s_tag[p.first + r] & J_MASK];
    if (p.prox_out)
        for (uint32_t x = tid; x < n_out * PX_ENTRY_WORDS; x += BLOCK) {
            const uint32_t r = x / PX_ENTRY_WORDS, w = x - r * PX_ENTRY_WORDS;
            p.prox_out[((size_t)q * p.k) * PX_ENTRY_WORDS + x] = ent[(size_t)(s_tag[p.first + r] & J_MASK) * PX_ENTRY_WORDS + w];
        }
    if (tid == 0) p.n_hits_out[q] = (int32_t)n_out;
}

constexpr int PS_SMALL = 64, PS_SMALL_PER = 2, PS_LARGE = 256, PS_LARGE_PER = 4;
static_assert(PS_LARGE * PS_LARGE_PER >= SS_MAX_TOPK, "k_prox_sort_hits holds a whole window in LDS");

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The checks of the query arrays, those of ss_best_passages: q_ptr to h_ptr (n_q + 1 offsets).  Enqueues nothing.
int32_t check_queries(ss_ctx* ctx, const char* entry, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, std::vector<uint32_t>* h_ptr) {
    const size_t nq = (size_t)n_q;
    h_ptr->assign(nq + 1, 0u);
    SS_TRY(fetch_ptr_array(ctx, entry, "q", q_ptr, nq, h_ptr->data()));
    for (size_t q = 0; q < nq; q++)
        if ((*h_ptr)[q + 1] - (*h_ptr)[q] > (uint32_t)SS_MAX_QUERY_TERMS)
            return ctx->fail(SS_ERR_UNSUPPORTED, "%s: query %zu has %u tokens, SS_MAX_QUERY_TERMS = %d", entry, q, (*h_ptr)[q + 1] - (*h_ptr)[q],
                             SS_MAX_QUERY_TERMS);
    if ((*h_ptr)[nq] - (*h_ptr)[0] && !q_terms) return ctx->fail(SS_ERR_INVALID, "%s: q_terms is NULL", entry);
    return SS_OK;
}

// a grow-only block that a refusal may still follow: no device memory is SS_ERR_OOM, and nothing has been enqueued
template <typename T>
int32_t ensure_or_oom(ss_ctx* ctx, const char* entry, ss::DevBuf<T>& b, size_t n) {
    const hipError_t e = ensure(b, n);
    if (e == hipSuccess) return SS_OK;
    (void)hipGetLastError();
    return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %zu bytes of scratch", entry, n * sizeof(T));
}

// The queries' table of a call in the pinned block of the next proximity turn (ptr | tokens | first).  Waits for the turn's last
// reader; enqueues nothing.
int32_t table_fill(ss_scorer* s, const std::vector<uint32_t>& h_ptr, const uint32_t* q_terms, QueryTurn** turn, hw::QueryTable* tab) {
    *turn = &s->prx[s->prx_turn];
    SS_TRY(hw::query_table_fill(s->ctx, **turn, h_ptr, q_terms, 2, tab));
    const size_t nq = tab->n_q;
    const uint32_t* const h_tok = tab->h + nq + 1;
    uint32_t* const h_first = tab->h + nq + 1 + tab->n_tok;
    for (size_t q = 0; q < nq; q++)
        for (uint32_t i = tab->h[q]; i < tab->h[q + 1]; i++) {
            uint32_t f = tab->h[q];
            while (h_tok[f] != h_tok[i]) f++;
            h_first[i] = f - tab->h[q];
        }
    return SS_OK;
}

// The table up and k_hit_proximity over rows and counts in device memory.  The caller records turn.ev behind the table's last reader.
int32_t enqueue_entries(ss_scorer* s, QueryTurn& turn, const hw::QueryTable& tab, int32_t k, const ss_hit* d_hits, const int32_t* d_n_hits,
                        uint32_t* d_out, ProxParams* p_out) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    s->prx_turn = (s->prx_turn + 1) % ss_scorer::TURNS;
    SS_HIP(ctx, hw::query_table_upload(ctx, turn, tab));
    ProxParams p{};
    p.b_ptr = s->body->term_ptr.p; p.b_doc = s->body->post_doc.p; p.b_terms = s->body->n_terms;
    p.b_pos_ptr = s->body->pos_ptr.p;
    p.b_pos = s->body->pos.p;
    p.n_docs = s->n_docs;
    p.q_ptr = turn.d_q.p;
    p.q_terms = turn.d_q.p + tab.n_q + 1;
    p.q_first = p.q_terms + tab.n_tok;
    p.hits = d_hits;
    p.n_hits = d_n_hits;
    p.out = d_out;
    p.k = (uint32_t)k;
    p.cap = (uint32_t)std::min(std::max(ctx->opt("proximity.lds_events", PX_CAP_DEFAULT), (int64_t)1), PX_CAP_MAX);
    size_t lds_events = 1;
    while (lds_events < p.cap) lds_events <<= 1;
    const size_t lds = PX_LDS_LISTS + lds_events * sizeof(uint64_t);      // <= 33 KiB: below the 64 KiB a launch gets unasked
    hipLaunchKernelGGL(k_hit_proximity, dim3((unsigned)(tab.n_q * (size_t)k)), dim3(PX_TPB), lds, st, p);   // (n_rows < 2^31)
    SS_HIP(ctx, hipGetLastError());
    *p_out = p;
    return SS_OK;
}

int32_t proximity_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                       const int32_t* n_hits, ss_proximity* out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and `out` is not touched before the last of them has passed
    if (!out || n_q < 0 || !q_ptr) return ctx->fail(SS_ERR_INVALID, "ss_hit_proximity: NULL argument or n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_hit_proximity: k = %d, must be >= 1", k);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_hit_proximity: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
    if ((uint64_t)n_q * (uint64_t)k >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_hit_proximity: n_q * k = %llu entries, must be below 2^31",
                         (unsigned long long)((uint64_t)n_q * (uint64_t)k));
    if (n_q == 0) return SS_OK;
    if (!hits || !n_hits) return ctx->fail(SS_ERR_INVALID, "ss_hit_proximity: hits or n_hits is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> h_ptr;
    SS_TRY(check_queries(ctx, "ss_hit_proximity", n_q, q_ptr, q_terms, &h_ptr));
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_hit_proximity", "k", n_q, k, hits, n_hits, &w));
    // ---- the table, the blocks of host arrays; then the pipeline
    QueryTurn* turn = nullptr;
    hw::QueryTable tab;
    SS_TRY(table_fill(s, h_ptr, q_terms, &turn, &tab));
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, out, (size_t)n_q * (size_t)k * sizeof(ss_proximity), &o));
    SS_TRY(hw::window_stage(s, &w));
    ProxParams p;
    SS_TRY(enqueue_entries(s, *turn, tab, k, w.hits, w.n_hits, static_cast<uint32_t*>(o.dev), &p));
    SS_HIP(ctx, turn->ev.record(ctx->stream));            // the turn's pinned block and its device copy are read until here
    return hw::entries_out_finish(s, o, w, sizeof(ss_proximity));   // every array in device memory: nothing is waited for
}

struct RerankArgs {
    int32_t n_q, k_in, first, k;
    double w_rank, w_prox;
    const ss_hit* hits;                                   // device memory ...
    const int32_t* n_hits;                                // ... both
    ss_hit* hits_out;                                     // host or device, the caller's
    int32_t* n_hits_out;
    double* scores_out;                                   // nullable
    ss_proximity* prox_out;                               // nullable
};

// The scratch of a re-rank, had before anything is enqueued: the window's entries, and the device block of host scores_out / prox_out.
int32_t rerank_scratch(ss_scorer* s, const char* entry, int32_t n_q, int32_t k_in, int32_t k, const double* scores_out, const ss_proximity* prox_out) {
    SS_TRY(ensure_or_oom(s->ctx, entry, s->d_prx_entries, (size_t)n_q * (size_t)k_in * PX_ENTRY_WORDS));
    const bool host_sc = scores_out && !ss::on_device(scores_out), host_px = prox_out && !ss::on_device(prox_out);
    if (host_sc || host_px) SS_TRY(ensure_or_oom(s->ctx, entry, s->d_prx_out, (size_t)n_q * (size_t)k * (sizeof(double) + sizeof(ss_proximity))));
    return SS_OK;
}

// Both kernels behind rows that are in device memory, and the way back of host outputs.  `last_reader` (nullable) is recorded behind
// the kernels.  Returns without waiting when every output is device memory and `staged` is false.
int32_t rerank_run(ss_scorer* s, const RerankArgs& a, QueryTurn& turn, const hw::QueryTable& tab, ss::Event* last_reader, bool staged) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t n_out_rows = (size_t)a.n_q * (size_t)a.k;
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)a.n_q, (size_t)a.k, a.hits_out, a.n_hits_out, nullptr, nullptr, 0, &o));
    // the two per-row outputs: the caller's arrays when they are device memory, else the halves of the call's own block
    const bool host_sc = a.scores_out && !ss::on_device(a.scores_out), host_px = a.prox_out && !ss::on_device(a.prox_out);
    uint64_t* d_sc = reinterpret_cast<uint64_t*>(a.scores_out);
    uint32_t* d_px = reinterpret_cast<uint32_t*>(a.prox_out);
    if (host_sc) d_sc = reinterpret_cast<uint64_t*>(s->d_prx_out.p);
    if (host_px) d_px = reinterpret_cast<uint32_t*>(s->d_prx_out.p + n_out_rows * sizeof(double));
    ProxParams pp;
    SS_TRY(enqueue_entries(s, turn, tab, a.k_in, a.hits, a.n_hits, s->d_prx_entries.p, &pp));
    ProxSortParams p{};
    p.entries = s->d_prx_entries.p;
    p.q_ptr = pp.q_ptr;
    p.q_first = pp.q_first;
    p.n_docs = s->n_docs;
    p.hits = a.hits;
    p.n_hits = a.n_hits;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.scores_out = d_sc;
    p.prox_out = d_px;
    p.w_rank = a.w_rank; p.w_prox = a.w_prox;
    p.k_in = (uint32_t)a.k_in; p.first = (uint32_t)a.first; p.k = (uint32_t)a.k;
    if (a.k_in <= PS_SMALL * PS_SMALL_PER)
        hipLaunchKernelGGL((k_prox_sort_hits<PS_SMALL, PS_SMALL_PER>), dim3((unsigned)a.n_q), dim3(PS_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_prox_sort_hits<PS_LARGE, PS_LARGE_PER>), dim3((unsigned)a.n_q), dim3(PS_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    if (last_reader) SS_HIP(ctx, last_reader->record(st));
    if (!host_sc && !host_px) return hw::rows_out_finish(s, o, staged);
    // ---- host scores_out / prox_out: the counts with them, then exactly the entries the kernel wrote (rows_out_finish waits)
    std::vector<int32_t> h_n((size_t)a.n_q);
    std::vector<unsigned char> h_sc(host_sc ? n_out_rows * sizeof(double) : 0), h_px(host_px ? n_out_rows * sizeof(ss_proximity) : 0);
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), o.n_hits, h_n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_sc) SS_HIP(ctx, hipMemcpyAsync(h_sc.data(), d_sc, h_sc.size(), hipMemcpyDeviceToHost, st));
    if (host_px) SS_HIP(ctx, hipMemcpyAsync(h_px.data(), d_px, h_px.size(), hipMemcpyDeviceToHost, st));
    SS_TRY(hw::rows_out_finish(s, o, true));
    if (host_sc) hw::copy_written(a.scores_out, h_sc.data(), (size_t)a.n_q, (size_t)a.k, sizeof(double), h_n.data());
    if (host_px) hw::copy_written(a.prox_out, h_px.data(), (size_t)a.n_q, (size_t)a.k, sizeof(ss_proximity), h_n.data());
    return SS_OK;
}

int32_t check_weights(ss_ctx* ctx, const char* entry, double w_rank, double w_prox) {
    if (!std::isfinite(w_rank) || !std::isfinite(w_prox)) return ctx->fail(SS_ERR_INVALID, "%s: w_rank = %g or w_prox = %g is not finite", entry, w_rank, w_prox);
    return SS_OK;
}

int32_t rerank_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k_in, const ss_hit* hits,
                    const int32_t* n_hits, double w_rank, double w_prox, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out,
                    double* scores_out, ss_proximity* prox_out) {
    const char* const entry = "ss_rerank_hits_by_proximity";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, entry, "k_in", n_q, k_in, k, first));
    if (!q_ptr) return ctx->fail(SS_ERR_INVALID, "%s: q_ptr is NULL", entry);
    SS_TRY(hw::check_page_arrays(ctx, entry, n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    SS_TRY(check_weights(ctx, entry, w_rank, w_prox));
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> h_ptr;
    SS_TRY(check_queries(ctx, entry, n_q, q_ptr, q_terms, &h_ptr));
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, entry, "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(rerank_scratch(s, entry, n_q, k_in, k, scores_out, prox_out));
    QueryTurn* turn = nullptr;
    hw::QueryTable tab;
    SS_TRY(table_fill(s, h_ptr, q_terms, &turn, &tab));
    SS_TRY(hw::window_stage(s, &w));
    const RerankArgs a{n_q, k_in, first, k, w_rank, w_prox, w.hits, w.n_hits, hits_out, n_hits_out, scores_out, prox_out};
    return rerank_run(s, a, *turn, tab, nullptr, w.staged);
}

int32_t score_proximity_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                             const double* topic_probs, const int32_t* mask_id, int32_t k_window, double w_rank, double w_prox, int32_t first,
                             int32_t k, ss_hit* hits_out, int32_t* n_hits_out, double* scores_out, ss_proximity* prox_out) {
    const char* const entry = "ss_score_topk_proximity";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks of this call; the scoring call below makes its own (mask ids, the prior, the queries) before it enqueues anything
    SS_TRY(hw::check_paging(ctx, entry, "k_window", n_q, k_window, k, first));
    if (!q_ptr || (n_q > 0 && (!hits_out || !n_hits_out))) return ctx->fail(SS_ERR_INVALID, "%s: q_ptr, hits_out or n_hits_out is NULL", entry);
    SS_TRY(check_weights(ctx, entry, w_rank, w_prox));
    if (topic_probs && s->k_topics == 0) return ctx->fail(SS_ERR_STATE, "%s: topic_probs given but no prior set (ss_scorer_set_prior)", entry);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> h_ptr;
    SS_TRY(check_queries(ctx, entry, n_q, q_ptr, q_terms, &h_ptr));
    SS_TRY(rerank_scratch(s, entry, n_q, k_window, k, scores_out, prox_out));
    // ---- the scoring call with k_window, rows in the turn's block
    TurnRows tr;
    if (const int32_t rc = ss::score_into_turn(s, n_q, q_ptr, q_terms, topic_probs, mask_id, k_window, &tr, query_len)) {
        const std::string why = ctx->last_error;          // (the shared steps name ss_score_topk; nothing has touched the outputs)
        return ctx->fail(rc, "%s: scoring the queries at k_window failed: %s", entry, why.c_str());
    }
    if (tr.turn < 0) return ctx->fail(SS_ERR_STATE, "%s: internal: the scoring call took no turn", entry);
    QueryTurn* turn = nullptr;
    hw::QueryTable tab;
    SS_TRY(table_fill(s, h_ptr, q_terms, &turn, &tab));
    // k_prox_sort_hits is the last reader of the turn's rows: the turn's batch_ev is recorded again behind it
    const RerankArgs a{n_q, k_window, first, k, w_rank, w_prox, tr.hits, tr.n_hits, hits_out, n_hits_out, scores_out, prox_out};
    return rerank_run(s, a, *turn, tab, &s->turn[tr.turn].batch_ev, false);
}

}  // namespace

extern "C" {

int32_t ss_hit_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                         const int32_t* n_hits, ss_proximity* out) {
    return hw::guarded(s, "ss_hit_proximity", [&] { return proximity_impl(s, n_q, q_ptr, q_terms, k, hits, n_hits, out); });
}

int32_t ss_rerank_hits_by_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k_in, const ss_hit* hits,
                                    const int32_t* n_hits, double w_rank, double w_prox, int32_t first, int32_t k, ss_hit* hits_out,
                                    int32_t* n_hits_out, double* scores_out, ss_proximity* prox_out) {
    return hw::guarded(s, "ss_rerank_hits_by_proximity", [&] {
        return rerank_impl(s, n_q, q_ptr, q_terms, k_in, hits, n_hits, w_rank, w_prox, first, k, hits_out, n_hits_out, scores_out, prox_out);
    });
}

int32_t ss_score_topk_proximity(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* query_len,
                                const double* topic_probs, const int32_t* mask_id, int32_t k_window, double w_rank, double w_prox,
                                int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, double* scores_out, ss_proximity* prox_out) {
    return hw::guarded(s, "ss_score_topk_proximity", [&] {
        return score_proximity_impl(s, n_q, q_ptr, q_terms, query_len, topic_probs, mask_id, k_window, w_rank, w_prox, first, k, hits_out,
                                    n_hits_out, scores_out, prox_out);
    });
}

}  // extern "C"
