// passage.hip — ss_best_passages: per result row the body window of `width` word positions that covers most of the query's terms
// (DESIGN.md K4j): the anchor of a snippet.  A step file beside explain.hip: one kernel behind whatever made the rows, no scoring
// kernel edited.
//
//   checks                     arguments, q_ptr, host n_hits — all before anything is enqueued
//   the queries' table         ptr [n_q + 1] | tokens | first, through one of the TURNS passage turns (hit_window.hpp:
//                              query_table_fill).  first[i] = the first token index of the query with token i's term: the device
//                              never de-duplicates, a term's SLOT is that index.
//   k_best_passages            one wave (a workgroup of 64) per (query, hit).  Lane i < n_tok owns token i; the lanes with
//                              first == i search the body list of their term for the doc (the plain lower bound of k_explain_hits)
//                              and take the posting's position list.  N = the lists' lengths together.
//     N <= cap ("passage.lds_events")   the wave loads every value as (pos_key << 6) | slot into the LDS (values that are no
//                              occurrence as the all-ones sentinel), sorts them (bitonic, padded to a power of two), and every
//                              lane walks from its candidate starts forward to the window's limit, collecting a slot mask, a
//                              count and the last key.  Equal keys are neighbours: only the first of a run is a start.
//     N > cap                  the same answer from global memory for any N: the wave takes 64 candidate starts at a time, one per
//                              lane, and reads every list once per such batch, 64 values per load, handing them round with shuffles.
//                              Quadratic in N and meant to be: it is the path of the few docs that hold a query's words thousands
//                              of times.
//                              The lanes' best windows (most slots, then most occurrences, then the smallest key) are reduced
//                              with shuffles; the token mask is one ballot over the tokens' slots; lanes 0 .. 5 store one dword each.
// The window in and the way back of a host `out`: hit_window.hpp.
#include "hit_window.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

constexpr int PS_TPB = 64;                                // one wave
constexpr uint32_t PS_NONE = 0xFFFFFFFFu;                 // position key of "no value >= 0" (keys are bits of non-NaN floats >= 0)
constexpr uint64_t PS_PAD = ~0ull;                        // LDS event of a value that is no occurrence, and of the padding
constexpr int64_t PS_CAP_DEFAULT = 512, PS_CAP_MAX = 4096;
constexpr size_t PS_LDS_LISTS = 2 * 64 * sizeof(uint64_t);   // the lists' [begin, end) in front of the events

struct PassageParams {
    const uint64_t* b_ptr;                                // term_ptr of the body table
    const uint32_t* b_doc;
    const uint64_t* b_pos_ptr;                            // NULL: the body table has no positional postings
    const float* b_pos;
    uint64_t b_terms, n_docs;
    const uint32_t *q_ptr, *q_terms, *q_first;            // the call's table: [n_q + 1] offsets | tokens | first index of the token's term
    const ss_hit* hits;                                   // [n_q][k]
    const int32_t* n_hits;                                // [n_q]
    uint32_t* out;                                        // [n_q][k] ss_passage as six dwords each
    uint32_t k, cap;
    double width;
};

// as explain.hip's: the float's bits (ascending with the value for v >= 0), both zeros -> 0; PS_NONE for a negative value or a NaN
__device__ __forceinline__ uint32_t pos_key(float v) {
    return v >= 0.0f ? (v == 0.0f ? 0u : __float_as_uint(v)) : PS_NONE;
}

// a lane's best window so far; n_occ == 0: none
struct Best {
    uint32_t nd, nocc, key, last;
    uint64_t slots;
};
__device__ __forceinline__ bool better(uint32_t nd, uint32_t nocc, uint32_t key, const Best& b) {
    return nd != b.nd ? nd > b.nd : nocc != b.nocc ? nocc > b.nocc : key < b.key;
}

__global__ __launch_bounds__(PS_TPB) void k_best_passages(PassageParams p) {
    extern __shared__ __attribute__((aligned(16))) uint64_t ps_lds[];
    uint64_t* const s_pb = ps_lds;                        // [64] per slot: the position list [pb, pe) (empty for a lane that owns none)
    uint64_t* const s_pe = ps_lds + 64;
    uint64_t* const ev = ps_lds + 128;                    // [pow2 >= cap] events
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
    Best best{0u, 0u, PS_NONE, 0u, 0ull};
    if (n_all <= (uint64_t)p.cap) {
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
                const uint32_t key = pos_key(p.b_pos[ob + x]);
                ev[base + x] = key == PS_NONE ? PS_PAD : ((uint64_t)key << 6) | (uint64_t)o;
            }
        }
        for (uint32_t x = n + lane; x < pw; x += 64) ev[x] = PS_PAD;
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
            if (e == PS_PAD) break;                       // (ascending: nothing but padding from here on)
            const uint32_t key = (uint32_t)(e >> 6);
            if (x > 0 && (uint32_t)(ev[x - 1] >> 6) == key) continue;     // the window of this value starts at the first of the run
            const double limit = (double)__uint_as_float(key) + p.width;
            uint64_t slots = 0;
            uint32_t nocc = 0, last = 0;
            for (uint32_t y = x; y < n; y++) {
                const uint64_t f = ev[y];
                if (f == PS_PAD) break;
                const uint32_t fk = (uint32_t)(f >> 6);
                if (!((double)__uint_as_float(fk) < limit)) break;
                slots |= 1ull << (f & 63u);
                nocc++;
                last = fk;
            }
            const uint32_t nd = (uint32_t)__popcll((unsigned long long)slots);
            if (nocc && better(nd, nocc, key, best)) best = Best{nd, nocc, key, last, slots};
        }
    } else {
        // ---- long path: 64 candidate starts per batch, every list read once per batch (all loops wave-uniform)
        uint64_t cand = owners;
        while (cand) {
            const int o = __ffsll((unsigned long long)cand) - 1;
            cand &= cand - 1;
            const uint64_t ob = s_pb[o], oe = s_pe[o];
            for (uint64_t xb = ob; xb < oe; xb += 64) {
                const uint32_t key = xb + lane < oe ? pos_key(p.b_pos[xb + lane]) : PS_NONE;
                if (!__any(key != PS_NONE)) continue;
                const double limit = (double)__uint_as_float(key == PS_NONE ? 0u : key) + p.width;
                uint64_t slots = 0;
                uint32_t nocc = 0, last = 0;
                uint64_t scan = owners;
                while (scan) {
                    const int o2 = __ffsll((unsigned long long)scan) - 1;
                    scan &= scan - 1;
                    const uint64_t sb = s_pb[o2], se = s_pe[o2];
                    uint32_t hit = 0;
                    for (uint64_t yb = sb; yb < se; yb += 64) {
                        const float mine = yb + lane < se ? p.b_pos[yb + lane] : -1.0f;      // (-1: no occurrence)
                        const int cnt = se - yb < 64 ? (int)(se - yb) : 64;
                        for (int l = 0; l < cnt; l++) {
                            const float v = __shfl(mine, l, 64);
                            const uint32_t vk = pos_key(v);
                            if (vk != PS_NONE && vk >= key && (double)v < limit) {
                                hit++;
                                last = vk > last ? vk : last;
                            }
                        }
                    }
                    if (hit) { slots |= 1ull << o2; nocc += hit; }
                }
                const uint32_t nd = (uint32_t)__popcll((unsigned long long)slots);
                if (key != PS_NONE && nocc && better(nd, nocc, key, best)) best = Best{nd, nocc, key, last, slots};
            }
        }
    }
    // ---- the wave's best window (every lane gets here)
    for (int off = 32; off > 0; off >>= 1) {
        Best o;
        o.nd = __shfl_xor(best.nd, off, 64);
        o.nocc = __shfl_xor(best.nocc, off, 64);
        o.key = __shfl_xor(best.key, off, 64);
        o.last = __shfl_xor(best.last, off, 64);
        o.slots = __shfl_xor(best.slots, off, 64);
        if (better(o.nd, o.nocc, o.key, best)) best = o;  // (equal triples are the same window)
    }
    const uint64_t token_mask = __ballot(lane < n_tok && best.nocc && ((best.slots >> first) & 1ull));
    static_assert(sizeof(ss_passage) == 24, "an entry is six dwords");
    if (lane < 6) {
        const bool any = best.nocc != 0;
        const uint32_t w = lane == 0 ? (any ? best.key : 0u) : lane == 1 ? (any ? best.last : 0u) : lane == 2 ? best.nd : lane == 3 ? best.nocc
                           : lane == 4 ? (uint32_t)token_mask : (uint32_t)(token_mask >> 32);
        p.out[(size_t)blockIdx.x * 6 + lane] = w;         // (a caller's array need only be aligned to 4 bytes)
    }
}

int32_t passages_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                      const int32_t* n_hits, int32_t width, ss_passage* out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and `out` is not touched before the last of them has passed
    if (!out || n_q < 0 || !q_ptr) return ctx->fail(SS_ERR_INVALID, "ss_best_passages: NULL argument or n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_best_passages: k = %d, must be >= 1", k);
    if (width < 1) return ctx->fail(SS_ERR_INVALID, "ss_best_passages: width = %d, must be >= 1", width);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_best_passages: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
    if (width > (1 << 24)) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_best_passages: width = %d exceeds 2^24", width);
    if ((uint64_t)n_q * (uint64_t)k >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_best_passages: n_q * k = %llu entries, must be below 2^31",
                         (unsigned long long)((uint64_t)n_q * (uint64_t)k));
    if (n_q == 0) return SS_OK;
    if (!hits || !n_hits) return ctx->fail(SS_ERR_INVALID, "ss_best_passages: hits or n_hits is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr(nq + 1);
    SS_TRY(fetch_ptr_array(ctx, "ss_best_passages", "q", q_ptr, nq, h_ptr.data()));
    for (size_t q = 0; q < nq; q++)
        if (h_ptr[q + 1] - h_ptr[q] > (uint32_t)SS_MAX_QUERY_TERMS)
            return ctx->fail(SS_ERR_UNSUPPORTED, "ss_best_passages: query %zu has %u tokens, SS_MAX_QUERY_TERMS = %d", q, h_ptr[q + 1] - h_ptr[q],
                             SS_MAX_QUERY_TERMS);
    const size_t tok0 = h_ptr[0], n_tok = h_ptr[nq] - tok0;
    if (n_tok && !q_terms) return ctx->fail(SS_ERR_INVALID, "ss_best_passages: q_terms is NULL");
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_best_passages", "k", n_q, k, hits, n_hits, &w));
    // ---- the queries' table in the pinned block of the next passage turn (ptr | tokens | first), the blocks of host arrays; then the
    // pipeline
    QueryTurn& turn = s->pas[s->pas_turn];
    hw::QueryTable tab;
    SS_TRY(hw::query_table_fill(ctx, turn, h_ptr, q_terms, 2, &tab));
    const uint32_t* const h_tok = tab.h + nq + 1;
    uint32_t* const h_first = tab.h + nq + 1 + n_tok;
    for (size_t q = 0; q < nq; q++)
        for (uint32_t i = tab.h[q]; i < tab.h[q + 1]; i++) {
            uint32_t f = tab.h[q];
            while (h_tok[f] != h_tok[i]) f++;
            h_first[i] = f - tab.h[q];
        }
    const size_t n_rows = nq * (size_t)k;
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, out, n_rows * sizeof(ss_passage), &o));
    SS_TRY(hw::window_stage(s, &w));
    s->pas_turn = (s->pas_turn + 1) % ss_scorer::TURNS;
    SS_HIP(ctx, hw::query_table_upload(ctx, turn, tab));
    PassageParams p{};
    p.b_ptr = s->body->term_ptr.p; p.b_doc = s->body->post_doc.p; p.b_terms = s->body->n_terms;
    p.b_pos_ptr = s->body->pos_ptr.p;
    p.b_pos = s->body->pos.p;
    p.n_docs = s->n_docs;
    p.q_ptr = turn.d_q.p;
    p.q_terms = turn.d_q.p + nq + 1;
    p.q_first = p.q_terms + n_tok;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.out = static_cast<uint32_t*>(o.dev);
    p.k = (uint32_t)k;
    p.cap = (uint32_t)std::min(std::max(ctx->opt("passage.lds_events", PS_CAP_DEFAULT), (int64_t)1), PS_CAP_MAX);
    p.width = (double)width;
    size_t lds_events = 1;
    while (lds_events < p.cap) lds_events <<= 1;
    const size_t lds = PS_LDS_LISTS + lds_events * sizeof(uint64_t);      // <= 33 KiB: below the 64 KiB a launch gets unasked
    hipLaunchKernelGGL(k_best_passages, dim3((unsigned)n_rows), dim3(PS_TPB), lds, st, p);   // (n_rows < 2^31)
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    return hw::entries_out_finish(s, o, w, sizeof(ss_passage));   // every array in device memory: nothing is waited for
}

}  // namespace

extern "C" {

int32_t ss_best_passages(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, int32_t k, const ss_hit* hits,
                         const int32_t* n_hits, int32_t width, ss_passage* out) {
    return hw::guarded(s, "ss_best_passages", [&] { return passages_impl(s, n_q, q_ptr, q_terms, k, hits, n_hits, width, out); });
}

}  // extern "C"
