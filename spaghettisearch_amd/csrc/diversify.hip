// diversify.hip — ss_diversify_hits: a result window re-ranked greedily by relevance minus similarity to the rows already chosen
// (maximal marginal relevance over the doc vectors of ss_scorer_set_doc_vectors).
//
//   k_div_gram          grid (tile pair, query of the group), one wave.  The wave owns the 64 x 64 tile (ti, tj), tj >= ti, of the
//                       window's Gram matrix sim(i, j): 4 x 4 accumulators of __builtin_amdgcn_mfma_i32_16x16x64_i8.  BOTH operands are
//                       doc rows gathered from the table by hits[..].doc, 16 bytes per lane, by the operand rule k_vec_topk documents
//                       (vector.hip): lane l holds bytes 16 (l >> 4) .. + 15 of the 64-byte k step of row l & 15, so byte t of one doc
//                       meets byte t of the other whatever order the instruction gives the 64 k positions of a step.  The C/D map is
//                       the one vector.hip states (column = l & 15, row = 4 (l >> 4) + register): register g of accumulator (ta, tb)
//                       is sim(i0 + 16 ta + 4 (l >> 4) + g, j0 + 16 tb + (l & 15)).  sim is symmetric and exact, so a tile off the
//                       diagonal is written twice, as it stands and transposed (16 bytes per lane).  A tile wholly past the window's
//                       length exits at once; a row past it, or an outside row (doc >= n_docs), gathers a clamped in-table row and its
//                       entries are never read.  Output: int32 [queries of the group][pitch][pitch].
//   k_div_select        one workgroup per query, a window row per thread and slot (at most 4 slots at 256 threads): relevance, running
//                       penalty and the chosen flag live in registers.  min(n_inside, first + k) steps; a step is one block arg-max over
//                       the keys diversify_plan.hpp defines ((value + 2^42) << 10 | (1023 - j): the largest value, then the smallest
//                       j) and one read of the chosen row of the Gram matrix, which raises the penalties.  The page, the info and the
//                       count are written with hit_window.hpp's copy_page / page_len.
// rel comes from k_vec_hit_scores, enqueued as ss_hit_vector_scores enqueues it, or is the window position.  No float anywhere.  The
// window in, the paging checks and the outputs' way back are hit_window.hpp's; with device arrays throughout the call only enqueues.
#include "diversify_plan.hpp"
#include "hit_window.hpp"

namespace {

namespace hw = ss::hitwin;
namespace dp = ss::divp;

typedef int v4i __attribute__((ext_vector_type(4)));
static_assert(SS_DIV_WEIGHT_MAX == dp::WEIGHT_MAX && SS_MAX_TOPK == dp::MAX_WINDOW, "diversify_plan.hpp states the ABI's limits");
static_assert(sizeof(ss_div_info) == 8, "an info entry is one 8-byte word");

struct DivGramParams {
    const int8_t* vec;                 // [n_docs][dim], n_docs > 0
    uint64_t n_docs;
    const ss_hit* hits;                // [n_q][k_in]
    const int32_t* n_hits;             // [n_q]
    int32_t* gram;                     // [queries of the group][pitch][pitch]
    uint32_t dim, k_in, pitch, n_tiles, q0;
};

__global__ __launch_bounds__(64) void k_div_gram(DivGramParams p) {
    const uint32_t lane = threadIdx.x, r = lane & 15u, h = lane >> 4;
    const uint32_t local = blockIdx.y, q = p.q0 + local;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);
    const dp::TilePair tp = dp::tile_of_pair(blockIdx.x, p.n_tiles);
    const uint32_t i0 = tp.ti * dp::TILE, j0 = tp.tj * dp::TILE;
    if (j0 >= n) return;                                                          // (j0 >= i0: no entry with both rows in the window)
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const int8_t *a_ptr[4], *b_ptr[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t ia = i0 + (uint32_t)t * 16 + r, ib = j0 + (uint32_t)t * 16 + r;
        uint64_t da = ia < n ? rows[ia].doc : 0u, db = ib < n ? rows[ib].doc : 0u;
        if (da >= p.n_docs) da = p.n_docs - 1;                                    // (an outside row: its entries are never read)
        if (db >= p.n_docs) db = p.n_docs - 1;
        a_ptr[t] = p.vec + da * p.dim + h * 16;
        b_ptr[t] = p.vec + db * p.dim + h * 16;
    }
    v4i acc[4][4];
#pragma unroll
    for (int ta = 0; ta < 4; ta++)
#pragma unroll
        for (int tb = 0; tb < 4; tb++) acc[ta][tb] = v4i{0, 0, 0, 0};
    for (uint32_t ks = 0; ks < p.dim; ks += 64) {
        v4i a[4], b[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            a[t] = *reinterpret_cast<const v4i*>(a_ptr[t] + ks);
            b[t] = *reinterpret_cast<const v4i*>(b_ptr[t] + ks);
        }
#pragma unroll
        for (int ta = 0; ta < 4; ta++)
#pragma unroll
            for (int tb = 0; tb < 4; tb++) acc[ta][tb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
    // ---- the tile and, off the diagonal, its transpose: only entries with both rows inside the window (all below pitch)
    int32_t* const g_q = p.gram + (size_t)local * p.pitch * p.pitch;
    const bool mirror = tp.ti != tp.tj;
#pragma unroll
    for (int ta = 0; ta < 4; ta++) {
        const uint32_t ib = i0 + (uint32_t)ta * 16 + h * 4;                       // rows ib .. ib + 3: the accumulator's four registers
#pragma unroll
        for (int tb = 0; tb < 4; tb++) {
            const uint32_t j = j0 + (uint32_t)tb * 16 + r;
            if (j >= n) continue;
#pragma unroll
            for (int g = 0; g < 4; g++)
                if (ib + (uint32_t)g < n) g_q[(size_t)(ib + (uint32_t)g) * p.pitch + j] = acc[ta][tb][g];
            if (!mirror) continue;
            int32_t* const t_row = g_q + (size_t)j * p.pitch + ib;               // (16-byte aligned: pitch and ib are multiples of 4)
            if (ib + 3 < n) *reinterpret_cast<v4i*>(t_row) = acc[ta][tb];
            else
#pragma unroll
                for (int g = 0; g < 4; g++)
                    if (ib + (uint32_t)g < n) t_row[g] = acc[ta][tb][g];
        }
    }
}

struct DivSelectParams {
    const int32_t* gram;               // [queries of the group][pitch][pitch]; never read when n_docs == 0
    const int32_t* rel;                // [n_q][k_in] from k_vec_hit_scores, or nullptr: rel(j) = -j
    uint64_t n_docs;
    const ss_hit* hits;
    const int32_t* n_hits;
    ss_hit* hits_out;                  // [n_q][k]
    int32_t* n_hits_out;
    ss_div_info* info_out;             // [n_q][k], nullable
    uint32_t k_in, pitch, q0, first, k;
    int32_t w_rel, w_div;
};

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_div_select(DivSelectParams p) {
    constexpr uint32_t CAP = PER * BLOCK, NW = BLOCK / 64;
    __shared__ uint16_t s_order[CAP];                     // [c]: the window row of choice c
    __shared__ int32_t s_pen[CAP];                        // [c]: its penalty at the moment of choice
    __shared__ uint16_t s_outside[CAP];                   // the outside rows in window order
    __shared__ uint32_t s_cnt[PER * NW];                  // outside rows per (slot, wave)
    __shared__ uint64_t s_wmax[2][NW];                    // the waves' largest keys of a step, double-buffered: one barrier per step
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t local = blockIdx.x, q = p.q0 + local;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    // ---- slot s of thread t is window row s * BLOCK + t: classes, relevance, and the outside rows numbered in window order
    int32_t rel[PER], pen[PER];
    bool live[PER];
    uint32_t out_rank[PER];
#pragma unroll
    for (int s = 0; s < PER; s++) {
        const uint32_t j = (uint32_t)s * BLOCK + tid;
        const bool in_win = j < n;
        const bool inside = in_win && (uint64_t)rows[j].doc < p.n_docs;
        const uint64_t b = __ballot(in_win && !inside);
        out_rank[s] = in_win && !inside ? (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) : ~0u;
        if (lane == 0) s_cnt[s * NW + wave] = (uint32_t)__popcll(b);
        live[s] = inside;
        pen[s] = 0;
        rel[s] = !inside ? 0 : p.rel ? p.rel[(size_t)q * p.k_in + j] : -(int32_t)j;
    }
    __syncthreads();
    uint32_t n_outside = 0;
#pragma unroll
    for (int s = 0; s < PER; s++) {
        uint32_t before = n_outside;
        for (uint32_t w = 0; w < NW; w++) {
            if (w < wave) before += s_cnt[s * NW + w];
            n_outside += s_cnt[s * NW + w];
        }
        if (out_rank[s] != ~0u) s_outside[before + out_rank[s]] = (uint16_t)((uint32_t)s * BLOCK + tid);
    }
    const uint32_t n_inside = n - n_outside;
    const uint64_t want = (uint64_t)p.first + p.k;
    const uint32_t steps = want < n_inside ? (uint32_t)want : n_inside;
    const int32_t* const g_q = p.gram + (size_t)local * p.pitch * p.pitch;
    for (uint32_t step = 0; step < steps; step++) {
        uint64_t best = 0;                                                        // (no key is 0; at least one row is live)
#pragma unroll
        for (int s = 0; s < PER; s++)
            if (live[s]) {
                const uint64_t key = dp::select_key(dp::value_of(p.w_rel, rel[s], p.w_div, pen[s]), (uint32_t)s * BLOCK + tid);
                best = key > best ? key : best;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, o, 64);
            best = other > best ? other : best;
        }
        if (NW > 1) {
            if (lane == 0) s_wmax[step & 1u][wave] = best;
            __syncthreads();
#pragma unroll
            for (uint32_t w = 0; w < NW; w++) {
                const uint64_t other = s_wmax[step & 1u][w];
                best = other > best ? other : best;
            }
        }
        const uint32_t chosen = dp::key_row(best);                                // an inside row: < n <= pitch
        const int32_t* const g_row = g_q + (size_t)chosen * p.pitch;
#pragma unroll
        for (int s = 0; s < PER; s++) {
            const uint32_t j = (uint32_t)s * BLOCK + tid;
            if (!live[s]) continue;
            if (j == chosen) {
                live[s] = false;
                s_order[step] = (uint16_t)j;
                s_pen[step] = step ? pen[s] : SS_NO_VEC_SCORE;
            } else {
                const int32_t sim = g_row[j];
                pen[s] = step == 0 || sim > pen[s] ? sim : pen[s];                // (the first chosen row replaces the empty set's 0)
            }
        }
    }
    __syncthreads();
    // ---- the page: positions [first, first + n_out) of the chosen rows followed by the outside rows; every position below n_inside
    // is below steps
    const uint32_t n_out = hw::page_len(n, p.first, p.k);
    const auto row_at = [&](uint32_t r) -> uint32_t {
        const uint32_t x = p.first + r;
        return x < n_inside ? s_order[x] : s_outside[x - n_inside];
    };
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, row_at);
    if (p.info_out)
        for (uint32_t rr = tid; rr < n_out; rr += BLOCK) {
            const uint32_t x = p.first + rr;
            ss_div_info info{SS_NO_VEC_SCORE, SS_NO_VEC_SCORE};
            if (x < n_inside) {
                const uint32_t j = s_order[x];
                info.rel = p.rel ? p.rel[(size_t)q * p.k_in + j] : -(int32_t)j;
                info.sim = s_pen[x];
            }
            p.info_out[(size_t)q * p.k + rr] = info;
        }
    if (tid == 0) p.n_hits_out[q] = (int32_t)n_out;
}

constexpr int DS_SMALL = 64, DS_SMALL_PER = 2, DS_LARGE = 256, DS_LARGE_PER = 4;
static_assert(DS_LARGE * DS_LARGE_PER >= SS_MAX_TOPK, "k_div_select holds a whole window in its threads");

// a block of exactly what is asked for (the Gram scratch is bounded by an option), grow-only
int32_t ensure_exact(ss_ctx* ctx, ss::DevBuf<int32_t>& b, size_t n, const char* what) {
    if (b.p && b.n >= n) return SS_OK;
    const hipError_t e = b.alloc(n);
    if (e == hipSuccess) return SS_OK;
    (void)hipGetLastError();
    return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "ss_diversify_hits: no device memory for %zu bytes of %s", n * sizeof(int32_t), what);
}

int32_t diversify_impl(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t w_rel,
                       int32_t w_div, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, ss_div_info* info_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, "ss_diversify_hits", "k_in", n_q, k_in, k, first));
    SS_TRY(hw::check_page_arrays(ctx, "ss_diversify_hits", n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    {
        char msg[256];
        if (dp::check_weights(msg, sizeof(msg), "ss_diversify_hits", w_rel, w_div) != dp::OK) return ctx->fail(SS_ERR_INVALID, "%s", msg);
    }
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_diversify_hits: no vector table registered (ss_scorer_set_doc_vectors)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_diversify_hits", "k_in", n_q, k_in, hits, n_hits, &w));
    const uint32_t pitch = dp::pitch((uint32_t)k_in);
    const uint32_t group = dp::group_queries((uint64_t)n_q, (uint32_t)k_in, dp::scratch_bytes_of(ctx->opt("div.scratch_bytes", 0)));
    const bool table = s->n_docs > 0;                                             // without docs every row is outside: no Gram matrix
    if (table) SS_TRY(ensure_exact(ctx, s->d_div_gram, (size_t)group * pitch * pitch, "Gram scratch"));
    if (qvec) SS_TRY(ensure_exact(ctx, s->d_div_rel, (size_t)n_q * (size_t)k_in, "relevance rows"));
    SS_TRY(hw::window_stage(s, &w));
    const int8_t* d_q = nullptr;
    if (qvec) SS_TRY(ss::vec_queries_to_device(s, qvec, (size_t)n_q * (size_t)s->vec_dim, &d_q, &w.staged));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)n_q, (size_t)k, hits_out, n_hits_out, nullptr, info_out, sizeof(ss_div_info), &o));
    if (qvec) {
        ss::launch_vec_hit_scores(s, d_q, w.hits, w.n_hits, n_q, k_in, s->d_div_rel.p, st);
        SS_HIP(ctx, hipGetLastError());
    }
    DivGramParams gp{};
    gp.vec = s->vec.p;
    gp.n_docs = s->n_docs;
    gp.hits = w.hits;
    gp.n_hits = w.n_hits;
    gp.gram = s->d_div_gram.p;
    gp.dim = (uint32_t)s->vec_dim; gp.k_in = (uint32_t)k_in; gp.pitch = pitch; gp.n_tiles = pitch / dp::TILE;
    DivSelectParams sp{};
    sp.gram = s->d_div_gram.p;
    sp.rel = qvec ? s->d_div_rel.p : nullptr;
    sp.n_docs = s->n_docs;
    sp.hits = w.hits;
    sp.n_hits = w.n_hits;
    sp.hits_out = o.hits;
    sp.n_hits_out = o.n_hits;
    sp.info_out = static_cast<ss_div_info*>(o.extra);
    sp.k_in = (uint32_t)k_in; sp.pitch = pitch; sp.first = (uint32_t)first; sp.k = (uint32_t)k;
    sp.w_rel = w_rel; sp.w_div = w_div;
    // ---- the groups, one after another: a group's k_div_gram waits in stream order for the k_div_select that read the scratch before
    for (const dp::Launch& l : dp::launches((uint64_t)n_q, group)) {
        gp.q0 = sp.q0 = l.first;
        if (table) {
            hipLaunchKernelGGL(k_div_gram, dim3(dp::tile_pairs(gp.n_tiles), l.count), dim3(64), 0, st, gp);
            SS_HIP(ctx, hipGetLastError());
        }
        if (k_in <= DS_SMALL * DS_SMALL_PER)
            hipLaunchKernelGGL((k_div_select<DS_SMALL, DS_SMALL_PER>), dim3(l.count), dim3(DS_SMALL), 0, st, sp);
        else
            hipLaunchKernelGGL((k_div_select<DS_LARGE, DS_LARGE_PER>), dim3(l.count), dim3(DS_LARGE), 0, st, sp);
        SS_HIP(ctx, hipGetLastError());
    }
    return hw::rows_out_finish(s, o, w.staged);
}

}  // namespace

extern "C" {

int32_t ss_diversify_hits(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t w_rel,
                          int32_t w_div, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, ss_div_info* info_out) {
    return hw::guarded(s, "ss_diversify_hits",
                       [&] { return diversify_impl(s, n_q, qvec, k_in, hits, n_hits, w_rel, w_div, first, k, hits_out, n_hits_out, info_out); });
}

}  // extern "C"
