// maxsim.hip — ss_scorer_set_doc_tokens, ss_hit_maxsim_scores and ss_rerank_hits_by_maxsim: one signed 8-bit vector per doc token and
// per query token, and the late-interaction score of a window's rows: the sum, over the query's tokens, of the largest 32-bit integer
// dot product any of the doc's tokens reaches.
//
//   k_maxsim_scores<QT>  grid (query, run of at most 64 window rows), four waves.  The query's token vectors sit in LDS for the whole
//                        run: 16 QT rows of dim bytes at a padded stride, rows past m_q zero.  A wave takes one window row at a time
//                        and walks the doc's tokens 64 per iteration: four tiles of 16 tokens, loaded straight from memory as the A
//                        operand of __builtin_amdgcn_mfma_i32_16x16x64_i8 and multiplied with every 16-slot B tile read from LDS:
//                        4 x QT accumulators of 4 registers.  Both operands are loaded by vector.hip's rule — lane l holds bytes
//                        16 (l >> 4) .. + 15 of the 64-byte k step of row l & 15 — so byte i of a doc token meets byte i of a query
//                        token.  The rows of the last tiles are clamped to the doc's last token, so every address is inside the
//                        table.  After the k loop register g of lane l of tile (t, j) is doc token 64 it + 16 t + 4 (l >> 4) + g under
//                        query slot 16 j + (l & 15): the lane folds it into one running maximum per j, a token at or past T_d as
//                        INT32_MIN, never as its product.  At the end of the row two cross-lane steps take the maximum over the four
//                        lane groups, slots at or past m_q become 0, and the sum over 16 lanes and QT tiles is stored by one lane.
//                        A row whose doc has at least `wide_tokens` tokens is left to a second pass in which the four waves take
//                        alternate iterations and join their maxima per slot in LDS by integer max before the sum.  Max is
//                        associative and commutative: the score does not depend on who saw which token.
// The re-rank sorts with k_vec_sort_hits (vector.hip, through ss::launch_vec_sort_hits).  No float, no atomics.  The window in, the
// paging checks and the outputs' way back are hit_window.hpp's; what needs no device is maxsim_plan.hpp's.
#include "hit_window.hpp"
#include "maxsim_plan.hpp"
#include "maxsim_topk_plan.hpp"

#include <algorithm>
#include <climits>

namespace {

namespace hw = ss::hitwin;
namespace mp = ss::msp;

static_assert(SS_MAX_QUERY_TOKENS == mp::MAX_QUERY_TOKENS && SS_MAX_VEC_DIM == mp::MAX_DIM && SS_MAX_TOPK == mp::MAX_WINDOW,
              "maxsim_plan.hpp states the ABI's limits");
static_assert(SS_NO_VEC_SCORE == INT32_MIN, "a row without a score");

typedef int v4i __attribute__((ext_vector_type(4)));

struct MaxSimParams {
    const int8_t* tok;                 // [tok_ptr[n_docs]][dim]
    const uint64_t* tok_ptr;           // [n_docs + 1]
    uint64_t n_docs;
    const int8_t* qtok;                // 16-byte aligned; query q's tokens at rows qt_ptr[q] ..
    const uint32_t* qt_ptr;            // [n_q + 1], device
    const ss_hit* hits;                // [n_q][k_in]
    const int32_t* n_hits;
    int32_t* out;                      // [n_q][k_in]
    uint32_t dim, k_in, wg_rows, wgs_per_query, wide_tokens, row_stride;
};

// The running maxima of one window row: iterations it0, it0 + step, .. of the doc's T > 0 tokens (row0: its first token) folded into
// mx[j] of every lane.  b_ptr: the lane's 16 bytes of query slot r in LDS.
template <int QT>
__device__ __forceinline__ void row_maxima(const int8_t* row0, uint32_t T, uint32_t dim, const unsigned char* b_ptr, uint32_t row_stride,
                                           uint32_t it0, uint32_t step, uint32_t r, uint32_t h, int32_t (&mx)[QT]) {
    const uint32_t n_iter = (T + mp::ITER_TOKENS - 1) / mp::ITER_TOKENS;
    for (uint32_t it = it0; it < n_iter; it += step) {
        const uint32_t t0 = it * mp::ITER_TOKENS;                                 // < T
        const int8_t* a_ptr[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t x = t0 + (uint32_t)t * 16 + r;
            if (x >= T) x = T - 1;                                                // (its slots are masked below)
            a_ptr[t] = row0 + (uint64_t)x * dim + h * 16;
        }
        v4i acc[4][QT];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int j = 0; j < QT; j++) acc[t][j] = v4i{0, 0, 0, 0};
        for (uint32_t ks = 0; ks < dim; ks += 64) {
            v4i a[4];
#pragma unroll
            for (int t = 0; t < 4; t++) a[t] = *reinterpret_cast<const v4i*>(a_ptr[t] + ks);
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const v4i b = *reinterpret_cast<const v4i*>(b_ptr + (size_t)j * 16 * row_stride + ks);
#pragma unroll
                for (int t = 0; t < 4; t++) acc[t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b, acc[t][j], 0, 0, 0);
            }
        }
        // ---- register g of tile (t, j): doc token t0 + 16 t + 4 h + g under query slot 16 j + r
        if (T - t0 >= mp::ITER_TOKENS) {                                          // (uniform) every slot is a token
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int j = 0; j < QT; j++)
#pragma unroll
                    for (int g = 0; g < 4; g++) mx[j] = max(mx[j], acc[t][j][g]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const bool live = t0 + (uint32_t)(t * 16 + g) + h * 4 < T;
#pragma unroll
                    for (int j = 0; j < QT; j++) mx[j] = max(mx[j], live ? acc[t][j][g] : INT32_MIN);
                }
        }
    }
}

// the maximum over the four lane groups: afterwards every lane holds, per j, the maximum of query slot 16 j + (lane & 15)
template <int QT>
__device__ __forceinline__ void join_lane_groups(int32_t (&mx)[QT]) {
#pragma unroll
    for (int j = 0; j < QT; j++) {
        mx[j] = max(mx[j], __shfl_xor(mx[j], 16));
        mx[j] = max(mx[j], __shfl_xor(mx[j], 32));
    }
}

// slots at or past m_q as 0, then the sum over the 16 slots of every tile: the row's score in every lane
template <int QT>
__device__ __forceinline__ int32_t sum_slots(const int32_t (&mx)[QT], uint32_t r, uint32_t m_q) {
    int32_t sum = 0;
#pragma unroll
    for (int j = 0; j < QT; j++) sum += (uint32_t)j * 16 + r < m_q ? mx[j] : 0;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
    return sum;
}

template <int QT>
__global__ __launch_bounds__(mp::TPB) void k_maxsim_scores(MaxSimParams p) {
    constexpr uint32_t QB = QT * 16;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const s_q = smem;                                              // [QB][row_stride]
    int32_t* const s_join = reinterpret_cast<int32_t*>(smem + (size_t)QB * p.row_stride);   // [WAVES][QB]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = lane & 15u, h = lane >> 4;
    const uint32_t q = blockIdx.x / p.wgs_per_query, r0 = (blockIdx.x - q * p.wgs_per_query) * p.wg_rows;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);
    if (r0 >= n) return;                                                          // (the whole workgroup)
    const uint32_t n_rows = n - r0 < p.wg_rows ? n - r0 : p.wg_rows;              // <= 64
    const uint32_t qb = p.qt_ptr[q];
    uint32_t m_q = p.qt_ptr[q + 1] - qb;
    if (m_q > QB) m_q = QB;                                                       // (the host chose QT from the largest m_q)
    const uint32_t dim = p.dim;
    // ---- the query's token vectors into LDS, rows past m_q zero
    const uint32_t row_chunks = dim / 16;
    for (uint32_t x = tid; x < QB * row_chunks; x += mp::TPB) {
        const uint32_t row = x / row_chunks, c = x - row * row_chunks;
        v4i v = {0, 0, 0, 0};
        if (row < m_q) v = *reinterpret_cast<const v4i*>(p.qtok + (size_t)(qb + row) * dim + (size_t)c * 16);
        *reinterpret_cast<v4i*>(s_q + (size_t)row * p.row_stride + (size_t)c * 16) = v;
    }
    // ---- the run's rows, one per lane (every wave reads the same): token count (0: no score) and first token
    uint32_t T = 0;
    uint64_t first_tok = 0;
    if (lane < n_rows) {
        const uint32_t d = p.hits[(size_t)q * p.k_in + r0 + lane].doc;
        if ((uint64_t)d < p.n_docs) {
            first_tok = p.tok_ptr[d];
            T = (uint32_t)(p.tok_ptr[(uint64_t)d + 1] - first_tok);               // < 2^31: checked when the table was registered
        }
    }
    const uint64_t wide = __ballot(T >= p.wide_tokens);                           // (wide_tokens >= 1) the same word in every wave
    __syncthreads();
    int32_t* const out = p.out + (size_t)q * p.k_in + r0;
    const unsigned char* const b_ptr = s_q + (size_t)r * p.row_stride + h * 16;
    // ---- pass 1: a wave takes a row at a time
    for (uint32_t i = wave; i < n_rows; i += mp::WAVES) {
        if (wide >> i & 1ull) continue;
        const uint32_t Ti = __shfl(T, (int)i);
        const uint64_t fi = (uint64_t)__shfl((uint32_t)first_tok, (int)i) | (uint64_t)__shfl((uint32_t)(first_tok >> 32), (int)i) << 32;
        int32_t score = SS_NO_VEC_SCORE;
        if (Ti) {
            int32_t mx[QT];
#pragma unroll
            for (int j = 0; j < QT; j++) mx[j] = INT32_MIN;
            row_maxima<QT>(p.tok + fi * dim, Ti, dim, b_ptr, p.row_stride, 0, 1, r, h, mx);
            join_lane_groups<QT>(mx);
            score = sum_slots<QT>(mx, r, m_q);
        }
        if (lane == 0) out[i] = score;
    }
    // ---- pass 2: the wide rows, every wave every fourth iteration, the maxima joined in LDS
    for (uint64_t left = wide; left; left &= left - 1) {
        const uint32_t i = (uint32_t)__builtin_ctzll(left);
        const uint32_t Ti = __shfl(T, (int)i);
        const uint64_t fi = (uint64_t)__shfl((uint32_t)first_tok, (int)i) | (uint64_t)__shfl((uint32_t)(first_tok >> 32), (int)i) << 32;
        int32_t mx[QT];
#pragma unroll
        for (int j = 0; j < QT; j++) mx[j] = INT32_MIN;
        row_maxima<QT>(p.tok + fi * dim, Ti, dim, b_ptr, p.row_stride, wave, mp::WAVES, r, h, mx);
        join_lane_groups<QT>(mx);
        if (h == 0) {
#pragma unroll
            for (int j = 0; j < QT; j++) s_join[wave * QB + (uint32_t)j * 16 + r] = mx[j];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int j = 0; j < QT; j++) {
                int32_t v = s_join[(uint32_t)j * 16 + r];
#pragma unroll
                for (uint32_t w = 1; w < mp::WAVES; w++) v = max(v, s_join[w * QB + (uint32_t)j * 16 + r]);
                mx[j] = v;
            }
            const int32_t score = sum_slots<QT>(mx, r, m_q);
            if (lane == 0) out[i] = score;
        }
        __syncthreads();                                                          // (s_join is free for the next wide row)
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The queries of a call after its host checks: qt_ptr on the host and the QT its kernel needs.
struct QueryTokens {
    std::vector<uint32_t> h_ptr;       // [n_q + 1]
    uint32_t qt = 1;
};

// qt_ptr fetched and checked; qtok present if any query has a token.  Enqueues nothing that writes.
int32_t fetch_query_tokens(ss_ctx* ctx, const char* entry, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, QueryTokens* out) {
    const size_t nq = (size_t)n_q;
    out->h_ptr.assign(nq + 1, 0u);
    if (nq == 0) return SS_OK;
    if (!qt_ptr) return ctx->fail(SS_ERR_INVALID, "%s: qt_ptr is NULL", entry);
    SS_HIP(ctx, ss::copy_in(ctx->stream, out->h_ptr.data(), qt_ptr, (nq + 1) * sizeof(uint32_t)));
    char msg[256];
    uint32_t max_m = 0;
    const int rc = mp::check_qt_ptr(msg, sizeof(msg), entry, out->h_ptr.data(), nq, &max_m);
    if (rc != mp::OK) return ctx->fail(rc == mp::INVALID ? SS_ERR_INVALID : SS_ERR_UNSUPPORTED, "%s", msg);
    if (!qtok && out->h_ptr[nq] != out->h_ptr[0]) return ctx->fail(SS_ERR_INVALID, "%s: qtok is NULL", entry);
    out->qt = mp::qt_of(max_m);
    return SS_OK;
}

// The query tokens on the device, 16-byte aligned, and qt_ptr rebased to their first row in a device block.  qtok: the caller's array
// when it is aligned device memory, otherwise a copy in a block the scorer owns (*staged: from host memory, so the call waits before it
// returns).  qt_ptr goes up through a pinned block whose last copy is waited for first: the call never waits for its own copy.
int32_t query_tokens_to_device(ss_scorer* s, const QueryTokens& qt, const int8_t* qtok, const int8_t** d_qtok, bool* staged) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t n = qt.h_ptr.size(), dim = (size_t)s->tok_dim;
    const uint32_t base = qt.h_ptr[0];
    const size_t bytes = (size_t)(qt.h_ptr[n - 1] - base) * dim;
    const int8_t* const src = qtok ? qtok + (size_t)base * dim : nullptr;
    const bool dev = ss::on_device(src);
    if (!bytes || (dev && ((uintptr_t)src & 15u) == 0)) *d_qtok = src;
    else {
        SS_HIP(ctx, ensure(s->d_ms_q, bytes));
        SS_HIP(ctx, hipMemcpyAsync(s->d_ms_q.p, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        *d_qtok = s->d_ms_q.p;
        if (!dev) *staged = true;
    }
    SS_HIP(ctx, s->ev_ms_qptr.wait());
    SS_HIP(ctx, s->h_ms_qptr.ensure(n * sizeof(uint32_t)));
    SS_HIP(ctx, ensure(s->d_ms_qptr, n));
    uint32_t* const h = s->h_ms_qptr.as<uint32_t>();
    for (size_t i = 0; i < n; i++) h[i] = qt.h_ptr[i] - base;
    SS_HIP(ctx, hipMemcpyAsync(s->d_ms_qptr.p, h, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, s->ev_ms_qptr.record(st));
    return SS_OK;
}

template <int QT>
int32_t launch_qt(ss_scorer* s, const MaxSimParams& p, const mp::Grid& g, uint32_t lds, hipStream_t st) {
    ss_ctx* ctx = s->ctx;
    if (s->ms_lds_attr[QT] < (int)lds) {
        SS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_maxsim_scores<QT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        s->ms_lds_attr[QT] = (int)lds;
    }
    hipLaunchKernelGGL((k_maxsim_scores<QT>), dim3((unsigned)g.n_wgs), dim3(mp::TPB), lds, st, p);
    return SS_OK;
}

// k_maxsim_scores over a window in device memory
int32_t launch_maxsim(ss_scorer* s, uint32_t qt, const mp::Grid& g, const int8_t* d_qtok, const hw::WindowIn& w, int32_t k_in, int32_t* out, hipStream_t st) {
    ss_ctx* ctx = s->ctx;
    MaxSimParams p{};
    p.tok = s->tok.p;
    p.tok_ptr = s->tok_ptr.p;
    p.n_docs = s->n_docs;
    p.qtok = d_qtok;
    p.qt_ptr = s->d_ms_qptr.p;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.out = out;
    p.dim = (uint32_t)s->tok_dim;
    p.k_in = (uint32_t)k_in;
    p.wg_rows = g.wg_rows;
    p.wgs_per_query = g.wgs_per_query;
    p.wide_tokens = mp::wide_tokens_of(ctx->opt("maxsim.wide_tokens", 0));
    p.row_stride = mp::row_stride(p.dim);
    const uint32_t lds = mp::lds_bytes(qt, p.dim);
    if (qt == 4) SS_TRY(launch_qt<4>(s, p, g, lds, st));
    else if (qt == 2) SS_TRY(launch_qt<2>(s, p, g, lds, st));
    else SS_TRY(launch_qt<1>(s, p, g, lds, st));
    SS_HIP(ctx, hipGetLastError());
    return SS_OK;
}

int32_t grid_of(ss_ctx* ctx, const char* entry, int32_t n_q, int32_t k_in, mp::Grid* g) {
    *g = mp::grid((uint64_t)n_q, (uint32_t)k_in, (uint32_t)ctx->cu_count);
    if (!g->ok) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: %d queries at k_in = %d need more workgroups than one launch holds", entry, n_q, k_in);
    return SS_OK;
}

int32_t hit_scores_impl(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, int32_t k_in, const ss_hit* hits, const int32_t* n_hits,
                        int32_t* scores_out) {
    static const char* const who = "ss_hit_maxsim_scores";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_q < 0", who);
    if (k_in < 1) return ctx->fail(SS_ERR_INVALID, "%s: k_in = %d must be >= 1", who, k_in);
    if (k_in > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: k_in = %d exceeds SS_MAX_TOPK = %d", who, k_in, SS_MAX_TOPK);
    if (n_q > 0 && (!hits || !n_hits || !scores_out)) return ctx->fail(SS_ERR_INVALID, "%s: hits, n_hits or scores_out is NULL", who);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    QueryTokens qt;
    SS_TRY(fetch_query_tokens(ctx, who, n_q, qt_ptr, qtok, &qt));
    if (s->tok_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no token table registered (ss_scorer_set_doc_tokens)", who);
    if (n_q == 0) return SS_OK;
    mp::Grid g;
    SS_TRY(grid_of(ctx, who, n_q, k_in, &g));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, who, "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const int8_t* d_q = nullptr;
    SS_TRY(query_tokens_to_device(s, qt, qtok, &d_q, &w.staged));
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, scores_out, (size_t)n_q * (size_t)k_in * sizeof(int32_t), &o));
    SS_TRY(launch_maxsim(s, qt.qt, g, d_q, w, k_in, static_cast<int32_t*>(o.dev), st));
    return hw::entries_out_finish(s, o, w, sizeof(int32_t));
}

int32_t rerank_impl(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, int32_t k_in, const ss_hit* hits, const int32_t* n_hits,
                    int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, int32_t* scores_out) {
    static const char* const who = "ss_rerank_hits_by_maxsim";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, who, "k_in", n_q, k_in, k, first));
    SS_TRY(hw::check_page_arrays(ctx, who, n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    SS_HIP(ctx, hipSetDevice(ctx->device));
    QueryTokens qt;
    SS_TRY(fetch_query_tokens(ctx, who, n_q, qt_ptr, qtok, &qt));
    if (s->tok_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no token table registered (ss_scorer_set_doc_tokens)", who);
    if (n_q == 0) return SS_OK;
    mp::Grid g;
    SS_TRY(grid_of(ctx, who, n_q, k_in, &g));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, who, "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const int8_t* d_q = nullptr;
    SS_TRY(query_tokens_to_device(s, qt, qtok, &d_q, &w.staged));
    SS_HIP(ctx, ensure(s->d_ms_scores, (size_t)n_q * (size_t)k_in));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)n_q, (size_t)k, hits_out, n_hits_out, nullptr, scores_out, sizeof(int32_t), &o));
    SS_TRY(launch_maxsim(s, qt.qt, g, d_q, w, k_in, s->d_ms_scores.p, st));
    ss::launch_vec_sort_hits(s->d_ms_scores.p, w.hits, w.n_hits, n_q, k_in, first, k, o.hits, o.n_hits, static_cast<int32_t*>(o.extra), st);
    SS_HIP(ctx, hipGetLastError());
    return hw::rows_out_finish(s, o, w.staged);
}

int32_t set_doc_tokens_impl(ss_scorer* s, int32_t dim, const uint64_t* tok_ptr, const int8_t* tok) {
    static const char* const who = "ss_scorer_set_doc_tokens";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool clear = dim == 0 || !tok;
    if (!clear && !mp::dim_ok(dim)) return ctx->fail(SS_ERR_INVALID, "%s: dim = %d is not a multiple of 64 in [64, %d]", who, dim, SS_MAX_VEC_DIM);
    if (!clear && !tok_ptr) return ctx->fail(SS_ERR_INVALID, "%s: tok_ptr is NULL", who);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    ss::DevBuf<int8_t> nb;
    ss::DevBuf<uint64_t> nbp;
    std::vector<uint64_t> h_ptr;
    ss::DevBuf<uint32_t> ncut;                                                    // ss_maxsim_topk's cut table (maxsim_topk_plan.hpp)
    std::vector<uint32_t> h_cut;
    const size_t nd = (size_t)s->n_docs;
    size_t rows = 0, bytes = 0;
    if (!clear) {
        h_ptr.resize(nd + 1);
        SS_HIP(ctx, ss::copy_in(ctx->stream, h_ptr.data(), tok_ptr, (nd + 1) * sizeof(uint64_t)));
        char msg[256];
        const int rc = mp::check_tok_ptr(msg, sizeof(msg), who, h_ptr.data(), nd);
        if (rc != mp::OK) return ctx->fail(rc == mp::INVALID ? SS_ERR_INVALID : SS_ERR_UNSUPPORTED, "%s", msg);
        rows = (size_t)h_ptr[nd];
        if (rows > SIZE_MAX / (size_t)dim) return ctx->fail(SS_ERR_OOM, "%s: %zu tokens of %d bytes do not fit", who, rows, dim);
        bytes = rows * (size_t)dim;
        hipError_t e = nb.alloc(std::max<size_t>(bytes, 16));                     // (a failure here leaves the old table in place)
        if (e == hipSuccess) e = nbp.alloc(nd + 1);
        if (!(s->n_docs >> 32)) ss::mtp::build_cuts(h_ptr.data(), nd, &h_cut);     // (doc ids of 32 bits; without it ss_maxsim_topk refuses)
        if (e == hipSuccess && !h_cut.empty()) e = ncut.alloc(h_cut.size());
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %zu bytes", who, bytes + (nd + 1) * 8);
        }
    }
    // the scorer's outstanding work may read the old table: drained, as ss_scorer_set_doc_vectors does, before the table is replaced
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    if (clear) {
        s->tok.release();
        s->tok_ptr.release();
        s->tok_cut.release();
        s->tok_slices = 0;
        s->tok_dim = 0;
        s->tok_rows = 0;
        return SS_OK;
    }
    if (bytes) SS_HIP(ctx, hipMemcpyAsync(nb.p, tok, bytes, hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipMemcpyAsync(nbp.p, h_ptr.data(), (nd + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (!h_cut.empty()) SS_HIP(ctx, hipMemcpyAsync(ncut.p, h_cut.data(), h_cut.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->tok = std::move(nb);
    s->tok_ptr = std::move(nbp);
    s->tok_cut = std::move(ncut);
    s->tok_slices = h_cut.empty() ? 0 : h_cut.size() - 1;
    s->tok_dim = dim;
    s->tok_rows = rows;
    return SS_OK;
}

}  // namespace

// for maxsim_topk.hip (scorer.hpp): the host checks and the staging of a call's query tokens, both as the calls above use them
int32_t ss::maxsim_check_query_tokens(ss_ctx* ctx, const char* entry, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok,
                                      std::vector<uint32_t>* h_ptr, uint32_t* qt) {
    QueryTokens t;
    SS_TRY(fetch_query_tokens(ctx, entry, n_q, qt_ptr, qtok, &t));
    *h_ptr = std::move(t.h_ptr);
    *qt = t.qt;
    return SS_OK;
}
int32_t ss::maxsim_query_tokens_to_device(ss_scorer* s, const std::vector<uint32_t>& h_ptr, const int8_t* qtok, const int8_t** d_qtok, bool* staged) {
    QueryTokens t;
    t.h_ptr = h_ptr;
    return query_tokens_to_device(s, t, qtok, d_qtok, staged);
}

extern "C" {

int32_t ss_scorer_set_doc_tokens(ss_scorer* s, int32_t dim, const uint64_t* tok_ptr, const int8_t* tok) {
    return hw::guarded(s, "ss_scorer_set_doc_tokens", [&] { return set_doc_tokens_impl(s, dim, tok_ptr, tok); });
}

int32_t ss_hit_maxsim_scores(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, int32_t k_in, const ss_hit* hits,
                             const int32_t* n_hits, int32_t* scores_out) {
    return hw::guarded(s, "ss_hit_maxsim_scores", [&] { return hit_scores_impl(s, n_q, qt_ptr, qtok, k_in, hits, n_hits, scores_out); });
}

int32_t ss_rerank_hits_by_maxsim(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, int32_t k_in, const ss_hit* hits,
                                 const int32_t* n_hits, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, int32_t* scores_out) {
    return hw::guarded(s, "ss_rerank_hits_by_maxsim",
                       [&] { return rerank_impl(s, n_q, qt_ptr, qtok, k_in, hits, n_hits, first, k, hits_out, n_hits_out, scores_out); });
}

}  // extern "C"
