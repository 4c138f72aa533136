// rank_model.hip — ss_rank_model_*, ss_hit_features and ss_rerank_hits_by_model: a tree ensemble over the signals of a result row, and a
// window re-ranked by its scores.  A step file beside proximity.hip and vector.hip: three kernels behind whatever made
// the rows, no scoring kernel edited.  rank_model_plan.hpp holds the pure host part: the validation of a model, the packed node, the
// chunk cut.
//
//   k_hit_features      one lane per window row: plain gathers of the row, its proximity entry, its vector score, the query's length
//                       and the doc's fields; the 15 values go through the LDS so that a wave's stores are contiguous runs.
//   k_forest_eval       the hot path, shared by ss_rank_model_eval and the re-rank.  A workgroup owns a tile of rows, one lane per row.
//                       The tile's feature values sit in the LDS column-major ([f][lane]): a lane's dynamically indexed read hits its
//                       own bank and no row of 15 to 64 doubles becomes scratch.  The forest is walked in chunks of consecutive whole
//                       trees (rankp::chunk_end, the same in every thread): the workgroup loads a chunk's nodes into the LDS, crosses a
//                       barrier, and every lane walks its row through the chunk's trees in order, adding each leaf into its
//                       accumulator.  A tree larger than the cap ("rank.lds_nodes") is walked from global memory by the same code.
//                       The additions are in tree order whatever the chunking: the same bytes for every cap.
//   k_model_sort_hits   one workgroup per query, the frame of k_prox_sort_hits with the scores given: (class, score key, window
//                       index) sorted in the LDS and the page copied out.  (k_prox_sort_hits computes its scores from the entries and
//                       cannot take them.)
// The window in and the way back of host outputs: hit_window.hpp.
#include "hit_window.hpp"
#include "rank_model_plan.hpp"

#include <algorithm>
#include <cstddef>
#include <memory>

namespace rp = ss::rankp;

static_assert(SS_MAX_RANK_FEATURES == rp::MAX_FEATURES && SS_MAX_RANK_TREES == rp::MAX_TREES, "rank_model_plan.hpp restates the ABI's limits");
static_assert(sizeof(ss_tree_node) == sizeof(rp::Node) && sizeof(ss_tree_node) == 24 && offsetof(ss_tree_node, feature) == offsetof(rp::Node, feature) &&
                  offsetof(ss_tree_node, left) == offsetof(rp::Node, left) && offsetof(ss_tree_node, right) == offsetof(rp::Node, right) &&
                  offsetof(ss_tree_node, nan_left) == offsetof(rp::Node, nan_left) && offsetof(ss_tree_node, value) == offsetof(rp::Node, value),
              "rankp::Node is ss_tree_node");
static_assert(sizeof(ss_rank_model_info) == sizeof(rp::Info) && offsetof(ss_rank_model_info, n_nodes) == offsetof(rp::Info, n_nodes) &&
                  offsetof(ss_rank_model_info, max_depth) == offsetof(rp::Info, max_depth),
              "rankp::Info is ss_rank_model_info");
static_assert(sizeof(rp::PNode) == 16, "a packed node is one 16-byte LDS read");

struct ss_rank_model {
    ss_ctx* ctx = nullptr;
    rp::Info info{};
    double base = 0.0;
    bool has_linear = false;
    ss::DevBuf<double> d_linear;                          // [n_features]
    ss::DevBuf<uint32_t> d_tree_ptr;                      // [n_trees + 1]
    ss::DevBuf<rp::PNode> d_nodes;                        // [n_nodes]
    // ss_rank_model_eval: device blocks of a HOST x / scores_out (grow-only; a call that uses one waits before it returns)
    ss::DevBuf<double> d_x, d_out;
};

namespace {

namespace hw = ss::hitwin;

constexpr uint64_t RM_NAN_BITS = 0x7FF8000000000000ull;   // "absent", and a NaN score
constexpr uint32_t NF = SS_RANK_N_FEATURES;
static_assert(sizeof(ss_proximity) == 24, "an entry is six dwords");
constexpr size_t PX_WORDS = sizeof(ss_proximity) / 4;

// ---- the features of a window ---------------------------------------------------------------------------------------------------
constexpr int HF_TPB = 256;

struct HitFeatParams {
    const ss_hit* hits;                                   // [n_q][k_in]
    const int32_t* n_hits;                                // [n_q]
    const uint32_t* prox;                                 // [n_q][k_in] six dwords each, nullable
    const int32_t* vec_scores;                            // [n_q][k_in], nullable
    const int32_t* query_len;                             // [n_q], nullable
    const int64_t* fields;                                // [n_fields][n_docs]
    uint64_t n_docs;
    uint64_t* out;                                        // [n_q][k_in][NF] the bits of doubles
    uint32_t k_in, n_fields;
    uint64_t total;                                       // n_q * k_in
};

__device__ __forceinline__ uint64_t rm_bits(double v) { return (uint64_t)__double_as_longlong(v); }

__global__ __launch_bounds__(HF_TPB) void k_hit_features(HitFeatParams p) {
    __shared__ uint64_t s_f[HF_TPB * NF];
    __shared__ uint32_t s_live[HF_TPB];
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * HF_TPB, row = row0 + tid;
    bool live = false;
    uint32_t q = 0, j = 0;
    if (row < p.total) {
        q = (uint32_t)(row / p.k_in);
        j = (uint32_t)(row - (uint64_t)q * p.k_in);
        live = j < hw::window_len(p.n_hits[q], p.k_in);
    }
    s_live[tid] = live ? 1u : 0u;
    if (live) {
        uint64_t* const f = s_f + (size_t)tid * NF;
        const uint64_t* const rw = reinterpret_cast<const uint64_t*>(p.hits + row);
        f[0] = rw[1]; f[1] = rw[2]; f[2] = rw[3]; f[3] = rw[4];               // title, body, pagerank, final: the bytes as given
        f[4] = rm_bits((double)j);
        f[5] = p.query_len ? rm_bits((double)p.query_len[q]) : RM_NAN_BITS;
        if (p.prox) {
            const uint32_t* const e = p.prox + row * PX_WORDS;                // (a caller's array need only be aligned to 4 bytes)
            const uint32_t n_present = e[2];
            const double sp = (double)__uint_as_float(e[1]) - (double)__uint_as_float(e[0]);
            const double gaps = (double)(n_present - 1u);
            const double prox = n_present < 2u ? 0.0 : gaps / (sp > gaps ? sp : gaps);
            f[6] = rm_bits((double)n_present);
            f[7] = rm_bits(sp);
            f[8] = rm_bits(prox);
            f[9] = rm_bits((double)e[3]);
        } else {
            f[6] = f[7] = f[8] = f[9] = RM_NAN_BITS;
        }
        const int32_t vs = p.vec_scores ? p.vec_scores[row] : SS_NO_VEC_SCORE;
        f[10] = vs == SS_NO_VEC_SCORE ? RM_NAN_BITS : rm_bits((double)vs);
        const uint64_t d = (uint64_t)p.hits[row].doc;
        for (uint32_t c = 0; c < (uint32_t)SS_MAX_DOC_FIELDS; c++) {
            const int64_t v = c < p.n_fields && d < p.n_docs ? p.fields[(uint64_t)c * p.n_docs + d] : SS_NO_FIELD_VALUE;
            f[11 + c] = v == SS_NO_FIELD_VALUE ? RM_NAN_BITS : rm_bits((double)v);
        }
    }
    __syncthreads();
    // the block's rows stand behind each other in `out`: lane x moves value x % NF of row x / NF
    uint64_t* const out = p.out + row0 * NF;
    for (uint32_t x = tid; x < HF_TPB * NF; x += HF_TPB)
        if (s_live[x / NF]) out[x] = s_f[x];
}
static_assert(NF == 11 + SS_MAX_DOC_FIELDS, "the fields are the last columns");

// ---- the forest --------------------------------------------------------------------------------------------------------------------
struct ForestParams {
    const double* x;                                      // [n_rows][n_features]
    uint64_t* out;                                        // [n_rows] the bits of a double
    const int32_t* n_hits;                                // nullable: row r is entry (r / k_in, r % k_in) of a window, skipped past its count
    const double* linear;                                 // [n_features], nullable
    const uint32_t* tree_ptr;                             // [n_trees + 1]
    const rp::PNode* nodes;
    double base;
    uint64_t n_rows;
    uint32_t n_features, n_trees, cap, k_in;
};

// One tree of `size` nodes from its node 0 to a leaf, for the row whose values are sx[f * ROWS]; the leaf's value.  Ends within `size`
// steps on any bytes: indices only grow in a checked model, and the loop counts as well.
template <int ROWS>
__device__ __forceinline__ double rm_walk(const rp::PNode* tree, uint32_t size, const double* sx) {
    uint32_t i = 0;
    rp::PNode nd = tree[0];
    for (uint32_t steps = size; steps > 1u && !rp::link_is_leaf(nd.link); steps--) {
        const double xv = sx[rp::link_feature(nd.link) * ROWS];
        const bool left = xv != xv ? rp::link_nan_left(nd.link) : xv <= nd.value;
        i = left ? rp::link_left(nd.link) : rp::link_right(nd.link);
        i = i < size ? i : size - 1u;                     // (never taken in a checked model)
        nd = tree[i];
    }
    return rp::link_is_leaf(nd.link) ? nd.value : 0.0;
}

template <int ROWS, int FCAP>
__global__ __launch_bounds__(ROWS) void k_forest_eval(ForestParams p) {
    __shared__ double s_x[FCAP * ROWS];                   // [f][lane]
    __shared__ __attribute__((aligned(16))) rp::PNode s_nodes[rp::LDS_NODES_MAX];
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * ROWS;
    const uint32_t n_here = p.n_rows - r0 < (uint64_t)ROWS ? (uint32_t)(p.n_rows - r0) : (uint32_t)ROWS;
    const uint32_t F = p.n_features;                      // <= FCAP: the launcher picks the instance
    const double* const src = p.x + r0 * F;
    for (uint32_t e = tid; e < n_here * F; e += ROWS) {   // the tile is one contiguous run of the matrix
        const uint32_t r = e / F, f = e - r * F;
        s_x[f * ROWS + r] = src[e];
    }
    __syncthreads();
    bool live = tid < n_here;
    if (live && p.n_hits) {
        const uint64_t row = r0 + tid, q = row / p.k_in;
        live = (uint32_t)(row - q * p.k_in) < hw::window_len(p.n_hits[q], p.k_in);
    }
    const double* const sx = s_x + tid;
    double acc = p.base;
    if (live && p.linear)
        for (uint32_t f = 0; f < F; f++) {
            const double w = p.linear[f], xv = sx[f * ROWS];
            if (w != 0.0 && xv == xv) {
                const double m = w * xv;
                acc = acc + m;
            }
        }
    for (uint32_t t = 0; t < p.n_trees;) {                // (the same in every thread: the barriers below are met by all)
        const uint32_t e = rp::chunk_end(p.tree_ptr, p.n_trees, t, p.cap);
        const uint32_t n0 = p.tree_ptr[t], nn = p.tree_ptr[e] - n0;
        if (nn > p.cap) {                                 // one tree larger than the cap: from global memory
            if (live) acc = acc + rm_walk<ROWS>(p.nodes + n0, nn, sx);
        } else {
            __syncthreads();                              // the last chunk's walks are over
            for (uint32_t i = tid; i < nn; i += ROWS) s_nodes[i] = p.nodes[n0 + i];   // nn <= cap <= LDS_NODES_MAX
            __syncthreads();
            if (live)
                for (uint32_t u = t; u < e; u++) {
                    const uint32_t b = p.tree_ptr[u];
                    acc = acc + rm_walk<ROWS>(s_nodes + (b - n0), p.tree_ptr[u + 1] - b, sx);
                }
        }
        t = e;
    }
    if (live) p.out[r0 + tid] = acc != acc ? RM_NAN_BITS : rm_bits(acc);
}

constexpr int FE_ROWS_NARROW = 256, FE_FCAP_NARROW = 16, FE_ROWS_WIDE = 64, FE_FCAP_WIDE = 64;
static_assert(FE_FCAP_WIDE >= SS_MAX_RANK_FEATURES && FE_FCAP_NARROW >= SS_RANK_N_FEATURES, "an instance for every model");
static_assert((size_t)FE_ROWS_NARROW * FE_FCAP_NARROW * 8 + rp::LDS_NODES_MAX * sizeof(rp::PNode) <= 64 * 1024 &&
                  (size_t)FE_ROWS_WIDE * FE_FCAP_WIDE * 8 + rp::LDS_NODES_MAX * sizeof(rp::PNode) <= 64 * 1024,
              "feature tile and chunk fit the static LDS limit");

// k_forest_eval over n_rows > 0 rows in device memory (n_hits / k_in: see ForestParams)
void launch_forest(const ss_rank_model* m, const double* d_x, double* d_out, uint64_t n_rows, const int32_t* d_n_hits, uint32_t k_in, hipStream_t st) {
    ForestParams p{};
    p.x = d_x;
    p.out = reinterpret_cast<uint64_t*>(d_out);
    p.n_hits = d_n_hits;
    p.linear = m->has_linear ? m->d_linear.p : nullptr;
    p.tree_ptr = m->d_tree_ptr.p;
    p.nodes = m->d_nodes.p;
    p.base = m->base;
    p.n_rows = n_rows;
    p.n_features = (uint32_t)m->info.n_features;
    p.n_trees = (uint32_t)m->info.n_trees;
    p.cap = rp::clamp_cap(m->ctx->opt("rank.lds_nodes", rp::LDS_NODES_DEFAULT));
    p.k_in = k_in;
    if (m->info.n_features <= FE_FCAP_NARROW)
        hipLaunchKernelGGL((k_forest_eval<FE_ROWS_NARROW, FE_FCAP_NARROW>), dim3((unsigned)((n_rows + FE_ROWS_NARROW - 1) / FE_ROWS_NARROW)),
                           dim3(FE_ROWS_NARROW), 0, st, p);
    else
        hipLaunchKernelGGL((k_forest_eval<FE_ROWS_WIDE, FE_FCAP_WIDE>), dim3((unsigned)((n_rows + FE_ROWS_WIDE - 1) / FE_ROWS_WIDE)),
                           dim3(FE_ROWS_WIDE), 0, st, p);
}

// ---- a window sorted by given scores ---------------------------------------------------------------------------------------------
constexpr uint32_t MS_CLASS_SHIFT = 16;                   // tag = class << 16 | window index (< SS_MAX_TOPK = 2^10)
constexpr uint32_t MS_NAN = 1, MS_OUTSIDE = 2, MS_DEAD = 3;

struct ModelSortParams {
    const uint64_t* scores;                               // [n_q][k_in] the bits of doubles, from k_forest_eval
    uint64_t n_docs;
    const ss_hit* hits;
    const int32_t* n_hits;
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;
    uint64_t* scores_out;                                 // [n_q][k], nullable
    uint32_t k_in, first, k;
};

__device__ __forceinline__ bool ms_after(uint64_t ka, uint32_t ta, uint64_t kb, uint32_t tb) {
    const uint32_t ca = ta >> MS_CLASS_SHIFT, cb = tb >> MS_CLASS_SHIFT;
    return ca != cb ? ca > cb : ka != kb ? ka > kb : ta > tb;
}

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_model_sort_hits(ModelSortParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    __shared__ uint64_t s_key[CAP];
    __shared__ uint64_t s_score[CAP];                     // by window index: the bits that scores_out gets
    __shared__ uint32_t s_tag[CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t np = hw::pow2_at_least(n);
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint64_t key = 0;
        uint32_t tag = MS_DEAD << MS_CLASS_SHIFT | j;
        if (j < n) {
            uint64_t bits = RM_NAN_BITS;
            tag = MS_OUTSIDE << MS_CLASS_SHIFT | j;
            if ((uint64_t)rows[j].doc < p.n_docs) {
                bits = p.scores[(size_t)q * p.k_in + j];
                const double score = __longlong_as_double((long long)bits);
                if (score != score) {
                    bits = RM_NAN_BITS;
                    tag = MS_NAN << MS_CLASS_SHIFT | j;
                } else {
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
        if (ms_after(ka, ta, kb, tb) == up) {
            s_key[i] = kb; s_tag[i] = tb;
            s_key[o] = ka; s_tag[o] = ta;
        }
    });
    const uint32_t n_out = hw::page_len(n, p.first, p.k);
    constexpr uint32_t J_MASK = (1u << MS_CLASS_SHIFT) - 1u;
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_tag[p.first + r] & J_MASK; });
    if (p.scores_out)
        for (uint32_t r = tid; r < n_out; r += BLOCK) p.scores_out[(size_t)q * p.k + r] = s_score[s_tag[p.first + r] & J_MASK];
    if (tid == 0) p.n_hits_out[q] = (int32_t)n_out;
}

constexpr int MS_SMALL = 64, MS_SMALL_PER = 2, MS_LARGE = 256, MS_LARGE_PER = 4;
static_assert(MS_LARGE * MS_LARGE_PER >= SS_MAX_TOPK, "k_model_sort_hits holds a whole window in LDS");

// ---- host side -------------------------------------------------------------------------------------------------------------------
// a grow-only block that a refusal may still follow: no device memory is SS_ERR_OOM, and nothing has been enqueued
template <typename T>
int32_t ensure_or_oom(ss_ctx* ctx, const char* entry, ss::DevBuf<T>& b, size_t n) {
    const hipError_t e = ensure(b, n);
    if (e == hipSuccess) return SS_OK;
    (void)hipGetLastError();
    return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %zu bytes of scratch", entry, n * sizeof(T));
}

int32_t create_impl(ss_ctx* ctx, int32_t n_features, const double* linear, double base, int32_t n_trees, const uint32_t* tree_ptr,
                    const ss_tree_node* nodes, ss_rank_model** out) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out) return ctx->fail(SS_ERR_INVALID, "ss_rank_model_create: out is NULL");
    *out = nullptr;
    char msg[256];
    rp::Info info{};
    const int rc = rp::check_model(msg, sizeof(msg), "ss_rank_model_create", n_features, linear, base, n_trees, tree_ptr,
                                   reinterpret_cast<const rp::Node*>(nodes), &info);
    if (rc != rp::OK) return ctx->fail(rc == rp::INVALID ? SS_ERR_INVALID : SS_ERR_UNSUPPORTED, "%s", msg);
    // ---- the model has passed: pack and upload (pageable sources: the copies have left the host arrays when they return)
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<ss_rank_model> m(new ss_rank_model());
    m->ctx = ctx;
    m->info = info;
    m->base = base;
    for (int32_t f = 0; linear && f < n_features; f++) m->has_linear |= linear[f] != 0.0;
    std::vector<rp::PNode> packed(info.n_nodes);
    rp::pack_nodes(reinterpret_cast<const rp::Node*>(nodes), info.n_nodes, packed.data());
    const uint32_t zero = 0;
    SS_HIP(ctx, m->d_linear.alloc((size_t)n_features));
    SS_HIP(ctx, m->d_tree_ptr.alloc((size_t)n_trees + 1));
    SS_HIP(ctx, m->d_nodes.alloc(info.n_nodes));
    if (m->has_linear) SS_HIP(ctx, hipMemcpyAsync(m->d_linear.p, linear, (size_t)n_features * sizeof(double), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipMemcpyAsync(m->d_tree_ptr.p, n_trees ? tree_ptr : &zero, ((size_t)n_trees + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (info.n_nodes) SS_HIP(ctx, hipMemcpyAsync(m->d_nodes.p, packed.data(), packed.size() * sizeof(rp::PNode), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    *out = m.release();
    return SS_OK;
}

int32_t eval_impl(ss_rank_model* m, int64_t n_rows, const double* x, double* scores_out) {
    const char* const entry = "ss_rank_model_eval";
    ss_ctx* ctx = m->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_rows < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_rows < 0", entry);
    if (n_rows >= (int64_t)1 << 31) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: n_rows = %lld, must be below 2^31", entry, (long long)n_rows);
    if (n_rows == 0) return SS_OK;
    if (!x || !scores_out) return ctx->fail(SS_ERR_INVALID, "%s: x or scores_out is NULL", entry);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_rows, nx = n * (size_t)m->info.n_features;
    const bool host_x = !ss::on_device(x), host_out = !ss::on_device(scores_out);
    if (host_x) SS_TRY(ensure_or_oom(ctx, entry, m->d_x, nx));
    if (host_out) SS_TRY(ensure_or_oom(ctx, entry, m->d_out, n));
    if (host_x) SS_HIP(ctx, hipMemcpyAsync(m->d_x.p, x, nx * sizeof(double), hipMemcpyHostToDevice, st));
    double* const d_out = host_out ? m->d_out.p : scores_out;
    launch_forest(m, host_x ? m->d_x.p : x, d_out, n, nullptr, 1, st);
    SS_HIP(ctx, hipGetLastError());
    if (host_out) SS_HIP(ctx, hipMemcpyAsync(scores_out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (host_x || host_out) SS_HIP(ctx, hipStreamSynchronize(st));
    return SS_OK;
}

// The optional arrays of a window, each the caller's when it is device memory, else a part of the scorer's block.
struct OptIn {
    const uint32_t* prox = nullptr;
    const int32_t *vec = nullptr, *qlen = nullptr;
    const void *h_prox = nullptr, *h_vec = nullptr, *h_qlen = nullptr;   // the host arrays still to go up
    size_t prox_bytes = 0, vec_bytes = 0, qlen_bytes = 0;
};
// Step 1, before anything is enqueued: where the arrays are, and the block for those in host memory.
int32_t opt_in_prepare(ss_scorer* s, const char* entry, size_t n_q, size_t k_in, const ss_proximity* prox, const int32_t* vec_scores,
                       const int32_t* query_len, OptIn* o) {
    o->prox = reinterpret_cast<const uint32_t*>(prox);
    o->vec = vec_scores;
    o->qlen = query_len;
    o->prox_bytes = n_q * k_in * sizeof(ss_proximity);
    o->vec_bytes = align16(n_q * k_in * sizeof(int32_t));
    o->qlen_bytes = align16(n_q * sizeof(int32_t));
    if (prox && !ss::on_device(prox)) o->h_prox = prox;
    if (vec_scores && !ss::on_device(vec_scores)) o->h_vec = vec_scores;
    if (query_len && !ss::on_device(query_len)) o->h_qlen = query_len;
    if (o->h_prox || o->h_vec || o->h_qlen) SS_TRY(ensure_or_oom(s->ctx, entry, s->d_rm_in, align16(o->prox_bytes) + o->vec_bytes + o->qlen_bytes));
    return SS_OK;
}
// Step 2: the host arrays up.  *staged is set when one went: the call waits before it returns.
int32_t opt_in_stage(ss_scorer* s, size_t n_q, size_t k_in, OptIn* o, bool* staged) {
    ss_ctx* ctx = s->ctx;
    unsigned char* const b = s->d_rm_in.p;
    unsigned char* const b_vec = b + align16(o->prox_bytes);
    unsigned char* const b_qlen = b_vec + o->vec_bytes;
    if (o->h_prox) {
        SS_HIP(ctx, hipMemcpyAsync(b, o->h_prox, o->prox_bytes, hipMemcpyHostToDevice, ctx->stream));
        o->prox = reinterpret_cast<const uint32_t*>(b);
    }
    if (o->h_vec) {
        SS_HIP(ctx, hipMemcpyAsync(b_vec, o->h_vec, n_q * k_in * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        o->vec = reinterpret_cast<const int32_t*>(b_vec);
    }
    if (o->h_qlen) {
        SS_HIP(ctx, hipMemcpyAsync(b_qlen, o->h_qlen, n_q * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        o->qlen = reinterpret_cast<const int32_t*>(b_qlen);
    }
    *staged |= o->h_prox || o->h_vec || o->h_qlen;
    return SS_OK;
}

// k_hit_features over rows, counts and optional arrays in device memory
void launch_features(ss_scorer* s, size_t n_q, size_t k_in, const ss_hit* d_hits, const int32_t* d_n_hits, const OptIn& o, double* d_out, hipStream_t st) {
    HitFeatParams p{};
    p.hits = d_hits;
    p.n_hits = d_n_hits;
    p.prox = o.prox;
    p.vec_scores = o.vec;
    p.query_len = o.qlen;
    p.fields = s->fields.p;
    p.n_docs = s->n_docs;
    p.out = reinterpret_cast<uint64_t*>(d_out);
    p.k_in = (uint32_t)k_in;
    p.n_fields = (uint32_t)s->n_fields;
    p.total = n_q * k_in;
    hipLaunchKernelGGL(k_hit_features, dim3((unsigned)((p.total + HF_TPB - 1) / HF_TPB)), dim3(HF_TPB), 0, st, p);   // (n_q * k_in < 2^31)
}

int32_t features_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, const ss_proximity* prox,
                      const int32_t* vec_scores, const int32_t* query_len, double* out) {
    const char* const entry = "ss_hit_features";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_q < 0", entry);
    if (k_in < 1) return ctx->fail(SS_ERR_INVALID, "%s: k_in = %d must be >= 1", entry, k_in);
    if (k_in > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: k_in = %d exceeds SS_MAX_TOPK = %d", entry, k_in, SS_MAX_TOPK);
    if ((uint64_t)n_q * (uint64_t)k_in >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "%s: n_q * k_in = %llu entries, must be below 2^31", entry, (unsigned long long)((uint64_t)n_q * (uint64_t)k_in));
    if (n_q > 0 && (!hits || !n_hits || !out)) return ctx->fail(SS_ERR_INVALID, "%s: hits, n_hits or out is NULL", entry);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, entry, "k_in", n_q, k_in, hits, n_hits, &w));
    OptIn oi;
    SS_TRY(opt_in_prepare(s, entry, (size_t)n_q, (size_t)k_in, prox, vec_scores, query_len, &oi));
    SS_TRY(hw::window_stage(s, &w));
    SS_TRY(opt_in_stage(s, (size_t)n_q, (size_t)k_in, &oi, &w.staged));
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, out, (size_t)n_q * (size_t)k_in * NF * sizeof(double), &o));
    launch_features(s, (size_t)n_q, (size_t)k_in, w.hits, w.n_hits, oi, static_cast<double*>(o.dev), ctx->stream);
    SS_HIP(ctx, hipGetLastError());
    return hw::entries_out_finish(s, o, w, sizeof(double), NF);
}

int32_t rerank_impl(ss_scorer* s, ss_rank_model* m, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, const ss_proximity* prox,
                    const int32_t* vec_scores, const int32_t* query_len, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out,
                    double* scores_out) {
    const char* const entry = "ss_rerank_hits_by_model";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (!m) return ctx->fail(SS_ERR_INVALID, "%s: the model is NULL", entry);
    if (m->ctx != ctx) return ctx->fail(SS_ERR_INVALID, "%s: the model belongs to another context", entry);
    if (m->info.n_features != SS_RANK_N_FEATURES)
        return ctx->fail(SS_ERR_INVALID, "%s: the model reads %d features, ss_hit_features has %d", entry, m->info.n_features, SS_RANK_N_FEATURES);
    SS_TRY(hw::check_paging(ctx, entry, "k_in", n_q, k_in, k, first));
    SS_TRY(hw::check_page_arrays(ctx, entry, n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, entry, "k_in", n_q, k_in, hits, n_hits, &w));
    const size_t nq = (size_t)n_q, kin = (size_t)k_in, n_rows = nq * kin;
    SS_TRY(ensure_or_oom(ctx, entry, s->d_rm_feat, n_rows * NF));
    SS_TRY(ensure_or_oom(ctx, entry, s->d_rm_scores, n_rows));
    OptIn oi;
    SS_TRY(opt_in_prepare(s, entry, nq, kin, prox, vec_scores, query_len, &oi));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, nq, (size_t)k, hits_out, n_hits_out, nullptr, scores_out, sizeof(double), &o));
    // ---- the pipeline
    SS_TRY(hw::window_stage(s, &w));
    SS_TRY(opt_in_stage(s, nq, kin, &oi, &w.staged));
    launch_features(s, nq, kin, w.hits, w.n_hits, oi, s->d_rm_feat.p, st);
    SS_HIP(ctx, hipGetLastError());
    launch_forest(m, s->d_rm_feat.p, s->d_rm_scores.p, n_rows, w.n_hits, (uint32_t)k_in, st);
    SS_HIP(ctx, hipGetLastError());
    ModelSortParams p{};
    p.scores = reinterpret_cast<const uint64_t*>(s->d_rm_scores.p);
    p.n_docs = s->n_docs;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.scores_out = static_cast<uint64_t*>(o.extra);
    p.k_in = (uint32_t)k_in; p.first = (uint32_t)first; p.k = (uint32_t)k;
    if (k_in <= MS_SMALL * MS_SMALL_PER)
        hipLaunchKernelGGL((k_model_sort_hits<MS_SMALL, MS_SMALL_PER>), dim3((unsigned)n_q), dim3(MS_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_model_sort_hits<MS_LARGE, MS_LARGE_PER>), dim3((unsigned)n_q), dim3(MS_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    return hw::rows_out_finish(s, o, w.staged);
}

}  // namespace

extern "C" {

int32_t ss_rank_model_create(ss_ctx* ctx, int32_t n_features, const double* linear, double base, int32_t n_trees, const uint32_t* tree_ptr,
                             const ss_tree_node* nodes, ss_rank_model** out) {
    if (!ctx) return SS_ERR_INVALID;
    return hw::guarded(ctx, "ss_rank_model_create", [&] { return create_impl(ctx, n_features, linear, base, n_trees, tree_ptr, nodes, out); });
}

int32_t ss_rank_model_destroy(ss_rank_model* m) {
    if (!m) return SS_ERR_INVALID;
    ss_ctx* ctx = m->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete m;
    return SS_OK;
}

int32_t ss_rank_model_get_info(ss_rank_model* m, ss_rank_model_info* out) {
    if (!m) return SS_ERR_INVALID;
    if (!out) return m->ctx->fail(SS_ERR_INVALID, "ss_rank_model_get_info: out is NULL");
    *out = ss_rank_model_info{m->info.n_features, m->info.n_trees, m->info.n_nodes, m->info.max_tree_nodes, m->info.max_depth, 0u};
    return SS_OK;
}

int32_t ss_rank_model_eval(ss_rank_model* m, int64_t n_rows, const double* x, double* scores_out) {
    if (!m) return SS_ERR_INVALID;
    return hw::guarded(m->ctx, "ss_rank_model_eval", [&] { return eval_impl(m, n_rows, x, scores_out); });
}

int32_t ss_hit_features(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, const ss_proximity* prox,
                        const int32_t* vec_scores, const int32_t* query_len, double* out) {
    return hw::guarded(s, "ss_hit_features", [&] { return features_impl(s, n_q, k_in, hits, n_hits, prox, vec_scores, query_len, out); });
}

int32_t ss_rerank_hits_by_model(ss_scorer* s, ss_rank_model* m, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits,
                                const ss_proximity* prox, const int32_t* vec_scores, const int32_t* query_len, int32_t first, int32_t k,
                                ss_hit* hits_out, int32_t* n_hits_out, double* scores_out) {
    return hw::guarded(s, "ss_rerank_hits_by_model", [&] {
        return rerank_impl(s, m, n_q, k_in, hits, n_hits, prox, vec_scores, query_len, first, k, hits_out, n_hits_out, scores_out);
    });
}

}  // extern "C"
