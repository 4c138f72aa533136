// vector.hip — ss_scorer_set_doc_vectors, ss_vector_topk, ss_hit_vector_scores and ss_rerank_hits_by_vector: one signed 8-bit vector per
// doc, the exact top k of every query vector by 32-bit integer dot product, and a result window re-ordered by it.
//
//   k_vec_topk          grid (chunk of docs, block of 16 / 32 / 64 queries), four waves.  The block's query vectors sit in LDS for the
//                       whole chunk; a wave takes a tile of 64 docs per round, loads its rows straight from memory as the A operand of
//                       __builtin_amdgcn_mfma_i32_16x16x64_i8 (16 docs x 64 bytes per instruction, 16 bytes per lane) and multiplies
//                       them with every 16-query B tile read from LDS: 4 x QT accumulators of 4 registers.  Both operands are loaded
//                       by the same rule — lane l holds bytes 16 (l >> 4) .. + 15 of the 64-byte k step of row l & 15 — so whatever
//                       order the instruction gives the 64 k positions inside a step, byte i of a doc meets byte i of the query.  The
//                       C/D map (column = l & 15, row = 4 (l >> 4) + register) puts one query per lane and tile.
//                       A score becomes the key ((uint32)score ^ 0x80000000) << 32 | (0xFFFFFFFF - doc): descending key order is score
//                       descending, doc ascending, and a key names its doc, so no order of arrival matters.  A lane compares its keys
//                       with the query's threshold in LDS straight from the accumulator; survivors whose doc is valid (inside the
//                       chunk and in the query's allow-list: one 64-bit word per wave, query and round) are appended to the query's LDS
//                       list.  A list that could overflow in the next round is cut back to its k largest keys by an exact radix
//                       select (8 digits of 8 bits, LDS histogram) and the k-th key becomes the threshold.  A wave whose 64 docs no
//                       query of the block may take skips the loads and the product.  The chunk's <= k keys per query go to the
//                       partial lists, unused slots as 0 (no key is 0).
//   k_vec_merge         one workgroup per query: the k-th largest key over the chunks' lists by the same select, the keys at or above
//                       it sorted in LDS (bitonic, <= 1024), rows and count written.
//   k_vec_hit_scores    a gather: 16 lanes per (query, row) pair, 16 bytes per lane and step, summed over the group.
//   k_vec_sort_hits     k_sort_hits_by_field's network over (class, key, window index) with the key taken from the scores
//                       k_vec_hit_scores wrote: written anew here so that field.hip's calls enqueue what they did.
// No float anywhere.  Device arrays throughout: the calls only enqueue on the context's stream.  ss_hit_vector_scores /
// ss_rerank_hits_by_vector: the window in, the paging checks and the outputs' way back are hit_window.hpp's.
#include "hit_window.hpp"
#include "vector_device.hpp"
#include "vector_plan.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

using ss::vecdev::VT_TILE;
using ss::vecdev::VT_WAVES;
using ss::vecdev::VT_TPB;
using ss::vecdev::VM_TPB;
using ss::vecdev::v4i;
using ss::vecdev::vec_key;
using ss::vecdev::vec_compact;
static_assert(SS_MAX_VEC_DIM == ss::vec::MAX_DIM && SS_MAX_TOPK == ss::vec::MAX_K, "vector_plan.hpp states the ABI's limits");
static_assert(sizeof(ss_vec_hit) == 8, "a row is one 8-byte word");

struct VecTopkParams {
    const int8_t* vec;                 // [n_docs][dim]
    uint64_t n_docs;
    const int8_t* qvec;                // [n_q][dim], 16-byte aligned
    const int32_t* q_mask;             // [n_q] or nullptr: every query -1
    const uint32_t* masks;             // the scorer's allow-lists [n_masks][mask_words]
    uint64_t mask_words;
    uint64_t* part;                    // [n_q][n_chunks][k]
    uint32_t dim, n_q, k, chunk_docs, n_chunks, cap, row_stride;
};

template <int QT>
__global__ __launch_bounds__(VT_TPB) void k_vec_topk(VecTopkParams p) {
    constexpr uint32_t QB = QT * 16;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const s_q = smem;                                              // [QB][row_stride]
    uint64_t* const s_buf = reinterpret_cast<uint64_t*>(smem + (size_t)QB * p.row_stride);   // [QB][cap]
    uint64_t* const s_thr = s_buf + (size_t)QB * p.cap;                           // [QB]
    uint64_t* const s_mw = s_thr + QB;                                            // [VT_WAVES][QB]
    uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_mw + VT_WAVES * QB);       // [QB]
    uint32_t* const s_hist = s_cnt + QB;                                          // [256]
    uint32_t* const s_sel = s_hist + 256;                                         // [16]: select's bin and count, compaction's counters, [4 .. 6] = the 'a list is nearly full' flags
    uint16_t* const s_holes = reinterpret_cast<uint16_t*>(s_sel + 16);            // [HOLES]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = lane & 15u, h = lane >> 4;
    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * QB;
    const uint64_t c_begin = (uint64_t)chunk * p.chunk_docs;
    const uint64_t c_end = c_begin + p.chunk_docs < p.n_docs ? c_begin + p.chunk_docs : p.n_docs;   // > c_begin: the launcher's grid
    const uint32_t n_tiles = (uint32_t)((c_end - c_begin + VT_TILE - 1) / VT_TILE);
    const uint32_t n_rounds = (n_tiles + VT_WAVES - 1) / VT_WAVES;
    const uint32_t k = p.k, cap = p.cap, dim = p.dim;
    const bool tight = cap < k + VT_WAVES * VT_TILE;                                    // a list cannot take a whole round: checked before every 16-doc step
    const uint32_t inc = tight ? VT_TILE : VT_WAVES * VT_TILE;                             // what one query can gain between two checks
    // ---- the block's queries into LDS (rows past n_q: zeros, never a candidate), lists empty, thresholds 0 (below every key)
    const uint32_t row_chunks = dim / 16;
    for (uint32_t x = tid; x < QB * row_chunks; x += VT_TPB) {
        const uint32_t row = x / row_chunks, c = x - row * row_chunks;
        v4i v = {0, 0, 0, 0};
        if (q0 + row < p.n_q) v = *reinterpret_cast<const v4i*>(p.qvec + (size_t)(q0 + row) * dim + (size_t)c * 16);
        *reinterpret_cast<v4i*>(s_q + (size_t)row * p.row_stride + (size_t)c * 16) = v;
    }
    if (tid < QB) { s_thr[tid] = 0; s_cnt[tid] = 0; }
    if (tid < 3) s_sel[4 + tid] = 0;
    uint32_t chk = 0;                                                             // checks so far
    int32_t mid = -1;                                                             // lane l < QB: query q0 + l's allow-list
    const bool q_live = lane < QB && q0 + lane < p.n_q;
    if (q_live && p.q_mask) mid = p.q_mask[q0 + lane];
    __syncthreads();
    for (uint32_t round = 0; round < n_rounds; round++) {
        const uint32_t tile = round * VT_WAVES + wave;
        const uint64_t d0 = c_begin + (uint64_t)tile * VT_TILE;                      // a multiple of 64
        // ---- which of the wave's 64 docs each query may take
        uint64_t w = 0;
        if (q_live && tile < n_tiles) {
            const uint64_t left = c_end - d0;
            w = left >= 64 ? ~0ull : (1ull << left) - 1ull;
            if (mid >= 0) {
                const uint64_t wi = d0 >> 5;                                      // < mask_words
                const uint32_t* const m = p.masks + (uint64_t)mid * p.mask_words;
                const uint64_t lo = m[wi], hi = wi + 1 < p.mask_words ? m[wi + 1] : 0u;
                w &= lo | hi << 32;
            }
        }
        if (lane < QB) s_mw[wave * QB + lane] = w;
        const bool any = __ballot(w != 0) != 0;
        v4i acc[4][QT];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int j = 0; j < QT; j++) acc[t][j] = v4i{0, 0, 0, 0};
        if (any) {
            const int8_t* a_ptr[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                uint64_t d = d0 + (uint64_t)t * 16 + r;
                if (d >= p.n_docs) d = p.n_docs - 1;                              // (its bit in w is 0)
                a_ptr[t] = p.vec + d * dim + h * 16;
            }
            const unsigned char* const b_ptr = s_q + (size_t)r * p.row_stride + h * 16;
            for (uint32_t ks = 0; ks < dim; ks += 64) {
                v4i a[4];
#pragma unroll
                for (int t = 0; t < 4; t++) a[t] = *reinterpret_cast<const v4i*>(a_ptr[t] + ks);
#pragma unroll
                for (int j = 0; j < QT; j++) {
                    const v4i b = *reinterpret_cast<const v4i*>(b_ptr + (size_t)j * 16 * p.row_stride + ks);
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b, acc[t][j], 0, 0, 0);
                }
            }
        }
        // ---- candidates: accumulator register g of tile (t, j) is doc d0 + 16 t + 4 h + g under query j * 16 + r
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (tight || t == 0) {
                // Check number chk reads flag chk % 3, the appends behind it raise flag (chk + 1) % 3, and thread 0 clears flag
                // (chk + 2) % 3 — read at the check before, raised again only behind the next one — so no thread can see a flag
                // change between the barrier and its own read: the branch is uniform.
                __syncthreads();                                                  // (the valid words and every earlier append stand)
                const bool full = s_sel[4 + chk % 3] != 0;
                if (tid == 0) s_sel[4 + (chk + 2) % 3] = 0;
                chk++;
                if (full) {
                    for (uint32_t ql = 0; ql < QB; ql++) {
                        const uint32_t n = s_cnt[ql];
                        if (n + inc > cap) vec_compact(s_buf + (size_t)ql * cap, n, k, &s_thr[ql], &s_cnt[ql], s_hist, s_sel, s_holes);
                    }
                }
            }
            if (any) {
#pragma unroll
                for (int j = 0; j < QT; j++) {
                    const uint32_t ql = (uint32_t)j * 16 + r;
                    const uint32_t bits = (uint32_t)(s_mw[wave * QB + ql] >> (t * 16 + h * 4)) & 15u;
                    if (bits) {
                        const uint64_t thr = s_thr[ql];
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const uint64_t key = vec_key(acc[t][j][g], (uint32_t)(d0 + (uint32_t)(t * 16 + h * 4 + g)));
                            if ((bits >> g & 1u) && key > thr) {
                                const uint32_t pos = atomicAdd(&s_cnt[ql], 1u);   // < cap: cnt + inc <= cap stood at the last check
                                s_buf[(size_t)ql * cap + pos] = key;
                                if (pos + 1 + inc > cap) s_sel[4 + chk % 3] = 1;
                            }
                        }
                    }
                }
            }
        }
    }
    // ---- the chunk's lists: at most k keys per query, the other slots 0
    __syncthreads();
    for (uint32_t ql = 0; ql < QB; ql++) {
        if (q0 + ql >= p.n_q) break;                                              // (uniform)
        uint32_t n = s_cnt[ql];
        if (n > k) {
            vec_compact(s_buf + (size_t)ql * cap, n, k, &s_thr[ql], &s_cnt[ql], s_hist, s_sel, s_holes);
            n = k;
        }
        uint64_t* const out = p.part + ((uint64_t)(q0 + ql) * p.n_chunks + chunk) * k;
        for (uint32_t i = tid; i < k; i += VT_TPB) out[i] = i < n ? s_buf[(size_t)ql * cap + i] : 0ull;
    }
}

struct VecMergeParams {
    const uint64_t* part;              // [n_q][n_slots]
    uint32_t n_slots, k;               // n_slots = n_chunks * k
    ss_vec_hit* hits_out;              // [n_q][k]
    int32_t* n_hits_out;               // [n_q]
};

__global__ __launch_bounds__(VM_TPB) void k_vec_merge(VecMergeParams p) {
    __shared__ uint64_t s_key[SS_MAX_TOPK];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[4];
    const uint32_t q = blockIdx.x;
    ss::vecdev::vec_merge_query(p.part + (uint64_t)q * p.n_slots, p.n_slots, p.k, p.hits_out + (size_t)q * p.k, p.n_hits_out + q, s_key, s_hist, s_sel);
}

// ---- scores of given rows ----------------------------------------------------------------------------------------------------
struct VecScoreParams {
    const int8_t* vec;
    uint64_t n_docs;
    const int8_t* qvec;                // 16-byte aligned
    const ss_hit* hits;                // [n_q][k_in]
    const int32_t* n_hits;
    int32_t* out;                      // [n_q][k_in]
    uint32_t dim, k_in;
    uint64_t total;                    // n_q * k_in
};

__global__ __launch_bounds__(256) void k_vec_hit_scores(VecScoreParams p) {
    const uint64_t pair = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (pair >= p.total) return;                                                  // (a whole group of 16)
    const uint64_t q = pair / p.k_in;
    const uint32_t j = (uint32_t)(pair - q * p.k_in);
    if (j >= hw::window_len(p.n_hits[q], p.k_in)) return;
    const uint32_t d = p.hits[pair].doc;
    if ((uint64_t)d >= p.n_docs) {
        if (sub == 0) p.out[pair] = SS_NO_VEC_SCORE;
        return;
    }
    const int8_t* const a = p.vec + (uint64_t)d * p.dim;
    const int8_t* const b = p.qvec + q * p.dim;
    int32_t sum = 0;
    for (uint32_t c = sub * 16; c < p.dim; c += 256) {
        const v4i x = *reinterpret_cast<const v4i*>(a + c), y = *reinterpret_cast<const v4i*>(b + c);
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int s = 0; s < 32; s += 8) sum += (int32_t)(int8_t)((uint32_t)x[w] >> s) * (int32_t)(int8_t)((uint32_t)y[w] >> s);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
    if (sub == 0) p.out[pair] = sum;
}

// ---- a window sorted by its scores -------------------------------------------------------------------------------------------
constexpr uint32_t VS_CLASS_SHIFT = 16;                   // tag = class << 16 | window index (< SS_MAX_TOPK = 2^10)
constexpr uint32_t VS_OUTSIDE = 1, VS_DEAD = 2;

struct VecSortParams {
    const int32_t* scores;             // [n_q][k_in] from k_vec_hit_scores
    const ss_hit* hits;
    const int32_t* n_hits;
    ss_hit* hits_out;                  // [n_q][k]
    int32_t* n_hits_out;
    int32_t* scores_out;               // [n_q][k], nullable
    uint32_t k_in, first, k;
};

// (class, key, window index) of a behind that of b; the key: the score's bits flipped so that the larger score comes first
__device__ __forceinline__ bool vs_after(uint32_t ka, uint32_t ta, uint32_t kb, uint32_t tb) {
    const uint32_t ca = ta >> VS_CLASS_SHIFT, cb = tb >> VS_CLASS_SHIFT;
    return ca != cb ? ca > cb : ka != kb ? ka > kb : ta > tb;
}

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_vec_sort_hits(VecSortParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    __shared__ uint32_t s_key[CAP];
    __shared__ uint32_t s_tag[CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t np = hw::pow2_at_least(n);
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint32_t key = 0, tag = VS_DEAD << VS_CLASS_SHIFT | j;
        if (j < n) {
            const int32_t sc = p.scores[(size_t)q * p.k_in + j];
            tag = VS_OUTSIDE << VS_CLASS_SHIFT | j;
            if (sc != SS_NO_VEC_SCORE) {                                          // (never a real score)
                key = ~((uint32_t)sc ^ 0x80000000u);
                tag = j;
            }
        }
        s_key[j] = key;
        s_tag[j] = tag;
    }
    __syncthreads();
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint32_t ka = s_key[i], kb = s_key[o], ta = s_tag[i], tb = s_tag[o];
        if (vs_after(ka, ta, kb, tb) == up) {
            s_key[i] = kb; s_tag[i] = tb;
            s_key[o] = ka; s_tag[o] = ta;
        }
    });
    // ---- the page: sorted positions [first, first + n_out), all below n
    const uint32_t n_out = hw::page_len(n, p.first, p.k);
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_tag[p.first + r] & ((1u << VS_CLASS_SHIFT) - 1u); });
    if (p.scores_out)
        for (uint32_t rr = tid; rr < n_out; rr += BLOCK) {
            const uint32_t tag = s_tag[p.first + rr];
            p.scores_out[(size_t)q * p.k + rr] = tag >> VS_CLASS_SHIFT ? SS_NO_VEC_SCORE : (int32_t)(~s_key[p.first + rr] ^ 0x80000000u);
        }
    if (tid == 0) p.n_hits_out[q] = (int32_t)n_out;
}

constexpr int VS_SMALL = 64, VS_SMALL_PER = 2, VS_LARGE = 256, VS_LARGE_PER = 4;
static_assert(VS_LARGE * VS_LARGE_PER >= SS_MAX_TOPK, "k_vec_sort_hits holds a whole window in LDS");

// ---- host side -------------------------------------------------------------------------------------------------------------
// the query vectors on the device, 16-byte aligned (the kernels load them 16 bytes at a time): the caller's array when it is such,
// otherwise a copy in a block the scorer owns (*staged: from host memory, so the call waits before it returns)
int32_t qvec_to_device(ss_scorer* s, const int8_t* qvec, size_t bytes, const int8_t** out, bool* staged) {
    ss_ctx* ctx = s->ctx;
    const bool dev = ss::on_device(qvec);
    if (dev && ((uintptr_t)qvec & 15u) == 0) { *out = qvec; return SS_OK; }
    SS_HIP(ctx, ensure(s->d_vec_q, bytes));
    SS_HIP(ctx, hipMemcpyAsync(s->d_vec_q.p, qvec, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    *out = s->d_vec_q.p;
    if (!dev) *staged = true;
    return SS_OK;
}

template <int QT>
int32_t launch_topk(ss_scorer* s, const VecTopkParams& p, const ss::vec::Plan& pl, hipStream_t st) {
    ss_ctx* ctx = s->ctx;
    if (s->vec_lds_attr[QT] < (int)pl.lds_bytes) {
        SS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vec_topk<QT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
        s->vec_lds_attr[QT] = (int)pl.lds_bytes;
    }
    hipLaunchKernelGGL((k_vec_topk<QT>), dim3(pl.n_chunks, pl.n_qblocks), dim3(VT_TPB), pl.lds_bytes, st, p);
    return SS_OK;
}

// k_vec_topk and k_vec_merge over the table [n_rows > 0][dim]: p carries the queries and their masks, the rest is filled in here
int32_t enqueue_topk(ss_scorer* s, const char* who, const int8_t* table, uint64_t n_rows, VecTopkParams p, const ss::vec::Plan& pl, uint32_t n_q,
                     uint32_t k, ss_vec_hit* o_hits, int32_t* o_n) {
    ss_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    {
        const hipError_t e = ensure(s->d_vec_part, (size_t)pl.part_keys);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %llu partial keys", who,
                             (unsigned long long)pl.part_keys);
        }
    }
    p.vec = table;
    p.n_docs = n_rows;
    p.masks = s->masks.p;
    p.mask_words = s->mask_words;
    p.part = s->d_vec_part.p;
    p.dim = (uint32_t)s->vec_dim; p.n_q = n_q; p.k = k;
    p.chunk_docs = pl.chunk_docs; p.n_chunks = pl.n_chunks; p.cap = pl.cap; p.row_stride = pl.row_stride;
    if (pl.q_block == 64) SS_TRY(launch_topk<4>(s, p, pl, st));
    else if (pl.q_block == 32) SS_TRY(launch_topk<2>(s, p, pl, st));
    else SS_TRY(launch_topk<1>(s, p, pl, st));
    SS_HIP(ctx, hipGetLastError());
    VecMergeParams m{};
    m.part = s->d_vec_part.p;
    m.n_slots = pl.n_chunks * k;
    m.k = k;
    m.hits_out = o_hits;
    m.n_hits_out = o_n;
    hipLaunchKernelGGL(k_vec_merge, dim3((unsigned)n_q), dim3(VM_TPB), 0, st, m);
    SS_HIP(ctx, hipGetLastError());
    return SS_OK;
}

int32_t topk_impl(ss_scorer* s, int32_t n_q, const int8_t* qvec, const int32_t* mask_id, int32_t k, ss_vec_hit* hits_out, int32_t* n_hits_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "ss_vector_topk: n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_vector_topk: k = %d must be >= 1", k);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_vector_topk: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
    if (n_q > 0 && (!qvec || !hits_out || !n_hits_out)) return ctx->fail(SS_ERR_INVALID, "ss_vector_topk: qvec, hits_out or n_hits_out is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    std::vector<int32_t> mid;
    bool masked = false;
    if (mask_id && nq) {
        mid.resize(nq);
        SS_HIP(ctx, ss::copy_in(ctx->stream, mid.data(), mask_id, nq * sizeof(int32_t)));
        for (size_t q = 0; q < nq; q++) {
            if (mid[q] < -1 || mid[q] >= s->n_masks)
                return ctx->fail(SS_ERR_INVALID, "ss_vector_topk: query %zu has mask id %d (the scorer has %d masks)", q, mid[q], s->n_masks);
            masked |= mid[q] >= 0;
        }
    }
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_vector_topk: no vector table registered (ss_scorer_set_doc_vectors)");
    if (n_q == 0) return SS_OK;
    int lds_limit = 0;
    SS_HIP(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const ss::vec::Plan pl = ss::vec::plan(s->n_docs, (uint32_t)s->vec_dim, nq, (uint32_t)k, ctx->opt("vec.chunk_docs", 0), (uint32_t)ctx->cu_count,
                                           (uint32_t)std::min(lds_limit, 160 << 10));
    if (pl.too_large) return ctx->fail(SS_ERR_OOM, "ss_vector_topk: the partial lists of %zu queries over %u chunks do not fit", nq, pl.n_chunks);
    if (!pl.ok)
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_vector_topk: %zu queries at k = %d and dim %d need more than the device's %d bytes of LDS or 65535 query blocks",
                         nq, k, s->vec_dim, lds_limit);
    hipStream_t st = ctx->stream;
    const bool dev_h = ss::on_device(hits_out), dev_n = ss::on_device(n_hits_out);
    if (!dev_h) SS_HIP(ctx, ensure(s->d_vec_hits, nq * (size_t)k));
    if (!dev_n) SS_HIP(ctx, ensure(s->d_vec_n, nq));
    ss_vec_hit* const o_hits = dev_h ? hits_out : s->d_vec_hits.p;
    int32_t* const o_n = dev_n ? n_hits_out : s->d_vec_n.p;
    bool staged = false;
    if (pl.n_chunks == 0 || (masked && s->mask_words == 0)) {                     // a scorer without docs: every row is empty
        SS_HIP(ctx, hipMemsetAsync(o_n, 0, nq * sizeof(int32_t), st));
    } else {
        VecTopkParams p{};
        SS_TRY(qvec_to_device(s, qvec, nq * (size_t)s->vec_dim, &p.qvec, &staged));
        if (masked) {                                                             // the ids go up through a pinned block; its last reader is waited for first
            if (ss::on_device(mask_id)) p.q_mask = mask_id;
            else {
                SS_HIP(ctx, s->ev_vec_mid.wait());
                SS_HIP(ctx, s->h_vec_mid.ensure(nq * sizeof(int32_t)));
                SS_HIP(ctx, ensure(s->d_vec_mid, nq));
                std::memcpy(s->h_vec_mid.p, mid.data(), nq * sizeof(int32_t));
                SS_HIP(ctx, hipMemcpyAsync(s->d_vec_mid.p, s->h_vec_mid.p, nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
                SS_HIP(ctx, s->ev_vec_mid.record(st));
                p.q_mask = s->d_vec_mid.p;
            }
        }
        SS_TRY(enqueue_topk(s, "ss_vector_topk", s->vec.p, s->n_docs, p, pl, (uint32_t)n_q, (uint32_t)k, o_hits, o_n));
    }
    if (dev_h && dev_n) {
        if (staged) SS_HIP(ctx, hipStreamSynchronize(st));
        return SS_OK;                                     // ordered on the ctx stream; nothing comes back
    }
    // ---- host outputs: the counts whole, of the rows exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq);
    std::vector<ss_vec_hit> h_rows;
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), o_n, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_h) {
        h_rows.resize(nq * (size_t)k);
        SS_HIP(ctx, hipMemcpyAsync(h_rows.data(), o_hits, nq * (size_t)k * sizeof(ss_vec_hit), hipMemcpyDeviceToHost, st));
    }
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_hits_out, h_n.data(), nq * sizeof(int32_t));
    if (!dev_h)
        for (size_t q = 0; q < nq; q++)
            std::memcpy(hits_out + q * (size_t)k, h_rows.data() + q * (size_t)k, (size_t)h_n[q] * sizeof(ss_vec_hit));
    return SS_OK;
}

void launch_hit_scores(ss_scorer* s, const int8_t* qvec, const hw::WindowIn& w, int32_t n_q, int32_t k_in, int32_t* out, hipStream_t st) {
    VecScoreParams p{};
    p.vec = s->vec.p;
    p.n_docs = s->n_docs;
    p.qvec = qvec;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.out = out;
    p.dim = (uint32_t)s->vec_dim;
    p.k_in = (uint32_t)k_in;
    p.total = (uint64_t)n_q * (uint64_t)k_in;
    hipLaunchKernelGGL(k_vec_hit_scores, dim3((unsigned)((p.total * 16 + 255) / 256)), dim3(256), 0, st, p);
}

int32_t hit_scores_impl(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t* scores_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "ss_hit_vector_scores: n_q < 0");
    if (k_in < 1) return ctx->fail(SS_ERR_INVALID, "ss_hit_vector_scores: k_in = %d must be >= 1", k_in);
    if (k_in > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_hit_vector_scores: k_in = %d exceeds SS_MAX_TOPK = %d", k_in, SS_MAX_TOPK);
    if (n_q > 0 && (!qvec || !hits || !n_hits || !scores_out))
        return ctx->fail(SS_ERR_INVALID, "ss_hit_vector_scores: qvec, hits, n_hits or scores_out is NULL");
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_hit_vector_scores: no vector table registered (ss_scorer_set_doc_vectors)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_hit_vector_scores", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const int8_t* d_q = nullptr;
    SS_TRY(qvec_to_device(s, qvec, (size_t)n_q * (size_t)s->vec_dim, &d_q, &w.staged));
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, scores_out, (size_t)n_q * (size_t)k_in * sizeof(int32_t), &o));
    launch_hit_scores(s, d_q, w, n_q, k_in, static_cast<int32_t*>(o.dev), st);
    SS_HIP(ctx, hipGetLastError());
    return hw::entries_out_finish(s, o, w, sizeof(int32_t));
}

int32_t rerank_impl(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t first, int32_t k,
                    ss_hit* hits_out, int32_t* n_hits_out, int32_t* scores_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, "ss_rerank_hits_by_vector", "k_in", n_q, k_in, k, first));
    if (n_q > 0 && !qvec) return ctx->fail(SS_ERR_INVALID, "ss_rerank_hits_by_vector: qvec is NULL");
    SS_TRY(hw::check_page_arrays(ctx, "ss_rerank_hits_by_vector", n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "ss_rerank_hits_by_vector: no vector table registered (ss_scorer_set_doc_vectors)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_rerank_hits_by_vector", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const int8_t* d_q = nullptr;
    SS_TRY(qvec_to_device(s, qvec, (size_t)n_q * (size_t)s->vec_dim, &d_q, &w.staged));
    SS_HIP(ctx, ensure(s->d_vec_scores, (size_t)n_q * (size_t)k_in));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)n_q, (size_t)k, hits_out, n_hits_out, nullptr, scores_out, sizeof(int32_t), &o));
    launch_hit_scores(s, d_q, w, n_q, k_in, s->d_vec_scores.p, st);
    SS_HIP(ctx, hipGetLastError());
    ss::launch_vec_sort_hits(s->d_vec_scores.p, w.hits, w.n_hits, n_q, k_in, first, k, o.hits, o.n_hits, static_cast<int32_t*>(o.extra), st);
    SS_HIP(ctx, hipGetLastError());
    return hw::rows_out_finish(s, o, w.staged);
}

}  // namespace

// for maxsim.hip (scorer.hpp): the launch of k_vec_sort_hits as ss_rerank_hits_by_vector uses it
void ss::launch_vec_sort_hits(const int32_t* d_scores, const ss_hit* d_hits, const int32_t* d_n_hits, int32_t n_q, int32_t k_in, int32_t first,
                              int32_t k, ss_hit* d_hits_out, int32_t* d_n_hits_out, int32_t* d_scores_out, hipStream_t st) {
    VecSortParams p{};
    p.scores = d_scores;
    p.hits = d_hits;
    p.n_hits = d_n_hits;
    p.hits_out = d_hits_out;
    p.n_hits_out = d_n_hits_out;
    p.scores_out = d_scores_out;
    p.k_in = (uint32_t)k_in; p.first = (uint32_t)first; p.k = (uint32_t)k;
    if (k_in <= VS_SMALL * VS_SMALL_PER)
        hipLaunchKernelGGL((k_vec_sort_hits<VS_SMALL, VS_SMALL_PER>), dim3((unsigned)n_q), dim3(VS_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_vec_sort_hits<VS_LARGE, VS_LARGE_PER>), dim3((unsigned)n_q), dim3(VS_LARGE), 0, st, p);
}

// for maxsim_topk.hip (scorer.hpp): the launch of k_vec_merge as ss_vector_topk uses it
void ss::launch_vec_merge(const uint64_t* d_part, uint32_t n_chunks, int32_t n_q, int32_t k, ss_vec_hit* d_hits_out, int32_t* d_n_hits_out,
                          hipStream_t st) {
    VecMergeParams m{};
    m.part = d_part;
    m.n_slots = n_chunks * (uint32_t)k;
    m.k = (uint32_t)k;
    m.hits_out = d_hits_out;
    m.n_hits_out = d_n_hits_out;
    hipLaunchKernelGGL(k_vec_merge, dim3((unsigned)n_q), dim3(VM_TPB), 0, st, m);
}

// for hybrid.hip (scorer.hpp): the staging of the query vectors and the launch of k_vec_hit_scores, both as the calls above use them
int32_t ss::vec_queries_to_device(ss_scorer* s, const int8_t* qvec, size_t bytes, const int8_t** out, bool* staged) {
    return qvec_to_device(s, qvec, bytes, out, staged);
}
void ss::launch_vec_hit_scores(ss_scorer* s, const int8_t* d_qvec, const ss_hit* d_hits, const int32_t* d_n_hits, int32_t n_q, int32_t k_in,
                               int32_t* d_out, hipStream_t st) {
    hw::WindowIn w;
    w.hits = d_hits;
    w.n_hits = d_n_hits;
    launch_hit_scores(s, d_qvec, w, n_q, k_in, d_out, st);
}

// for vector_lists.hip (scorer.hpp): the exact top k of device query vectors over any table of int8 rows, as ss_vector_topk enqueues it
int32_t ss::vec_table_topk(ss_scorer* s, const char* who, const int8_t* table, uint64_t n_rows, int32_t n_q, const int8_t* d_qvec, int32_t k,
                           ss_vec_hit* d_hits, int32_t* d_n_hits) {
    ss_ctx* ctx = s->ctx;
    int lds_limit = 0;
    SS_HIP(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const ss::vec::Plan pl = ss::vec::plan(n_rows, (uint32_t)s->vec_dim, (uint64_t)n_q, (uint32_t)k, 0, (uint32_t)ctx->cu_count,
                                           (uint32_t)std::min(lds_limit, 160 << 10));
    if (pl.too_large) return ctx->fail(SS_ERR_OOM, "%s: the partial lists of %d queries over %u chunks do not fit", who, n_q, pl.n_chunks);
    if (!pl.ok) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: %d queries at k = %d and dim %d need more LDS than the device has or 65535 query blocks", who, n_q, k, s->vec_dim);
    VecTopkParams p{};
    p.qvec = d_qvec;
    return enqueue_topk(s, who, table, n_rows, p, pl, (uint32_t)n_q, (uint32_t)k, d_hits, d_n_hits);
}

extern "C" {

int32_t ss_scorer_set_doc_vectors(ss_scorer* s, int32_t dim, const int8_t* vec) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool clear = dim == 0 || !vec;
    if (!clear && (dim < 64 || dim > SS_MAX_VEC_DIM || dim % 64))
        return ctx->fail(SS_ERR_INVALID, "ss_scorer_set_doc_vectors: dim = %d is not a multiple of 64 in [64, %d]", dim, SS_MAX_VEC_DIM);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    ss::DevBuf<int8_t> nb;
    const size_t n = clear ? 0 : (size_t)dim * (size_t)s->n_docs;
    if (!clear) {
        const hipError_t e = nb.alloc(std::max<size_t>(n, 1));                    // (a failure here leaves the old table in place)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "ss_scorer_set_doc_vectors: no device memory for %zu bytes", n);
        }
    }
    // the scorer's outstanding work may read the old table (the vector kernels on the context's stream): drained, as
    // ss_scorer_set_doc_groups does, before the table is replaced
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    if (clear) {
        ss::vec_lists_drop(s);                                                    // (they describe the old table)
        s->vec.release();
        s->vec_dim = 0;
        return SS_OK;
    }
    if (n) {
        SS_HIP(ctx, hipMemcpyAsync(nb.p, vec, n, hipMemcpyDefault, ctx->stream));
        SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ss::vec_lists_drop(s);
    s->vec = std::move(nb);
    s->vec_dim = dim;
    return SS_OK;
}

int32_t ss_vector_topk(ss_scorer* s, int32_t n_q, const int8_t* qvec, const int32_t* mask_id, int32_t k, ss_vec_hit* hits_out, int32_t* n_hits_out) {
    return hw::guarded(s, "ss_vector_topk", [&] { return topk_impl(s, n_q, qvec, mask_id, k, hits_out, n_hits_out); });
}

int32_t ss_hit_vector_scores(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits,
                             int32_t* scores_out) {
    return hw::guarded(s, "ss_hit_vector_scores", [&] { return hit_scores_impl(s, n_q, qvec, k_in, hits, n_hits, scores_out); });
}

int32_t ss_rerank_hits_by_vector(ss_scorer* s, int32_t n_q, const int8_t* qvec, int32_t k_in, const ss_hit* hits, const int32_t* n_hits,
                                 int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, int32_t* scores_out) {
    return hw::guarded(s, "ss_rerank_hits_by_vector", [&] { return rerank_impl(s, n_q, qvec, k_in, hits, n_hits, first, k, hits_out, n_hits_out, scores_out); });
}

}  // extern "C"
