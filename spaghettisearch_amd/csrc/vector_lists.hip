// vector_lists.hip — ss_scorer_set_vector_lists, ss_vector_assign_lists and ss_vector_topk_probed: the docs of the vector table cut into
// lists around centroids the caller brings, and the exact top k over the docs of the n_probe lists nearest to a query.
//
//   registration        a stable sort of (list, doc) by list, least significant 8-bit digit first: per digit k_vl_hist (one wave per tile
//                       of 2048 docs, LDS histogram), k_vl_scan_u32 (digit-major, tile-minor) and k_vl_scatter (the wave walks its tile 64
//                       docs at a time; a lane's place is its digit's running offset plus the number of lower lanes with that digit, so
//                       docs stay in ascending id inside a list).  k_vl_gather_rows copies the vector rows into that order.  A doc at
//                       SS_NO_LIST sorts behind the last list.
//   probe step          the exact top n_probe over the centroid table: ss::vec_table_topk, i.e. k_vec_topk and k_vec_merge.
//   inversion           k_vl_count (queries per list; per query the first partial slot of every probe rank), k_vl_scan_lists (run begins
//                       and work items per list), k_vl_fill (the runs of (query, rank) pairs).  The order inside a run is arbitrary.
//   k_vec_topk_lists    a fixed grid; a workgroup loops over work items (list, segment, group of up to QB queries that probe the list)
//                       found by bisection in the items' scan.  k_vec_topk's tile, LDS image and candidate lists, with the query rows
//                       gathered by index, the doc rows streamed from the list-major copy, a key's doc read from row_doc[] and the
//                       allow-list bit tested per surviving key.  One partial list of k keys per (query, rank, segment).
//   k_vec_merge_lists   k_vec_merge's body over the slots a query filled.
//   assign              ss::vec_table_topk at k = 1 with the centroids as the table and batches of doc rows as the queries.
#include "hit_window.hpp"
#include "vector_device.hpp"
#include "vector_lists_plan.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;
namespace vl = ss::veclists;
using ss::vecdev::VT_TILE;
using ss::vecdev::VT_WAVES;
using ss::vecdev::VT_TPB;
using ss::vecdev::VM_TPB;
using ss::vecdev::v4i;
using ss::vecdev::vec_key;
using ss::vecdev::vec_compact;
static_assert(SS_MAX_VEC_LISTS == vl::MAX_LISTS, "vector_lists_plan.hpp states the ABI's limit");

// ---- registration: a stable radix sort of the docs by list ---------------------------------------------------------------------
constexpr uint32_t SORT_TILE = 2048;                      // docs of one wave

__global__ __launch_bounds__(256) void k_vl_init(uint32_t* key, uint32_t* val, uint64_t n, uint32_t n_lists) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t raw = key[i];
    key[i] = raw < n_lists ? raw : n_lists;               // (SS_NO_LIST: behind the last list)
    val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(64) void k_vl_hist(const uint32_t* key, uint64_t n, uint32_t shift, uint32_t n_tiles, uint32_t* hist /*[256][n_tiles]*/) {
    __shared__ uint32_t s_hist[256];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    for (uint32_t b = lane; b < 256; b += 64) s_hist[b] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)tile * SORT_TILE, end = begin + SORT_TILE < n ? begin + SORT_TILE : n;
    for (uint64_t i = begin + lane; i < end; i += 64) atomicAdd(&s_hist[key[i] >> shift & 255u], 1u);
    __syncthreads();
    for (uint32_t b = lane; b < 256; b += 64) hist[(uint64_t)b * n_tiles + tile] = s_hist[b];
}

// exclusive scan of a[0 .. n) in place by one workgroup of 1024 threads (the totals fit 32 bits: they count docs)
__global__ __launch_bounds__(1024) void k_vl_scan_u32(uint32_t* a, uint64_t n) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, begin = (uint64_t)tid * per < n ? (uint64_t)tid * per : n, end = begin + per < n ? begin + per : n;
    uint32_t sum = 0;
    for (uint64_t i = begin; i < end; i++) sum += a[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t o = tid >= d ? s_sum[tid - d] : 0u;
        __syncthreads();
        s_sum[tid] += o;
        __syncthreads();
    }
    uint32_t run = s_sum[tid] - sum;
    for (uint64_t i = begin; i < end; i++) {
        const uint32_t v = a[i];
        a[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(64) void k_vl_scatter(const uint32_t* key_in, const uint32_t* val_in, uint32_t* key_out, uint32_t* val_out, uint64_t n,
                                                   uint32_t shift, uint32_t n_tiles, const uint32_t* offs /*[256][n_tiles], scanned*/) {
    __shared__ uint32_t s_off[256];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    for (uint32_t b = lane; b < 256; b += 64) s_off[b] = offs[(uint64_t)b * n_tiles + tile];
    __syncthreads();
    const uint64_t begin = (uint64_t)tile * SORT_TILE, end = begin + SORT_TILE < n ? begin + SORT_TILE : n;
    for (uint64_t i0 = begin; i0 < end; i0 += 64) {                               // (uniform: every lane takes every step)
        const uint64_t i = i0 + lane;
        const bool act = i < end;
        const uint32_t key = act ? key_in[i] : 0u, val = act ? val_in[i] : 0u;
        const uint32_t digit = key >> shift & 255u;
        uint64_t peers = __ballot(act);                                           // the active lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b & 1u) != 0;
            const uint64_t m = __ballot(act && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1ull));
        const uint32_t base = s_off[digit];
        __syncthreads();
        if (act && (peers >> lane) <= 1ull) s_off[digit] = base + (uint32_t)__popcll(peers);   // the highest lane of the digit
        __syncthreads();
        if (act) {
            key_out[base + rank] = key;
            val_out[base + rank] = val;
        }
    }
}

__global__ __launch_bounds__(256) void k_vl_gather_rows(const int8_t* vec, const uint32_t* row_doc, int8_t* out, uint64_t n_rows, uint32_t dim) {
    const uint32_t per = dim / 16;
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t row = x / per;
    if (row >= n_rows) return;
    const uint32_t c = (uint32_t)(x - row * per);
    *reinterpret_cast<v4i*>(out + row * dim + (uint64_t)c * 16) = *reinterpret_cast<const v4i*>(vec + (uint64_t)row_doc[row] * dim + (uint64_t)c * 16);
}

// ---- a call: the inversion of the probes -----------------------------------------------------------------------------------------
struct VlInvertParams {
    const ss_vec_hit* probe;           // [n_q][n_probe]: .doc = the list
    const uint32_t* list_begin;        // [n_lists + 1]
    uint32_t* cnt;                     // [n_lists] queries per list
    uint32_t* q_begin;                 // [n_lists] the list's run in run[]
    uint32_t* cur;                     // [n_lists] fill cursor
    uint32_t* run;                     // [n_q * n_probe] pairs q * n_probe + rank
    uint64_t* item_begin;              // [n_lists + 1]
    uint32_t* slot_base;               // [n_q * n_probe] first partial slot of the pair, inside the query's slots
    uint32_t* n_slots;                 // [n_q]
    uint32_t* probes_out;              // [n_q][n_probe], nullable
    uint64_t seg_rows;
    uint32_t n_probe, n_lists, q_block;
};

__device__ __forceinline__ uint32_t vl_segs(const uint32_t* list_begin, uint32_t l, uint64_t seg_rows) {
    return (uint32_t)(((uint64_t)(list_begin[l + 1] - list_begin[l]) + seg_rows - 1) / seg_rows);
}

// one workgroup of 64 lanes per query; lane i owns ranks 16 i .. 16 i + 15 (n_probe <= 1024)
__global__ __launch_bounds__(64) void k_vl_count(VlInvertParams p) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x, P = p.n_probe;
    uint32_t segs[16], sum = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t r = lane * 16 + (uint32_t)j;
        segs[j] = 0;
        if (r < P) {
            const uint32_t l = p.probe[(uint64_t)q * P + r].doc;                  // < n_lists: a row of the centroid table
            atomicAdd(&p.cnt[l], 1u);
            if (p.probes_out) p.probes_out[(uint64_t)q * P + r] = l;
            segs[j] = vl_segs(p.list_begin, l, p.seg_rows);
        }
        sum += segs[j];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= (uint32_t)d) incl += o;
    }
    uint32_t run = incl - sum;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t r = lane * 16 + (uint32_t)j;
        if (r < P) p.slot_base[(uint64_t)q * P + r] = run;
        run += segs[j];
    }
    if (lane == 63) p.n_slots[q] = incl;
}

// one workgroup of 1024 threads: per list the begin of its run and of its work items (segments x groups of q_block queries)
__global__ __launch_bounds__(1024) void k_vl_scan_lists(VlInvertParams p) {
    __shared__ uint32_t s_q[1024];
    __shared__ uint64_t s_i[1024];
    const uint32_t tid = threadIdx.x, per = (p.n_lists + 1023) / 1024;
    const uint32_t begin = tid * per < p.n_lists ? tid * per : p.n_lists, end = begin + per < p.n_lists ? begin + per : p.n_lists;
    uint32_t qs = 0;
    uint64_t is = 0;
    for (uint32_t l = begin; l < end; l++) {
        const uint32_t c = p.cnt[l];
        qs += c;
        is += (uint64_t)((c + p.q_block - 1) / p.q_block) * vl_segs(p.list_begin, l, p.seg_rows);
    }
    s_q[tid] = qs;
    s_i[tid] = is;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t oq = tid >= d ? s_q[tid - d] : 0u;
        const uint64_t oi = tid >= d ? s_i[tid - d] : 0ull;
        __syncthreads();
        s_q[tid] += oq;
        s_i[tid] += oi;
        __syncthreads();
    }
    uint32_t rq = s_q[tid] - qs;
    uint64_t ri = s_i[tid] - is;
    for (uint32_t l = begin; l < end; l++) {
        const uint32_t c = p.cnt[l];
        p.q_begin[l] = rq;
        p.item_begin[l] = ri;
        p.cur[l] = 0;
        rq += c;
        ri += (uint64_t)((c + p.q_block - 1) / p.q_block) * vl_segs(p.list_begin, l, p.seg_rows);
    }
    if (tid == 1023) p.item_begin[p.n_lists] = s_i[1023];
}

__global__ __launch_bounds__(256) void k_vl_fill(VlInvertParams p, uint64_t n_pairs) {
    const uint64_t pair = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pair >= n_pairs) return;
    const uint32_t l = p.probe[pair].doc;
    p.run[p.q_begin[l] + atomicAdd(&p.cur[l], 1u)] = (uint32_t)pair;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------------
struct VecListsParams {
    const int8_t* lvec;                // [n_rows][dim] list-major
    const uint32_t* row_doc;           // [n_rows]
    const uint32_t* list_begin;        // [n_lists + 1]
    uint64_t n_rows;                   // rows that are in a list
    const int8_t* qvec;                // [n_q][dim], 16-byte aligned
    const int32_t* q_mask;             // [n_q] or nullptr
    const uint32_t* masks;
    uint64_t mask_words;
    const uint32_t* cnt;
    const uint32_t* q_begin;
    const uint32_t* run;
    const uint64_t* item_begin;
    const uint32_t* slot_base;
    uint64_t* part;                    // [n_q][slots_per_q][k]
    uint64_t slots_per_q, seg_rows;
    uint32_t dim, k, cap, row_stride, n_lists, n_probe;
};

constexpr uint32_t VL_NO_QUERY = 0xFFFFFFFFu;

template <int QT>
__global__ __launch_bounds__(VT_TPB) void k_vec_topk_lists(VecListsParams p) {
    constexpr uint32_t QB = QT * 16;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* const s_q = smem;                                              // [QB][row_stride]: k_vec_topk's image
    uint64_t* const s_buf = reinterpret_cast<uint64_t*>(smem + (size_t)QB * p.row_stride);   // [QB][cap]
    uint64_t* const s_thr = s_buf + (size_t)QB * p.cap;                           // [QB]
    uint64_t* const s_out = s_thr + QB;                                           // [QB] the query's partial slot of this item   } in the place of
    int32_t* const s_mid = reinterpret_cast<int32_t*>(s_out + QB);                // [QB] its allow-list                          } k_vec_topk's
    uint32_t* const s_qi = reinterpret_cast<uint32_t*>(s_mid + QB);               // [QB] the query, VL_NO_QUERY past the group   } [VT_WAVES][QB] words
    uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_out + VT_WAVES * QB);   // [QB]
    uint32_t* const s_hist = s_cnt + QB;                                          // [256]
    uint32_t* const s_sel = s_hist + 256;                                         // [16]
    uint16_t* const s_holes = reinterpret_cast<uint16_t*>(s_sel + 16);            // [HOLES]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = lane & 15u, h = lane >> 4;
    const uint32_t k = p.k, cap = p.cap, dim = p.dim;
    const bool tight = cap < k + VT_WAVES * VT_TILE;
    const uint32_t inc = tight ? VT_TILE : VT_WAVES * VT_TILE;
    const uint32_t row_chunks = dim / 16;
    const uint64_t total = p.item_begin[p.n_lists];
    for (uint64_t item = blockIdx.x; item < total; item += gridDim.x) {
        // ---- the item's list: item_begin[l] <= item < item_begin[l + 1]; its segment and group of queries
        uint32_t lo = 0, hi = p.n_lists;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (p.item_begin[mid] <= item) lo = mid;
            else hi = mid;
        }
        const uint32_t l = lo, c = p.cnt[l], n_groups = (c + QB - 1) / QB;
        const uint64_t local = item - p.item_begin[l];
        const uint32_t seg = (uint32_t)(local / n_groups), group = (uint32_t)(local - (uint64_t)seg * n_groups);
        const uint32_t gq = c - group * QB < QB ? c - group * QB : QB;            // queries of the group, >= 1
        const uint64_t l_end = p.list_begin[l + 1];
        const uint64_t r_begin = (uint64_t)p.list_begin[l] + (uint64_t)seg * p.seg_rows;          // < l_end
        const uint64_t r_end = r_begin + p.seg_rows < l_end ? r_begin + p.seg_rows : l_end;      // rows behind it belong to the next segment or list
        const uint32_t n_tiles = (uint32_t)((r_end - r_begin + VT_TILE - 1) / VT_TILE);
        const uint32_t n_rounds = (n_tiles + VT_WAVES - 1) / VT_WAVES;
        __syncthreads();                                                          // (the item before has left the LDS)
        if (tid < QB) {
            uint32_t qi = VL_NO_QUERY;
            int32_t mid = -1;
            uint64_t out = 0;
            if (tid < gq) {
                const uint32_t pair = p.run[p.q_begin[l] + group * QB + tid];
                qi = pair / p.n_probe;
                if (p.q_mask) mid = p.q_mask[qi];
                out = (uint64_t)qi * p.slots_per_q + p.slot_base[pair] + seg;
            }
            s_qi[tid] = qi; s_mid[tid] = mid; s_out[tid] = out;
            s_thr[tid] = 0; s_cnt[tid] = 0;
        }
        if (tid < 3) s_sel[4 + tid] = 0;
        __syncthreads();
        for (uint32_t x = tid; x < QB * row_chunks; x += VT_TPB) {
            const uint32_t row = x / row_chunks, cc = x - row * row_chunks;
            const uint32_t qi = s_qi[row];
            v4i v = {0, 0, 0, 0};
            if (qi != VL_NO_QUERY) v = *reinterpret_cast<const v4i*>(p.qvec + (size_t)qi * dim + (size_t)cc * 16);
            *reinterpret_cast<v4i*>(s_q + (size_t)row * p.row_stride + (size_t)cc * 16) = v;
        }
        uint32_t chk = 0;
        __syncthreads();
        for (uint32_t round = 0; round < n_rounds; round++) {
            const uint32_t tile = round * VT_WAVES + wave;
            const uint64_t d0 = r_begin + (uint64_t)tile * VT_TILE;
            uint64_t w = 0;                                                       // which of the wave's 64 rows are the segment's
            if (tile < n_tiles) {
                const uint64_t left = r_end - d0;
                w = left >= 64 ? ~0ull : (1ull << left) - 1ull;
            }
            const bool any = w != 0;
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
                    if (d >= p.n_rows) d = p.n_rows - 1;                          // (its bit in w is 0)
                    a_ptr[t] = p.lvec + d * dim + h * 16;
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
            // ---- candidates: accumulator register g of tile (t, j) is row d0 + 16 t + 4 h + g under the group's query j * 16 + r
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (tight || t == 0) {                                            // k_vec_topk's three-flag check: the branch is uniform
                    __syncthreads();
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
                    const uint32_t bits = (uint32_t)(w >> (t * 16 + h * 4)) & 15u;
#pragma unroll
                    for (int j = 0; j < QT; j++) {
                        const uint32_t ql = (uint32_t)j * 16 + r;
                        if (bits && ql < gq) {
                            const uint64_t thr = s_thr[ql];
                            const int32_t mid = s_mid[ql];
#pragma unroll
                            for (int g = 0; g < 4; g++) {
                                if ((bits >> g & 1u) && ((uint32_t)acc[t][j][g] ^ 0x80000000u) >= (uint32_t)(thr >> 32)) {
                                    const uint32_t doc = p.row_doc[d0 + (uint32_t)(t * 16 + h * 4 + g)];
                                    const uint64_t key = vec_key(acc[t][j][g], doc);
                                    if (key > thr && (mid < 0 || (p.masks[(uint64_t)mid * p.mask_words + (doc >> 5)] >> (doc & 31u) & 1u))) {
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
        }
        // ---- the item's lists: at most k keys per query, the other slots 0
        __syncthreads();
        for (uint32_t ql = 0; ql < gq; ql++) {
            uint32_t n = s_cnt[ql];
            if (n > k) {
                vec_compact(s_buf + (size_t)ql * cap, n, k, &s_thr[ql], &s_cnt[ql], s_hist, s_sel, s_holes);
                n = k;
            }
            uint64_t* const out = p.part + s_out[ql] * k;
            for (uint32_t i = tid; i < k; i += VT_TPB) out[i] = i < n ? s_buf[(size_t)ql * cap + i] : 0ull;
        }
    }
}

struct VecListsMergeParams {
    const uint64_t* part;              // [n_q][slots_per_q][k]
    const uint32_t* n_slots;           // [n_q] slots the query filled
    uint64_t slots_per_q;
    uint32_t k;
    ss_vec_hit* hits_out;
    int32_t* n_hits_out;
};

__global__ __launch_bounds__(VM_TPB) void k_vec_merge_lists(VecListsMergeParams p) {
    __shared__ uint64_t s_key[SS_MAX_TOPK];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[4];
    const uint32_t q = blockIdx.x;
    ss::vecdev::vec_merge_query(p.part + (uint64_t)q * p.slots_per_q * p.k, p.n_slots[q] * p.k, p.k, p.hits_out + (size_t)q * p.k, p.n_hits_out + q, s_key,
                                s_hist, s_sel);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <typename T>
int32_t need(ss_ctx* ctx, const char* who, ss::DevBuf<T>& b, size_t n) {
    const hipError_t e = ensure(b, n);
    if (e == hipSuccess) return SS_OK;
    (void)hipGetLastError();
    return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %zu bytes", who, n * sizeof(T));
}
template <typename T>
int32_t fresh(ss_ctx* ctx, const char* who, ss::DevBuf<T>& b, size_t n) {
    const hipError_t e = b.alloc(std::max<size_t>(n, 1));
    if (e == hipSuccess) return SS_OK;
    (void)hipGetLastError();
    return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %zu bytes", who, n * sizeof(T));
}

template <int QT>
int32_t launch_lists(ss_scorer* s, const VecListsParams& p, const vl::Plan& pl, unsigned grid, hipStream_t st) {
    ss_ctx* ctx = s->ctx;
    if (s->vl_lds_attr[QT] < (int)pl.lds_bytes) {
        SS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vec_topk_lists<QT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
        s->vl_lds_attr[QT] = (int)pl.lds_bytes;
    }
    hipLaunchKernelGGL((k_vec_topk_lists<QT>), dim3(grid), dim3(VT_TPB), pl.lds_bytes, st, p);
    return SS_OK;
}

int32_t set_lists_impl(ss_scorer* s, int32_t n_lists, const int8_t* centroids, const uint32_t* list_of_doc) {
    static const char* const who = "ss_scorer_set_vector_lists";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool clear = n_lists == 0 || !centroids;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (clear) {
        SS_HIP(ctx, hipStreamSynchronize(st));
        for (hipStream_t ws : ctx->wave_stream)
            if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
        ss::vec_lists_drop(s);
        return SS_OK;
    }
    if (n_lists < 0 || n_lists > SS_MAX_VEC_LISTS) return ctx->fail(SS_ERR_INVALID, "%s: n_lists = %d is outside [0, %d]", who, n_lists, SS_MAX_VEC_LISTS);
    if (!list_of_doc) return ctx->fail(SS_ERR_INVALID, "%s: list_of_doc is NULL", who);
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no vector table registered (ss_scorer_set_doc_vectors)", who);
    const size_t n = (size_t)s->n_docs, dim = (size_t)s->vec_dim, L = (size_t)n_lists;
    // ---- every entry checked on the host; the list lengths stay there
    std::vector<uint32_t> lod(n), len(L, 0u);
    SS_HIP(ctx, ss::copy_in(st, lod.data(), list_of_doc, n * sizeof(uint32_t)));
    size_t rows = 0;
    for (size_t d = 0; d < n; d++) {
        if (lod[d] == SS_NO_LIST) continue;
        if (lod[d] >= (uint32_t)n_lists)
            return ctx->fail(SS_ERR_INVALID, "%s: doc %zu is in list %u (there are %d lists)", who, d, lod[d], n_lists);
        len[lod[d]]++;
        rows++;
    }
    std::vector<uint32_t> begin(L + 1, 0u);
    for (size_t l = 0; l < L; l++) begin[l + 1] = begin[l] + len[l];
    // ---- the new blocks: a failure leaves the old lists in place
    ss::DevBuf<int8_t> n_cent, n_vec;
    ss::DevBuf<uint32_t> n_begin, key_a, key_b, val_a, val_b, hist;
    const uint32_t n_tiles = (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    SS_TRY(fresh(ctx, who, n_cent, L * dim));
    SS_TRY(fresh(ctx, who, n_vec, rows * dim));
    SS_TRY(fresh(ctx, who, n_begin, L + 1));
    SS_TRY(fresh(ctx, who, key_a, n));
    SS_TRY(fresh(ctx, who, key_b, n));
    SS_TRY(fresh(ctx, who, val_a, n));
    SS_TRY(fresh(ctx, who, val_b, n));
    SS_TRY(fresh(ctx, who, hist, (size_t)256 * std::max<uint32_t>(n_tiles, 1)));
    SS_HIP(ctx, hipMemcpyAsync(n_cent.p, centroids, L * dim, hipMemcpyDefault, st));
    SS_HIP(ctx, hipMemcpyAsync(n_begin.p, begin.data(), (L + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    uint32_t *k_in = key_a.p, *k_out = key_b.p, *v_in = val_a.p, *v_out = val_b.p;
    if (n) {
        SS_HIP(ctx, hipMemcpyAsync(key_a.p, lod.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vl_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, key_a.p, val_a.p, (uint64_t)n, (uint32_t)n_lists);
        const uint32_t max_key = rows < n ? (uint32_t)n_lists : (uint32_t)n_lists - 1;
        for (uint32_t shift = 0; shift < 32 && (max_key >> shift) != 0; shift += 8) {
            hipLaunchKernelGGL(k_vl_hist, dim3(n_tiles), dim3(64), 0, st, k_in, (uint64_t)n, shift, n_tiles, hist.p);
            hipLaunchKernelGGL(k_vl_scan_u32, dim3(1), dim3(1024), 0, st, hist.p, (uint64_t)256 * n_tiles);
            hipLaunchKernelGGL(k_vl_scatter, dim3(n_tiles), dim3(64), 0, st, k_in, v_in, k_out, v_out, (uint64_t)n, shift, n_tiles, hist.p);
            std::swap(k_in, k_out);
            std::swap(v_in, v_out);
        }
        if (rows) {
            const uint64_t threads = (uint64_t)rows * (dim / 16);
            hipLaunchKernelGGL(k_vl_gather_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, s->vec.p, v_in, n_vec.p, (uint64_t)rows, (uint32_t)dim);
        }
        SS_HIP(ctx, hipGetLastError());
    }
    // the scorer's outstanding work may read the old lists: drained, as ss_scorer_set_doc_vectors does, before they are replaced
    SS_HIP(ctx, hipStreamSynchronize(st));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    std::sort(len.begin(), len.end(), [](uint32_t a, uint32_t b) { return a > b; });
    s->vl_centroids = std::move(n_cent);
    s->vl_vec = std::move(n_vec);
    s->vl_row_doc = std::move(v_in == val_a.p ? val_a : val_b);
    s->vl_list_begin = std::move(n_begin);
    s->vl_len_desc = std::move(len);
    s->vl_rows = rows;
    s->vl_n_lists = n_lists;
    return SS_OK;
}

int32_t assign_impl(ss_scorer* s, int32_t n_lists, const int8_t* centroids, uint32_t* list_out, int32_t* score_out) {
    static const char* const who = "ss_vector_assign_lists";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_lists < 1 || n_lists > SS_MAX_VEC_LISTS) return ctx->fail(SS_ERR_INVALID, "%s: n_lists = %d is outside [1, %d]", who, n_lists, SS_MAX_VEC_LISTS);
    if (!centroids || !list_out) return ctx->fail(SS_ERR_INVALID, "%s: centroids or list_out is NULL", who);
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no vector table registered (ss_scorer_set_doc_vectors)", who);
    if (s->n_docs == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)s->n_docs, dim = (size_t)s->vec_dim;
    const size_t batch = (size_t)std::min<uint64_t>(vl::assign_batch(ctx->opt("vec.assign_batch", 0)), n);
    SS_TRY(need(ctx, who, s->d_vl_cent, (size_t)n_lists * dim));
    SS_TRY(need(ctx, who, s->d_vl_assign, batch));
    SS_TRY(need(ctx, who, s->d_vl_assign_n, batch));
    SS_HIP(ctx, hipMemcpyAsync(s->d_vl_cent.p, centroids, (size_t)n_lists * dim, hipMemcpyDefault, st));
    const bool dev_l = ss::on_device(list_out), dev_s = score_out && ss::on_device(score_out);
    std::vector<ss_vec_hit> rows;
    if (!dev_l || (score_out && !dev_s)) rows.resize(n);
    for (size_t b0 = 0; b0 < n; b0 += batch) {
        const size_t nb = std::min(batch, n - b0);
        SS_TRY(ss::vec_table_topk(s, who, s->d_vl_cent.p, (uint64_t)n_lists, (int32_t)nb, s->vec.p + b0 * dim, 1, s->d_vl_assign.p, s->d_vl_assign_n.p));
        // {doc, score} of the row becomes {list_out, score_out}: a strided copy, no kernel
        if (dev_l) SS_HIP(ctx, hipMemcpy2DAsync(list_out + b0, 4, &s->d_vl_assign.p->doc, 8, 4, nb, hipMemcpyDeviceToDevice, st));
        if (dev_s) SS_HIP(ctx, hipMemcpy2DAsync(score_out + b0, 4, &s->d_vl_assign.p->score, 8, 4, nb, hipMemcpyDeviceToDevice, st));
        if (!rows.empty()) {
            SS_HIP(ctx, hipMemcpyAsync(rows.data() + b0, s->d_vl_assign.p, nb * sizeof(ss_vec_hit), hipMemcpyDeviceToHost, st));
            SS_HIP(ctx, hipStreamSynchronize(st));                                // (the block is the next batch's)
        }
    }
    if (!rows.empty()) {
        for (size_t d = 0; d < n; d++) {
            if (!dev_l) list_out[d] = rows[d].doc;
            if (score_out && !dev_s) score_out[d] = rows[d].score;
        }
    }
    return SS_OK;
}

int32_t probed_impl(ss_scorer* s, int32_t n_q, const int8_t* qvec, const int32_t* mask_id, int32_t k, int32_t n_probe, ss_vec_hit* hits_out,
                    int32_t* n_hits_out, uint32_t* probes_out) {
    static const char* const who = "ss_vector_topk_probed";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_q < 0", who);
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "%s: k = %d must be >= 1", who, k);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: k = %d exceeds SS_MAX_TOPK = %d", who, k, SS_MAX_TOPK);
    if (n_probe < 1) return ctx->fail(SS_ERR_INVALID, "%s: n_probe = %d must be >= 1", who, n_probe);
    if (n_probe > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: n_probe = %d exceeds SS_MAX_TOPK = %d", who, n_probe, SS_MAX_TOPK);
    if (n_q > 0 && (!qvec || !hits_out || !n_hits_out)) return ctx->fail(SS_ERR_INVALID, "%s: qvec, hits_out or n_hits_out is NULL", who);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_q;
    std::vector<int32_t> mid;
    bool masked = false;
    if (mask_id && nq) {
        mid.resize(nq);
        SS_HIP(ctx, ss::copy_in(ctx->stream, mid.data(), mask_id, nq * sizeof(int32_t)));
        for (size_t q = 0; q < nq; q++) {
            if (mid[q] < -1 || mid[q] >= s->n_masks)
                return ctx->fail(SS_ERR_INVALID, "%s: query %zu has mask id %d (the scorer has %d masks)", who, q, mid[q], s->n_masks);
            masked |= mid[q] >= 0;
        }
    }
    if (s->vec_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no vector table registered (ss_scorer_set_doc_vectors)", who);
    if (s->vl_n_lists == 0) return ctx->fail(SS_ERR_STATE, "%s: no vector lists registered (ss_scorer_set_vector_lists)", who);
    if (n_q == 0) return SS_OK;
    int lds_limit = 0;
    SS_HIP(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const uint32_t L = (uint32_t)s->vl_n_lists;
    const vl::Plan pl = vl::plan(s->vl_len_desc.data(), L, s->vl_rows, (uint32_t)s->vec_dim, nq, (uint32_t)k, (uint32_t)n_probe, ctx->opt("vec.list_seg_rows", 0),
                                 ctx->opt("vec.list_batch_q", 0), (uint32_t)ctx->cu_count, (uint32_t)std::min(lds_limit, 160 << 10));
    if (pl.too_large) return ctx->fail(SS_ERR_OOM, "%s: the partial lists of one query (%llu segments at k = %d) do not fit", who, (unsigned long long)pl.slots_per_q, k);
    if (!pl.ok) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: k = %d and dim %d need more than the device's %d bytes of LDS", who, k, s->vec_dim, lds_limit);
    hipStream_t st = ctx->stream;
    const uint32_t P = pl.n_probe;
    const size_t qb = (size_t)std::min<uint64_t>(pl.q_batch, nq);
    const bool dev_h = ss::on_device(hits_out), dev_n = ss::on_device(n_hits_out), dev_p = probes_out && ss::on_device(probes_out);
    if (!dev_h) SS_TRY(need(ctx, who, s->d_vl_hits, nq * (size_t)k));
    if (!dev_n) SS_TRY(need(ctx, who, s->d_vl_n, nq));
    if (probes_out && !dev_p) SS_TRY(need(ctx, who, s->d_vl_probes_out, nq * (size_t)P));
    SS_TRY(need(ctx, who, s->d_vl_probe, qb * P));
    SS_TRY(need(ctx, who, s->d_vl_probe_n, qb));
    SS_TRY(need(ctx, who, s->d_vl_cnt, (size_t)3 * L));
    SS_TRY(need(ctx, who, s->d_vl_run, qb * P));
    SS_TRY(need(ctx, who, s->d_vl_slot, qb * P));
    SS_TRY(need(ctx, who, s->d_vl_nslots, qb));
    SS_TRY(need(ctx, who, s->d_vl_item_begin, (size_t)L + 1));
    SS_TRY(need(ctx, who, s->d_vl_part, (size_t)pl.part_keys));
    ss_vec_hit* const o_hits = dev_h ? hits_out : s->d_vl_hits.p;
    int32_t* const o_n = dev_n ? n_hits_out : s->d_vl_n.p;
    uint32_t* const o_p = !probes_out ? nullptr : dev_p ? probes_out : s->d_vl_probes_out.p;
    bool staged = false;
    const int8_t* d_q = nullptr;
    SS_TRY(ss::vec_queries_to_device(s, qvec, nq * (size_t)s->vec_dim, &d_q, &staged));
    const int32_t* d_mid = nullptr;
    if (masked && s->mask_words) {                                                // the ids go up as ss_vector_topk's do
        if (ss::on_device(mask_id)) d_mid = mask_id;
        else {
            SS_HIP(ctx, s->ev_vec_mid.wait());
            SS_HIP(ctx, s->h_vec_mid.ensure(nq * sizeof(int32_t)));
            SS_TRY(need(ctx, who, s->d_vec_mid, nq));
            std::memcpy(s->h_vec_mid.p, mid.data(), nq * sizeof(int32_t));
            SS_HIP(ctx, hipMemcpyAsync(s->d_vec_mid.p, s->h_vec_mid.p, nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
            SS_HIP(ctx, s->ev_vec_mid.record(st));
            d_mid = s->d_vec_mid.p;
        }
    }
    const unsigned grid = (unsigned)std::max(1, 4 * ctx->cu_count);
    for (size_t q0 = 0; q0 < nq; q0 += qb) {                                      // query batches: the partial lists stay in bound
        const size_t nb = std::min(qb, nq - q0);
        SS_TRY(ss::vec_table_topk(s, who, s->vl_centroids.p, L, (int32_t)nb, d_q + q0 * (size_t)s->vec_dim, (int32_t)P, s->d_vl_probe.p, s->d_vl_probe_n.p));
        VlInvertParams iv{};
        iv.probe = s->d_vl_probe.p;
        iv.list_begin = s->vl_list_begin.p;
        iv.cnt = s->d_vl_cnt.p; iv.q_begin = s->d_vl_cnt.p + L; iv.cur = s->d_vl_cnt.p + 2 * (size_t)L;
        iv.run = s->d_vl_run.p;
        iv.item_begin = s->d_vl_item_begin.p;
        iv.slot_base = s->d_vl_slot.p;
        iv.n_slots = s->d_vl_nslots.p;
        iv.probes_out = o_p ? o_p + q0 * P : nullptr;
        iv.seg_rows = pl.seg_rows;
        iv.n_probe = P; iv.n_lists = L; iv.q_block = pl.q_block;
        SS_HIP(ctx, hipMemsetAsync(iv.cnt, 0, (size_t)L * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_vl_count, dim3((unsigned)nb), dim3(64), 0, st, iv);
        hipLaunchKernelGGL(k_vl_scan_lists, dim3(1), dim3(1024), 0, st, iv);
        hipLaunchKernelGGL(k_vl_fill, dim3((unsigned)((nb * P + 255) / 256)), dim3(256), 0, st, iv, (uint64_t)nb * P);
        SS_HIP(ctx, hipGetLastError());
        VecListsParams p{};
        p.lvec = s->vl_vec.p;
        p.row_doc = s->vl_row_doc.p;
        p.list_begin = s->vl_list_begin.p;
        p.n_rows = s->vl_rows;
        p.qvec = d_q + q0 * (size_t)s->vec_dim;
        p.q_mask = d_mid ? d_mid + q0 : nullptr;
        p.masks = s->masks.p;
        p.mask_words = s->mask_words;
        p.cnt = iv.cnt; p.q_begin = iv.q_begin; p.run = iv.run; p.item_begin = iv.item_begin; p.slot_base = iv.slot_base;
        p.part = s->d_vl_part.p;
        p.slots_per_q = pl.slots_per_q; p.seg_rows = pl.seg_rows;
        p.dim = (uint32_t)s->vec_dim; p.k = (uint32_t)k; p.cap = pl.cap; p.row_stride = pl.row_stride; p.n_lists = L; p.n_probe = P;
        if (s->vl_rows && !(masked && s->mask_words == 0)) {                      // (otherwise every item would be empty)
            if (pl.q_block == 64) SS_TRY(launch_lists<4>(s, p, pl, grid, st));
            else if (pl.q_block == 32) SS_TRY(launch_lists<2>(s, p, pl, grid, st));
            else SS_TRY(launch_lists<1>(s, p, pl, grid, st));
            SS_HIP(ctx, hipGetLastError());
            VecListsMergeParams m{};
            m.part = s->d_vl_part.p;
            m.n_slots = s->d_vl_nslots.p;
            m.slots_per_q = pl.slots_per_q;
            m.k = (uint32_t)k;
            m.hits_out = o_hits + q0 * (size_t)k;
            m.n_hits_out = o_n + q0;
            hipLaunchKernelGGL(k_vec_merge_lists, dim3((unsigned)nb), dim3(VM_TPB), 0, st, m);
            SS_HIP(ctx, hipGetLastError());
        } else {
            SS_HIP(ctx, hipMemsetAsync(o_n + q0, 0, nb * sizeof(int32_t), st));
        }
    }
    if (dev_h && dev_n && (!probes_out || dev_p)) {
        if (staged) SS_HIP(ctx, hipStreamSynchronize(st));
        return SS_OK;                                     // ordered on the ctx stream; nothing comes back
    }
    // ---- host outputs: the counts and the probes whole, of the rows exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq);
    std::vector<ss_vec_hit> h_rows;
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), o_n, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_h) {
        h_rows.resize(nq * (size_t)k);
        SS_HIP(ctx, hipMemcpyAsync(h_rows.data(), o_hits, nq * (size_t)k * sizeof(ss_vec_hit), hipMemcpyDeviceToHost, st));
    }
    if (probes_out && !dev_p) SS_HIP(ctx, hipMemcpyAsync(probes_out, o_p, nq * (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_hits_out, h_n.data(), nq * sizeof(int32_t));
    if (!dev_h)
        for (size_t q = 0; q < nq; q++)
            std::memcpy(hits_out + q * (size_t)k, h_rows.data() + q * (size_t)k, (size_t)h_n[q] * sizeof(ss_vec_hit));
    return SS_OK;
}

}  // namespace

void ss::vec_lists_drop(ss_scorer* s) {
    s->vl_centroids.release();
    s->vl_vec.release();
    s->vl_row_doc.release();
    s->vl_list_begin.release();
    s->vl_len_desc.clear();
    s->vl_rows = 0;
    s->vl_n_lists = 0;
}

extern "C" {

int32_t ss_scorer_set_vector_lists(ss_scorer* s, int32_t n_lists, const int8_t* centroids, const uint32_t* list_of_doc) {
    return hw::guarded(s, "ss_scorer_set_vector_lists", [&] { return set_lists_impl(s, n_lists, centroids, list_of_doc); });
}

int32_t ss_vector_assign_lists(ss_scorer* s, int32_t n_lists, const int8_t* centroids, uint32_t* list_out, int32_t* score_out) {
    return hw::guarded(s, "ss_vector_assign_lists", [&] { return assign_impl(s, n_lists, centroids, list_out, score_out); });
}

int32_t ss_vector_topk_probed(ss_scorer* s, int32_t n_q, const int8_t* qvec, const int32_t* mask_id, int32_t k, int32_t n_probe, ss_vec_hit* hits_out,
                              int32_t* n_hits_out, uint32_t* probes_out) {
    return hw::guarded(s, "ss_vector_topk_probed", [&] { return probed_impl(s, n_q, qvec, mask_id, k, n_probe, hits_out, n_hits_out, probes_out); });
}

}  // extern "C"
