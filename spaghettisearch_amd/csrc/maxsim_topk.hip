// maxsim_topk.hip — ss_maxsim_topk: the exact top k of every query by late-interaction score over ALL docs of the token table
// ss_scorer_set_doc_tokens registered (maxsim.hip), not over a window some other call produced.
//
//   k_maxsim_topk<QT>  grid (chunk of docs, block of qb <= 16 queries), four waves.  A chunk is a run of slices of the cut table, i.e. the
//                      docs [cut[first slice], cut[end slice]): chunks are cut at doc boundaries by token count.  The block's queries
//                      sit in LDS for the whole chunk, each as 16 QT token slots in k_maxsim_scores' row layout (slots at or past m_q
//                      zero, and masked out of the sum).  The chunk is walked in groups of 64 consecutive docs (aligned to 64, so a
//                      group's allow-list bits are two 32-bit words).  Every wave forms the same two ballot words per group from the
//                      same read-only memory — lane l: doc 64 g + l, its token count, and one bit per query of the block that may
//                      take it — `own` (docs a single wave walks) and `wide` (docs of at least "maxsim.wide_tokens" tokens, walked by
//                      all four).  A doc without tokens or that no query of the block may take has no bit: nothing of it is loaded.
//                      The docs of `own` are dealt to the waves in turn.  A wave walks its doc 16 tokens at a time — only the tiles
//                      the doc has — loads the tile once, straight from memory, as the A operand of
//                      __builtin_amdgcn_mfma_i32_16x16x64_i8 by maxsim.hip's rule (rows at or past T_d clamped to the doc's last
//                      token, so every address lies in the doc's rows) and multiplies it with the B tiles of EVERY query of the block
//                      that may take the doc, eight queries at a time: 8 x QT accumulators of 4 registers.  Register g of lane l of
//                      accumulator (q, j) is doc token 16 tile + 4 (l >> 4) + g under slot 16 j + (l & 15) of query q: folded into one running maximum per
//                      (q, j), a token at or past T_d as INT32_MIN, never as its product.  At the end of the doc the maxima are joined
//                      over the four lane groups, the slots below m_q summed, and lane q forms vector.hip's key of (score, doc) and
//                      appends it to query q's LDS list if it beats the query's threshold.
//                      A wide doc's tiles are dealt to the four waves, which join their maxima per (query, slot) by integer max in
//                      LDS; wave 0 sums and appends.  Max is associative and commutative, and a key names its doc: no row depends on
//                      which wave saw which token or finished first.
//                      One barrier and one 'a list is nearly full' check per group with a candidate (k_vec_topk's three-flag
//                      protocol; a query gains at most 64 keys per group): a list that could overflow in the next group is cut back to
//                      its k largest keys by vecdev::vec_compact and the k-th becomes the threshold.  The chunk's <= k keys per query
//                      go to the partial lists, unused slots 0; k_vec_merge (vector.hip) merges the chunks.
// No float.  The host side only enqueues: the plan (maxsim_topk_plan.hpp) uses what the host knew when the table was registered.
#include "hit_window.hpp"
#include "maxsim_plan.hpp"
#include "maxsim_topk_plan.hpp"
#include "vector_device.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>

namespace {

namespace hw = ss::hitwin;
namespace mp = ss::msp;
namespace tp = ss::mtp;

using ss::vecdev::v4i;
using ss::vecdev::vec_compact;
using ss::vecdev::vec_key;

static_assert(tp::HOLES == ss::vec::HOLES && tp::MAX_K == SS_MAX_TOPK && ss::vec::MAX_K == SS_MAX_TOPK, "maxsim_topk_plan.hpp states the limits");
static_assert(ss::vecdev::VT_TPB == (int)mp::TPB, "vec_compact runs with the workgroup of k_maxsim_topk");
static_assert(tp::GROUP_DOCS == 64 && tp::MAX_QB == 16, "one ballot word per group, one lane group of queries");

struct MaxSimTopkParams {
    const int8_t* tok;                 // [tok_ptr[n_docs]][dim]
    const uint64_t* tok_ptr;           // [n_docs + 1]
    const uint32_t* cut;               // [n_slices + 1]
    uint64_t n_slices, chunk_slices;
    const int8_t* qtok;                // 16-byte aligned; query q's tokens at rows qt_ptr[q] ..
    const uint32_t* qt_ptr;            // [n_q + 1], device
    const int32_t* q_mask;             // [n_q] or nullptr: every query -1
    const uint32_t* masks;             // the scorer's allow-lists [n_masks][mask_words]
    uint64_t mask_words;
    uint64_t* part;                    // [n_q][n_chunks][k]
    uint32_t dim, n_q, k, qb, n_chunks, cap, row_stride, wide_tokens;
};

// One 16-token tile of a doc against QG = 8 queries, Q0 .. Q0 + 7: the products, then register g of accumulator (q, j) — doc token
// t0 + 4 h + g under slot 16 j + r of query Q0 + q — folded into mx[Q0 + q][j].  ALL: every query of the group is multiplied, with no
// branch between the products, so the LDS reads of one k step are in flight together (with a uniform branch per query every B tile
// waited for its own read: measured 4.8 us per tile, a tenth of the matrix cores' rate); otherwise only the queries of `bits`.
template <int QT, int Q0, bool ALL>
__device__ __forceinline__ void tile_maxima(const int8_t* a_ptr, uint32_t dim, const unsigned char* b_ptr, uint32_t row_stride, uint32_t q_stride,
                                            uint32_t bits, uint32_t t0, uint32_t T, uint32_t h, int32_t (&mx)[tp::MAX_QB][QT]) {
    constexpr int QG = 8;
    v4i acc[QG][QT];
#pragma unroll
    for (int q = 0; q < QG; q++)
#pragma unroll
        for (int j = 0; j < QT; j++) acc[q][j] = v4i{0, 0, 0, 0};
    for (uint32_t ks = 0; ks < dim; ks += 64) {
        const v4i a = *reinterpret_cast<const v4i*>(a_ptr + ks);
#pragma unroll
        for (int q = 0; q < QG; q++) {
            if (ALL || (bits >> q & 1u)) {                                        // (uniform)
#pragma unroll
                for (int j = 0; j < QT; j++) {
                    const v4i b = *reinterpret_cast<const v4i*>(b_ptr + (size_t)(Q0 + q) * q_stride + (size_t)j * 16 * row_stride + ks);
                    acc[q][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[q][j], 0, 0, 0);
                }
            }
        }
    }
    if (T - t0 >= mp::TILE_TOKENS) {                                              // (uniform) every row is a token
#pragma unroll
        for (int q = 0; q < QG; q++) {
            if (ALL || (bits >> q & 1u)) {
#pragma unroll
                for (int j = 0; j < QT; j++)
#pragma unroll
                    for (int g = 0; g < 4; g++) mx[Q0 + q][j] = max(mx[Q0 + q][j], acc[q][j][g]);
            }
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const bool live = t0 + h * 4 + (uint32_t)g < T;
#pragma unroll
            for (int q = 0; q < QG; q++) {
                if (ALL || (bits >> q & 1u)) {
#pragma unroll
                    for (int j = 0; j < QT; j++) mx[Q0 + q][j] = max(mx[Q0 + q][j], live ? acc[q][j][g] : INT32_MIN);
                }
            }
        }
    }
}

// The running maxima of one doc: tiles tile0, tile0 + step, .. of its T > 0 tokens (row0: its first token) folded into mx[q][j] of every
// lane, for the queries q of `take` (uniform) — and, where a group of eight queries lies wholly inside the block's qb images, for all
// eight (a query outside `take` then holds maxima nobody reads).  b_ptr: the lane's 16 bytes of slot r of query 0 in LDS; q_stride:
// bytes from one query's image to the next.  Every address: row0 + x * dim + [0, dim) with x < T.
template <int QT>
__device__ __forceinline__ void doc_maxima(const int8_t* row0, uint32_t T, uint32_t dim, const unsigned char* b_ptr, uint32_t row_stride,
                                           uint32_t q_stride, uint32_t tile0, uint32_t step, uint32_t take, uint32_t qb, uint32_t r, uint32_t h,
                                           int32_t (&mx)[tp::MAX_QB][QT]) {
    const uint32_t lo = take & 255u, hi = take >> 8;
    const bool all_lo = qb >= 8, all_hi = qb >= 16;
    const uint32_t n_tiles = (T + mp::TILE_TOKENS - 1) / mp::TILE_TOKENS;
    for (uint32_t tile = tile0; tile < n_tiles; tile += step) {
        const uint32_t t0 = tile * mp::TILE_TOKENS;                               // < T
        uint32_t x = t0 + r;
        if (x >= T) x = T - 1;                                                    // (its slots are masked in the fold)
        const int8_t* const a_ptr = row0 + (uint64_t)x * dim + h * 16;
        // eight queries at a time (16 QT accumulators of 4 registers would not leave QT = 4 its maxima); the second half finds the tile in L1
        if (lo) {
            if (all_lo) tile_maxima<QT, 0, true>(a_ptr, dim, b_ptr, row_stride, q_stride, lo, t0, T, h, mx);
            else tile_maxima<QT, 0, false>(a_ptr, dim, b_ptr, row_stride, q_stride, lo, t0, T, h, mx);
        }
        if (hi) {
            if (all_hi) tile_maxima<QT, 8, true>(a_ptr, dim, b_ptr, row_stride, q_stride, hi, t0, T, h, mx);
            else tile_maxima<QT, 8, false>(a_ptr, dim, b_ptr, row_stride, q_stride, hi, t0, T, h, mx);
        }
    }
}

template <int QT>
__global__ __launch_bounds__(mp::TPB) void k_maxsim_topk(MaxSimTopkParams p) {
    constexpr uint32_t SLOTS = QT * 16;
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t qb = p.qb, cap = p.cap, k = p.k, dim = p.dim;
    const uint32_t q_stride = SLOTS * p.row_stride;
    unsigned char* const s_q = smem;                                              // [qb][SLOTS][row_stride]
    uint64_t* const s_buf = reinterpret_cast<uint64_t*>(smem + (size_t)qb * q_stride);   // [qb][cap]
    uint64_t* const s_thr = s_buf + (size_t)qb * cap;                             // [qb]
    int32_t* const s_join = reinterpret_cast<int32_t*>(s_thr + qb);               // [qb][SLOTS]: a wide doc's maxima, INT32_MIN between docs
    uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_join + (size_t)qb * SLOTS);    // [qb]
    int32_t* const s_mid = reinterpret_cast<int32_t*>(s_cnt + qb);                // [qb]: the query's allow-list, -1 = every doc
    uint32_t* const s_mq = reinterpret_cast<uint32_t*>(s_mid + qb);               // [qb]: its token count
    uint32_t* const s_hist = s_mq + qb;                                           // [256]
    uint32_t* const s_sel = s_hist + 256;                                         // [16]: vec_compact's words, [4 .. 6] = the 'a list is nearly full' flags
    uint16_t* const s_holes = reinterpret_cast<uint16_t*>(s_sel + 16);            // [HOLES]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = lane & 15u, h = lane >> 4;
    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * qb;
    const uint32_t n_live = p.n_q - q0 < qb ? p.n_q - q0 : qb;                    // >= 1: the launcher's grid
    // ---- the chunk's docs
    const uint64_t s_first = (uint64_t)chunk * p.chunk_slices;                    // < n_slices: the launcher's grid
    const uint64_t s_end = s_first + p.chunk_slices < p.n_slices ? s_first + p.chunk_slices : p.n_slices;
    const uint64_t d_begin = p.cut[s_first], d_end = p.cut[s_end];                // d_begin <= d_end <= n_docs
    // ---- the block's queries into LDS (slots at or past m_q, and queries past n_q: zeros), lists empty, thresholds 0 (below every key)
    const uint32_t row_chunks = dim / 16;
    for (uint32_t x = tid; x < qb * SLOTS * row_chunks; x += mp::TPB) {
        const uint32_t row = x / row_chunks, c = x - row * row_chunks;
        const uint32_t ql = row / SLOTS, slot = row - ql * SLOTS;
        v4i v = {0, 0, 0, 0};
        if (ql < n_live) {
            const uint32_t base = p.qt_ptr[q0 + ql], m = p.qt_ptr[q0 + ql + 1] - base;
            if (slot < m) v = *reinterpret_cast<const v4i*>(p.qtok + (size_t)(base + slot) * dim + (size_t)c * 16);   // (m <= SLOTS: the host chose QT)
        }
        *reinterpret_cast<v4i*>(s_q + (size_t)row * p.row_stride + (size_t)c * 16) = v;
    }
    for (uint32_t x = tid; x < qb * SLOTS; x += mp::TPB) s_join[x] = INT32_MIN;
    if (tid < qb) {
        s_thr[tid] = 0;
        s_cnt[tid] = 0;
        int32_t mid = -1;
        uint32_t m = 0;
        if (tid < n_live) {
            if (p.q_mask) mid = p.q_mask[q0 + tid];
            m = p.qt_ptr[q0 + tid + 1] - p.qt_ptr[q0 + tid];
            if (m > SLOTS) m = SLOTS;
        }
        s_mid[tid] = mid;
        s_mq[tid] = m;
    }
    if (tid < 3) s_sel[4 + tid] = 0;
    __syncthreads();
    uint32_t open_bits = 0, masked_bits = 0;                                      // (uniform) the block's queries that take every doc / have a list
    for (uint32_t ql = 0; ql < n_live; ql++) {
        if (s_mid[ql] < 0) open_bits |= 1u << ql;
        else masked_bits |= 1u << ql;
    }
    const unsigned char* const b_ptr = s_q + (size_t)r * p.row_stride + h * 16;
    uint32_t chk = 0;                                                             // checks so far
    const uint64_t g_first = d_begin >> 6;
    const uint64_t n_groups = d_end > d_begin ? ((d_end + 63) >> 6) - g_first : 0;

    // One doc's maxima of this wave, joined over the lane groups, as scores: lane q < 16 gets query q's.
    auto scores_of = [&](int32_t (&mx)[tp::MAX_QB][QT], uint32_t take, bool joined) -> int32_t {
        int32_t mine = 0;
#pragma unroll
        for (int q = 0; q < (int)tp::MAX_QB; q++) {
            if (take >> q & 1u) {                                                 // (uniform)
                if (!joined) {
#pragma unroll
                    for (int j = 0; j < QT; j++) {
                        mx[q][j] = max(mx[q][j], __shfl_xor(mx[q][j], 16));
                        mx[q][j] = max(mx[q][j], __shfl_xor(mx[q][j], 32));
                    }
                }
                const uint32_t m_q = s_mq[q];
                int32_t sum = 0;
#pragma unroll
                for (int j = 0; j < QT; j++) sum += (uint32_t)j * 16 + r < m_q ? mx[q][j] : 0;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
                if (lane == (uint32_t)q) mine = sum;
            }
        }
        return mine;
    };
    // lane q of `take` appends (score, doc) to query q's list if it beats the threshold
    auto append = [&](int32_t score, uint32_t doc, uint32_t take) {
        if (lane < tp::MAX_QB && (take >> lane & 1u)) {
            const uint64_t key = vec_key(score, doc);
            if (key > s_thr[lane]) {
                const uint32_t pos = atomicAdd(&s_cnt[lane], 1u);                 // < cap: cnt + INC <= cap stood at the last check
                s_buf[(size_t)lane * cap + pos] = key;
                if (pos + 1 + tp::INC > cap) s_sel[4 + chk % 3] = 1;
            }
        }
    };

    for (uint64_t grp = 0; grp < n_groups; grp++) {
        // ---- lane l: doc 64 (g_first + grp) + l, its tokens, and the queries of the block that may take it
        const uint64_t d = (g_first + grp) * 64 + lane;
        uint32_t T = 0, abits = 0;
        uint64_t first_tok = 0;
        if (d >= d_begin && d < d_end) {                                          // d + 1 <= n_docs
            first_tok = p.tok_ptr[d];
            T = (uint32_t)(p.tok_ptr[d + 1] - first_tok);                         // < 2^31: checked when the table was registered
            if (T) {
                abits = open_bits;
                const uint64_t wi = d >> 5;
                if (masked_bits && wi < p.mask_words) {
                    for (uint32_t ql = 0; ql < n_live; ql++) {
                        const int32_t mid = s_mid[ql];
                        if (mid >= 0) abits |= (p.masks[(uint64_t)mid * p.mask_words + wi] >> (d & 31u) & 1u) << ql;
                    }
                }
            }
        }
        // Every wave reads the same read-only words (cut, tok_ptr, masks, s_mid), so `cand` and `wide` are the same in all four: the
        // skip, the barriers below and the deal of the docs are uniform over the workgroup.
        const uint64_t cand = __ballot(abits != 0);
        if (!cand) continue;
        const uint64_t wide = __ballot(abits != 0 && T >= p.wide_tokens);         // (wide_tokens >= 1)
        // Check number chk reads flag chk % 3, the appends behind it raise flag (chk + 1) % 3, and thread 0 clears flag (chk + 2) % 3 —
        // read at the check before, raised again only behind the next one — so no thread can see a flag change between the barrier and
        // its own read: the branch is uniform.  Between two checks a query gains at most one key per doc of the group, INC in all.
        __syncthreads();                                                          // (every earlier append stands)
        const bool full = s_sel[4 + chk % 3] != 0;
        if (tid == 0) s_sel[4 + (chk + 2) % 3] = 0;
        chk++;
        if (full) {
            for (uint32_t ql = 0; ql < n_live; ql++) {
                const uint32_t n = s_cnt[ql];
                if (n + tp::INC > cap) vec_compact(s_buf + (size_t)ql * cap, n, k, &s_thr[ql], &s_cnt[ql], s_hist, s_sel, s_holes);
            }
        }
        // ---- pass 1: the docs one wave walks, dealt in turn
        uint32_t nth = 0;
        for (uint64_t left = cand & ~wide; left; left &= left - 1, nth++) {
            if ((nth & 3u) != wave) continue;
            const int i = __builtin_ctzll(left);
            const uint32_t Ti = __builtin_amdgcn_readfirstlane(__shfl(T, i));
            const uint32_t take = __builtin_amdgcn_readfirstlane(__shfl(abits, i));
            const uint64_t fi = (uint64_t)__builtin_amdgcn_readfirstlane(__shfl((uint32_t)first_tok, i)) |
                                (uint64_t)__builtin_amdgcn_readfirstlane(__shfl((uint32_t)(first_tok >> 32), i)) << 32;
            int32_t mx[tp::MAX_QB][QT];
#pragma unroll
            for (int q = 0; q < (int)tp::MAX_QB; q++)
#pragma unroll
                for (int j = 0; j < QT; j++) mx[q][j] = INT32_MIN;
            doc_maxima<QT>(p.tok + fi * dim, Ti, dim, b_ptr, p.row_stride, q_stride, 0, 1, take, qb, r, h, mx);
            const int32_t score = scores_of(mx, take, false);
            append(score, (uint32_t)((g_first + grp) * 64 + (uint32_t)i), take);
        }
        // ---- pass 2: the wide docs, every wave every fourth tile, the maxima joined in LDS
        for (uint64_t left = wide; left; left &= left - 1) {
            const int i = __builtin_ctzll(left);
            const uint32_t Ti = __builtin_amdgcn_readfirstlane(__shfl(T, i));
            const uint32_t take = __builtin_amdgcn_readfirstlane(__shfl(abits, i));
            const uint64_t fi = (uint64_t)__builtin_amdgcn_readfirstlane(__shfl((uint32_t)first_tok, i)) |
                                (uint64_t)__builtin_amdgcn_readfirstlane(__shfl((uint32_t)(first_tok >> 32), i)) << 32;
            int32_t mx[tp::MAX_QB][QT];
#pragma unroll
            for (int q = 0; q < (int)tp::MAX_QB; q++)
#pragma unroll
                for (int j = 0; j < QT; j++) mx[q][j] = INT32_MIN;
            doc_maxima<QT>(p.tok + fi * dim, Ti, dim, b_ptr, p.row_stride, q_stride, wave, mp::WAVES, take, qb, r, h, mx);
#pragma unroll
            for (int q = 0; q < (int)tp::MAX_QB; q++) {
                if (take >> q & 1u) {
#pragma unroll
                    for (int j = 0; j < QT; j++) {
                        int32_t v = max(mx[q][j], __shfl_xor(mx[q][j], 16));
                        v = max(v, __shfl_xor(v, 32));
                        if (h == 0) atomicMax(&s_join[(uint32_t)q * SLOTS + (uint32_t)j * 16 + r], v);   // (q < n_live <= qb)
                    }
                }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int q = 0; q < (int)tp::MAX_QB; q++) {
                    if (take >> q & 1u) {
#pragma unroll
                        for (int j = 0; j < QT; j++) {
                            mx[q][j] = s_join[(uint32_t)q * SLOTS + (uint32_t)j * 16 + r];
                        }
                    }
                }
                const int32_t score = scores_of(mx, take, true);
                append(score, (uint32_t)((g_first + grp) * 64 + (uint32_t)i), take);
#pragma unroll
                for (int q = 0; q < (int)tp::MAX_QB; q++) {
                    if (take >> q & 1u) {
#pragma unroll
                        for (int j = 0; j < QT; j++)
                            if (h == 0) s_join[(uint32_t)q * SLOTS + (uint32_t)j * 16 + r] = INT32_MIN;
                    }
                }
            }
            __syncthreads();                                                      // (s_join is INT32_MIN again for the next wide doc)
        }
    }
    // ---- the chunk's lists: at most k keys per query, the other slots 0
    __syncthreads();
    for (uint32_t ql = 0; ql < n_live; ql++) {
        uint32_t n = s_cnt[ql];
        if (n > k) {
            vec_compact(s_buf + (size_t)ql * cap, n, k, &s_thr[ql], &s_cnt[ql], s_hist, s_sel, s_holes);
            n = k;
        }
        uint64_t* const out = p.part + ((uint64_t)(q0 + ql) * p.n_chunks + chunk) * k;
        for (uint32_t i = tid; i < k; i += mp::TPB) out[i] = i < n ? s_buf[(size_t)ql * cap + i] : 0ull;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The dynamic LDS a kernel may ask for is an attribute of the function on a device, not of a scorer: the largest value any launch of
// this process has needed is kept per QT and set before every launch, attribute and launch under one lock, so that no other scorer or
// context can lower it in between.  (hipFuncSetAttribute is a host call: nothing is enqueued and nothing waits.)
std::mutex g_lds_mu;
int g_lds_most[5] = {0, 0, 0, 0, 0};

template <int QT>
int32_t launch_qt(ss_scorer* s, const MaxSimTopkParams& p, const tp::Block& b, const tp::Chunks& c, hipStream_t st) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(g_lds_mu);
    if (g_lds_most[QT] < (int)b.lds_bytes) g_lds_most[QT] = (int)b.lds_bytes;
    SS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_maxsim_topk<QT>), hipFuncAttributeMaxDynamicSharedMemorySize, g_lds_most[QT]));
    hipLaunchKernelGGL((k_maxsim_topk<QT>), dim3(c.n_chunks, c.n_qblocks), dim3(mp::TPB), b.lds_bytes, st, p);
    return SS_OK;
}

int32_t topk_impl(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, const int32_t* mask_id, int32_t k, ss_vec_hit* hits_out,
                  int32_t* n_hits_out) {
    static const char* const who = "ss_maxsim_topk";
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "%s: n_q < 0", who);
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "%s: k = %d must be >= 1", who, k);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: k = %d exceeds SS_MAX_TOPK = %d", who, k, SS_MAX_TOPK);
    if (n_q > 0 && (!hits_out || !n_hits_out)) return ctx->fail(SS_ERR_INVALID, "%s: hits_out or n_hits_out is NULL", who);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> h_qptr;
    uint32_t qt = 1;
    SS_TRY(ss::maxsim_check_query_tokens(ctx, who, n_q, qt_ptr, qtok, &h_qptr, &qt));
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
    if (s->tok_dim == 0) return ctx->fail(SS_ERR_STATE, "%s: no token table registered (ss_scorer_set_doc_tokens)", who);
    if (n_q == 0) return SS_OK;
    if (s->n_docs >> 32) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: 2^32 docs or more", who);
    int lds_limit = 0;
    SS_HIP(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const tp::Block b = tp::block((uint32_t)s->tok_dim, qt, (uint32_t)k, nq, (uint32_t)std::min(lds_limit, 160 << 10));
    if (!b.ok)
        return ctx->fail(SS_ERR_UNSUPPORTED, "%s: one query of %u token slots at k = %d and dim %d needs more than the device's %d bytes of LDS", who,
                         16 * qt, k, s->tok_dim, lds_limit);
    const tp::Chunks c = tp::chunks(s->tok_slices, nq, b.qb, (uint32_t)k, ctx->opt("maxsim.chunk_tokens", 0), (uint32_t)ctx->cu_count);
    if (c.too_large) return ctx->fail(SS_ERR_OOM, "%s: the partial lists of %zu queries over %u chunks do not fit", who, nq, c.n_chunks);
    if (!c.ok) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: %zu queries in blocks of %u need more query blocks or chunks than one launch holds", who, nq, b.qb);
    const bool run = c.n_chunks != 0 && !(masked && s->mask_words == 0);          // otherwise a table without a token: every row is empty
    if (run) {
        const hipError_t e = ensure(s->d_mst_part, (size_t)c.part_keys);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: no device memory for %llu partial keys", who,
                             (unsigned long long)c.part_keys);
        }
    }
    hipStream_t st = ctx->stream;
    const bool dev_h = ss::on_device(hits_out), dev_n = ss::on_device(n_hits_out);
    if (!dev_h) SS_HIP(ctx, ensure(s->d_mst_hits, nq * (size_t)k));
    if (!dev_n) SS_HIP(ctx, ensure(s->d_mst_n, nq));
    ss_vec_hit* const o_hits = dev_h ? hits_out : s->d_mst_hits.p;
    int32_t* const o_n = dev_n ? n_hits_out : s->d_mst_n.p;
    bool staged = false;
    if (!run) {
        SS_HIP(ctx, hipMemsetAsync(o_n, 0, nq * sizeof(int32_t), st));
    } else {
        MaxSimTopkParams p{};
        SS_TRY(ss::maxsim_query_tokens_to_device(s, h_qptr, qtok, &p.qtok, &staged));
        if (masked) {                                                             // the ids go up through a pinned block; its last reader is waited for first
            if (ss::on_device(mask_id)) p.q_mask = mask_id;
            else {
                SS_HIP(ctx, s->ev_mst_mid.wait());
                SS_HIP(ctx, s->h_mst_mid.ensure(nq * sizeof(int32_t)));
                SS_HIP(ctx, ensure(s->d_mst_mid, nq));
                std::memcpy(s->h_mst_mid.p, mid.data(), nq * sizeof(int32_t));
                SS_HIP(ctx, hipMemcpyAsync(s->d_mst_mid.p, s->h_mst_mid.p, nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
                SS_HIP(ctx, s->ev_mst_mid.record(st));
                p.q_mask = s->d_mst_mid.p;
            }
        }
        p.tok = s->tok.p;
        p.tok_ptr = s->tok_ptr.p;
        p.cut = s->tok_cut.p;
        p.n_slices = s->tok_slices;
        p.chunk_slices = c.chunk_slices;
        p.qt_ptr = s->d_ms_qptr.p;
        p.masks = s->masks.p;
        p.mask_words = s->mask_words;
        p.part = s->d_mst_part.p;
        p.dim = (uint32_t)s->tok_dim; p.n_q = (uint32_t)n_q; p.k = (uint32_t)k;
        p.qb = b.qb; p.n_chunks = c.n_chunks; p.cap = b.cap;
        p.row_stride = mp::row_stride(p.dim);
        p.wide_tokens = mp::wide_tokens_of(ctx->opt("maxsim.wide_tokens", 0));
        if (qt == 4) SS_TRY(launch_qt<4>(s, p, b, c, st));
        else if (qt == 2) SS_TRY(launch_qt<2>(s, p, b, c, st));
        else SS_TRY(launch_qt<1>(s, p, b, c, st));
        SS_HIP(ctx, hipGetLastError());
        ss::launch_vec_merge(s->d_mst_part.p, c.n_chunks, n_q, k, o_hits, o_n, st);
        SS_HIP(ctx, hipGetLastError());
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

}  // namespace

extern "C" {

int32_t ss_maxsim_topk(ss_scorer* s, int32_t n_q, const uint32_t* qt_ptr, const int8_t* qtok, const int32_t* mask_id, int32_t k, ss_vec_hit* hits_out,
                       int32_t* n_hits_out) {
    return hw::guarded(s, "ss_maxsim_topk", [&] { return topk_impl(s, n_q, qt_ptr, qtok, mask_id, k, hits_out, n_hits_out); });
}

}  // extern "C"
