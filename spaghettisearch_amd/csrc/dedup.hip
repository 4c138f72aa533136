// dedup.hip — ss_index_build_signatures / _drop_signatures / _read_signatures and ss_dedup_hits: a MinHash signature per doc and the
// walk that drops the near-duplicate rows of a result window.  A step file beside collapse.hip: one kernel behind
// whatever scoring call made the rows, no scoring kernel edited.  Integer arithmetic only: every result is defined bit for bit.
//
//   k_doc_signatures           one pass over the doc view (doc_ptr, doc_term; weights are not read).  A wave owns 64 / SG_GROUP docs
//                              that follow each other.  Rows of up to SG_GROUP_MAX terms: one group of SG_GROUP lanes each, all groups
//                              of the wave at once.  Longer rows of up to SG_WAVE_MAX terms: the whole wave, one row after the other.
//                              Rows beyond that: the row is filled with SS_SIG_EMPTY and its doc appended to a list.  Slots are made
//                              four at a time (a row's terms are read again per four slots, from L1 / L2: the pass is bound by the
//                              hash's integer ops, not by its loads), reduced with shuffles and stored as one 16-byte word.
//   k_doc_signatures_split     the listed rows in chunks of SG_CHUNK terms, a workgroup per chunk; the chunk's four minima per wave go
//                              into the row with atomicMin.  A minimum does not depend on the order of its operands: the bytes stay
//                              defined whatever order the list and the chunks come in.
//   k_read_signatures          sig_out[i] = sig[docs[i]]
//   k_dedup_hits               one workgroup per query.  The walk is sequential in j, but only inside a tile of 64 rows: for tile T every
//                              row first finds, in parallel, its smallest matching kept row among the EARLIER tiles (their kept rows
//                              are final and listed in LDS; the waves share the list), and the bits of the tile's own 64 x 64 match
//                              matrix (bit i of row j: i < j and match(i, j) >= min_match).  Then wave 0 resolves the tile in 64 ballot
//                              steps: row i is kept iff it has no leader in an earlier tile and none of the tile's kept rows so far
//                              is in its mask.  Two barriers per tile.  Signatures are read from global memory (a window's are at most
//                              128 KB, L2-resident; a leader's row is one address for the whole wave) by both instances: 1024 rows of 32
//                              slots do not fit a static LDS block.  Kept rows are numbered from the tiles' kept masks and copied
//                              out as collapse.hip does, five lanes to a row.
// The window in, the paging checks and the outputs' way back: hit_window.hpp.
#include "hit_window.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

// ---------------------------------------------------------------- signatures
constexpr uint32_t SG_GROUP = 8;                          // lanes of a sub-wave group
constexpr uint32_t SG_GROUP_MAX = 32;                     // rows of up to this many terms: one group
constexpr uint32_t SG_WAVE_MAX = 1024;                    // longer rows of up to this many terms: one wave
constexpr uint32_t SG_CHUNK = 4096;                       // rows beyond: chunks of this many terms, a workgroup each, joined by atomicMin
constexpr int SG_BLOCK = 256;
constexpr uint32_t SG_WAVES = SG_BLOCK / 64, SG_DOCS_PER_WAVE = 64 / SG_GROUP;
constexpr uint32_t SG_GOLD = 0x9E3779B9u;
static_assert(SS_MAX_SIG_SLOTS <= 64, "a wave fills a listed row with one store per lane");

__device__ __forceinline__ uint32_t sg_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the minima of slots sb .. sb + 3 over terms[first], terms[first + step], .. below len
__device__ __forceinline__ uint4 sg_minima(const uint32_t* __restrict__ terms, uint32_t first, uint32_t step, uint32_t len, uint32_t sb) {
    const uint32_t c0 = SG_GOLD * (sb + 1), c1 = SG_GOLD * (sb + 2), c2 = SG_GOLD * (sb + 3), c3 = SG_GOLD * (sb + 4);
    uint4 m = make_uint4(SS_SIG_EMPTY, SS_SIG_EMPTY, SS_SIG_EMPTY, SS_SIG_EMPTY);
    for (uint32_t j = first; j < len; j += step) {
        const uint32_t t = terms[j];
        m.x = umin32(m.x, sg_mix(t + c0));
        m.y = umin32(m.y, sg_mix(t + c1));
        m.z = umin32(m.z, sg_mix(t + c2));
        m.w = umin32(m.w, sg_mix(t + c3));
    }
    return m;
}
// the minimum over the lanes whose ids differ in the bits below `width` (a power of two <= 64)
__device__ __forceinline__ uint4 sg_reduce(uint4 m, int width) {
    for (int off = 1; off < width; off <<= 1) {
        m.x = umin32(m.x, __shfl_xor(m.x, off, 64));
        m.y = umin32(m.y, __shfl_xor(m.y, off, 64));
        m.z = umin32(m.z, __shfl_xor(m.z, off, 64));
        m.w = umin32(m.w, __shfl_xor(m.w, off, 64));
    }
    return m;
}

// sig [n_docs][n_slots] (n_slots a multiple of 4; rows 16-byte aligned).  long_list[0] counts the listed docs, long_list[1 ..
// long_cap] holds them (no more than long_cap rows can be longer than SG_WAVE_MAX: the host sized it from the posting count).
__global__ __launch_bounds__(SG_BLOCK) void k_doc_signatures(const uint64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ doc_term,
                                                             uint64_t n_docs, uint32_t n_slots, uint32_t* __restrict__ sig,
                                                             uint32_t* __restrict__ long_list, uint32_t long_cap) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = ((uint64_t)blockIdx.x * SG_WAVES + wave) * SG_DOCS_PER_WAVE;
    if (base >= n_docs) return;                           // (a whole wave leaves: no lane of it takes part in the shuffles below)
    const uint32_t grp = lane / SG_GROUP, sub = lane % SG_GROUP;
    const uint64_t d = base + grp;
    uint64_t b = 0;
    uint32_t len = 0;
    if (d < n_docs) {
        b = doc_ptr[d];
        len = (uint32_t)(doc_ptr[d + 1] - b);             // (the view holds fewer than 2^32 postings)
    }
    // ---- short rows: every group its own doc (an empty row comes out as SS_SIG_EMPTY throughout)
    const bool is_short = d < n_docs && len <= SG_GROUP_MAX;
    for (uint32_t sb = 0; sb < n_slots; sb += 4) {
        const uint4 m = sg_reduce(sg_minima(doc_term + b, sub, SG_GROUP, is_short ? len : 0u, sb), SG_GROUP);
        if (is_short && sub == 0) *reinterpret_cast<uint4*>(sig + d * n_slots + sb) = m;
    }
    // ---- the wave's longer rows, one after the other
    for (uint32_t r = 0; r < SG_DOCS_PER_WAVE; r++) {
        const uint64_t dr = base + r;
        if (dr >= n_docs) break;                          // (the same in every lane)
        const uint64_t br = __shfl(b, r * SG_GROUP, 64);
        const uint32_t lr = __shfl(len, r * SG_GROUP, 64);
        if (lr <= SG_GROUP_MAX) continue;
        if (lr <= SG_WAVE_MAX) {
            for (uint32_t sb = 0; sb < n_slots; sb += 4) {
                const uint4 m = sg_reduce(sg_minima(doc_term + br, lane, 64, lr, sb), 64);
                if (lane == 0) *reinterpret_cast<uint4*>(sig + dr * n_slots + sb) = m;
            }
        } else {
            if (lane < n_slots) sig[dr * n_slots + lane] = SS_SIG_EMPTY;
            if (lane == 0) {
                const uint32_t at = atomicAdd(long_list, 1u);
                if (at < long_cap) long_list[1 + at] = (uint32_t)dr;
            }
        }
    }
}

// Chunk c of listed row i goes to workgroup (c + i) mod gridDim.x: rows of a few chunks spread over the grid.
__global__ __launch_bounds__(SG_BLOCK) void k_doc_signatures_split(const uint64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ doc_term,
                                                                   uint32_t n_slots, uint32_t* __restrict__ sig,
                                                                   const uint32_t* __restrict__ long_list, uint32_t long_cap) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t listed = long_list[0] < long_cap ? long_list[0] : long_cap;
    for (uint32_t i = 0; i < listed; i++) {
        const uint64_t d = long_list[1 + i];
        const uint64_t b = doc_ptr[d];
        const uint32_t len = (uint32_t)(doc_ptr[d + 1] - b);
        const uint32_t n_chunks = (len + SG_CHUNK - 1) / SG_CHUNK;
        for (uint32_t c = (blockIdx.x + gridDim.x - i % gridDim.x) % gridDim.x; c < n_chunks; c += gridDim.x) {
            const uint32_t cb = c * SG_CHUNK, cl = len - cb < SG_CHUNK ? len - cb : SG_CHUNK;
            for (uint32_t sb = 0; sb < n_slots; sb += 4) {
                const uint4 m = sg_reduce(sg_minima(doc_term + b + cb, threadIdx.x, SG_BLOCK, cl, sb), 64);
                if (lane == 0) {
                    uint32_t* const row = sig + d * n_slots + sb;
                    atomicMin(row + 0, m.x);
                    atomicMin(row + 1, m.y);
                    atomicMin(row + 2, m.z);
                    atomicMin(row + 3, m.w);
                }
            }
        }
    }
}

constexpr int RD_TPB = 256;

// docs[] has been checked on the host (every id < n_docs)
__global__ __launch_bounds__(RD_TPB) void k_read_signatures(const uint32_t* __restrict__ sig, uint32_t n_slots, const uint32_t* __restrict__ docs,
                                                         uint64_t n_words, uint32_t* __restrict__ out) {
    const uint64_t x = (uint64_t)blockIdx.x * RD_TPB + threadIdx.x;
    if (x >= n_words) return;
    const uint64_t i = x / n_slots;
    out[x] = sig[(uint64_t)docs[i] * n_slots + (x - i * n_slots)];
}

int32_t build_signatures(ss_index* idx, int32_t n_slots) {
    ss_ctx* ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t N = idx->n_docs, P = idx->dv_term.n;
    idx->drop_signatures();                               // signatures that exist go FIRST (the header says so)
    ss::DevBuf<uint32_t> sig, long_list;
    const uint64_t long_cap = P / (SG_WAVE_MAX + 1) + 1;  // more rows than this cannot be longer than SG_WAVE_MAX
    SS_HIP(ctx, sig.alloc((size_t)N * (size_t)n_slots));
    SS_HIP(ctx, long_list.alloc((size_t)long_cap + 1));
    SS_HIP(ctx, hipMemsetAsync(long_list.p, 0, sizeof(uint32_t), st));
    if (N) {
        const unsigned grid = ss::div_up(N, SG_WAVES * SG_DOCS_PER_WAVE);
        hipLaunchKernelGGL(k_doc_signatures, dim3(grid), dim3(SG_BLOCK), 0, st, (const uint64_t*)idx->dv_ptr.p, (const uint32_t*)idx->dv_term.p,
                           N, (uint32_t)n_slots, sig.p, long_list.p, (uint32_t)long_cap);
        hipLaunchKernelGGL(k_doc_signatures_split, dim3((unsigned)std::max(ctx->cu_count, 1) * 4u), dim3(SG_BLOCK), 0, st,
                           (const uint64_t*)idx->dv_ptr.p, (const uint32_t*)idx->dv_term.p, (uint32_t)n_slots, sig.p,
                           (const uint32_t*)long_list.p, (uint32_t)long_cap);
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, hipStreamSynchronize(st));                // complete, and an error of the build reported, when the call returns
    idx->sig = std::move(sig);
    idx->sig_slots = n_slots;
    idx->has_signatures = true;
    return SS_OK;
}

int32_t read_signatures(ss_index* idx, uint64_t n, const uint32_t* docs, uint32_t* sig_out, int32_t* n_slots_out) {
    ss_ctx* ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t S = (uint32_t)idx->sig_slots;
    std::vector<uint32_t> h_docs(n);
    SS_HIP(ctx, ss::copy_in(st, h_docs.data(), docs, n * sizeof(uint32_t)));
    for (uint64_t i = 0; i < n; i++)
        if ((uint64_t)h_docs[i] >= idx->n_docs)
            return ctx->fail(SS_ERR_INVALID, "ss_index_read_signatures: docs[%llu] = %u, the table has %llu docs", (unsigned long long)i, h_docs[i],
                             (unsigned long long)idx->n_docs);
    if (n_slots_out) *n_slots_out = (int32_t)S;
    if (n == 0) return SS_OK;
    const bool dev_o = ss::on_device(sig_out);
    const uint64_t words = n * S;
    ss::DevBuf<uint32_t> d_docs, d_out;
    SS_HIP(ctx, d_docs.alloc(n));
    if (!dev_o) SS_HIP(ctx, d_out.alloc(words));
    SS_HIP(ctx, hipMemcpyAsync(d_docs.p, h_docs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_read_signatures, dim3(ss::div_up(words, RD_TPB)), dim3(RD_TPB), 0, st, (const uint32_t*)idx->sig.p, S,
                       (const uint32_t*)d_docs.p, words, dev_o ? sig_out : d_out.p);
    SS_HIP(ctx, hipGetLastError());
    if (!dev_o) SS_HIP(ctx, hipMemcpyAsync(sig_out, d_out.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));                // (h_docs and the device blocks outlive their copies)
    return SS_OK;
}

// ---------------------------------------------------------------- the walk over a window
constexpr uint32_t DD_NONE = 0xFFFFFFFFu;                 // s_doc of a row on its own (no doc id reaches it); s_lead of a row without a leader yet
constexpr uint32_t DD_TILE = 64;                          // rows of a tile: one per lane of the resolving wave, one bit each of a 64-bit mask
constexpr int DD_SLOT_WORDS = SS_MAX_SIG_SLOTS / 4;       // a signature as 16-byte words, at most

struct DedupParams {
    const uint32_t* sig;                                  // [n_docs][n_slots]
    uint64_t n_docs;
    uint32_t n_slots;
    const ss_hit* hits;                                   // [n_q][k_in]
    const int32_t* n_hits;                                // [n_q]
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;                                  // [n_q]
    uint32_t* sim_out;                                    // [n_q][k], nullable
    int32_t* n_kept_out;                                  // [n_q], nullable
    uint32_t k_in, min_match, first, k;
};

// the number of slots in which the row at `other` (the same address in every lane) equals `mine`
__device__ __forceinline__ uint32_t dd_match(const uint4* __restrict__ other, const uint4 (&mine)[DD_SLOT_WORDS], uint32_t nb) {
    uint32_t cnt = 0;
#pragma unroll
    for (int b = 0; b < DD_SLOT_WORDS; b++)
        if ((uint32_t)b < nb) {
            const uint4 v = other[b];
            cnt += (uint32_t)(v.x == mine[b].x) + (uint32_t)(v.y == mine[b].y) + (uint32_t)(v.z == mine[b].z) + (uint32_t)(v.w == mine[b].w);
        }
    return cnt;
}

// One workgroup of BLOCK threads per query; windows of up to CAP = PER * BLOCK rows (the launcher picks the instance by k_in).
template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_dedup_hits(DedupParams p) {
    constexpr uint32_t CAP = PER * BLOCK, WAVES = BLOCK / 64, TILES = CAP / DD_TILE, SLICE = DD_TILE / WAVES;
    static_assert(CAP % DD_TILE == 0 && DD_TILE % WAVES == 0, "whole tiles, and a tile's rows split evenly over the waves");
    __shared__ uint32_t s_doc[CAP];                       // by window index: the doc of a row with a signature, DD_NONE of a row on its own
    __shared__ uint32_t s_lead[CAP];                      // by window index: the row's leader (itself if kept)
    __shared__ uint32_t s_sim[CAP];                       // by window index: the rows led by this row
    __shared__ uint32_t s_list[CAP];                      // the kept rows that have a signature, ascending; afterwards the window row of every output slot
    __shared__ uint64_t s_kept[TILES];                    // per tile: bit l = row 64 * tile + l is kept
    __shared__ uint64_t s_mask[WAVES][DD_TILE];           // per wave: its slice of every row's mask over the tile's own rows
    __shared__ uint32_t s_n_list;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t nb = p.n_slots / 4;                    // <= DD_SLOT_WORDS: checked by the build
    const uint4* const sig4 = reinterpret_cast<const uint4*>(p.sig);
    // ---- which rows have a signature
    for (uint32_t j = tid; j < n; j += BLOCK) {
        const uint32_t d = rows[j].doc;
        uint32_t doc = DD_NONE;
        if ((uint64_t)d < p.n_docs) {
            uint32_t all = SS_SIG_EMPTY;
            for (uint32_t b = 0; b < nb; b++) {
                const uint4 v = sig4[(size_t)d * nb + b];
                all &= v.x & v.y & v.z & v.w;
            }
            if (all != SS_SIG_EMPTY) doc = d;
        }
        s_doc[j] = doc;
        s_lead[j] = DD_NONE;
        s_sim[j] = 0;
    }
    if (tid == 0) s_n_list = 0;
    __syncthreads();
    const uint32_t n_tiles = (n + DD_TILE - 1) / DD_TILE; // <= TILES
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
        const uint32_t base = tile * DD_TILE, j = base + lane;   // j < CAP
        const bool live = j < n;
        const uint32_t dj = live ? s_doc[j] : DD_NONE;
        const bool has = dj != DD_NONE;
        uint4 mine[DD_SLOT_WORDS];
#pragma unroll
        for (int b = 0; b < DD_SLOT_WORDS; b++) {
            mine[b] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint32_t)b < nb && has) mine[b] = sig4[(size_t)dj * nb + b];
        }
        // ---- the smallest matching kept row of the earlier tiles: wave w takes entries w, w + WAVES, .. of the list
        const uint32_t n_list = s_n_list;
        uint32_t found = DD_NONE;
        for (uint32_t e = wave; e < n_list; e += WAVES) {
            if (__ballot(has && found == DD_NONE) == 0ull) break;
            const uint32_t di = __builtin_amdgcn_readfirstlane(s_doc[s_list[e]]);   // (listed rows have a signature)
            const uint32_t cnt = dd_match(sig4 + (size_t)di * nb, mine, nb);
            if (has && found == DD_NONE && cnt >= p.min_match) found = s_list[e];
        }
        if (found != DD_NONE) atomicMin(&s_lead[j], found);
        // ---- this wave's slice of the tile's own match matrix
        uint64_t part = 0;
        for (uint32_t x = 0; x < SLICE; x++) {
            const uint32_t il = wave * SLICE + x, i = base + il;
            if (i >= n) break;                            // (the same in every lane)
            const uint32_t di = __builtin_amdgcn_readfirstlane(s_doc[i]);
            if (di == DD_NONE) continue;
            const uint32_t cnt = dd_match(sig4 + (size_t)di * nb, mine, nb);
            if (has && lane > il && cnt >= p.min_match) part |= 1ull << il;
        }
        s_mask[wave][lane] = part;
        __syncthreads();
        // ---- wave 0 walks the tile
        if (wave == 0) {
            uint64_t mask = 0;
#pragma unroll
            for (uint32_t w = 0; w < WAVES; w++) mask |= s_mask[w][lane];
            const uint32_t pre = live ? s_lead[j] : DD_NONE;
            uint64_t kept = 0;                            // (the same in every lane)
            for (uint32_t i = 0; i < DD_TILE; i++)
                kept |= __ballot(lane == i && live && pre == DD_NONE && (mask & kept) == 0ull);
            const bool is_kept = (kept >> lane) & 1ull;
            if (live) s_lead[j] = is_kept ? j : pre != DD_NONE ? pre : base + (uint32_t)__ffsll((long long)(mask & kept)) - 1u;
            const uint64_t listed = __ballot(is_kept && has);
            if (is_kept && has) s_list[n_list + (uint32_t)__popcll(listed & ((1ull << lane) - 1ull))] = j;
            if (lane == 0) {
                s_kept[tile] = kept;
                s_n_list = n_list + (uint32_t)__popcll(listed);
            }
        }
        __syncthreads();
    }
    // ---- how many rows every row leads; the kept rows' numbers from the tiles' masks
    for (uint32_t j = tid; j < n; j += BLOCK) atomicAdd(&s_sim[s_lead[j]], 1u);
    uint32_t n_kept = 0;
    for (uint32_t t = 0; t < n_tiles; t++) n_kept += (uint32_t)__popcll(s_kept[t]);
    const uint32_t n_out = hw::page_len(n_kept, p.first, p.k);                   // <= k, <= n
    uint32_t* const s_src = s_list;                       // [n_out], n_out <= n <= CAP (the list was last read before the last barrier)
    for (uint32_t j = tid; j < n; j += BLOCK) {
        const uint32_t t = j / DD_TILE, l = j % DD_TILE;
        const uint64_t w = s_kept[t];
        if (!((w >> l) & 1ull)) continue;
        uint32_t pos = (uint32_t)__popcll(w & ((1ull << l) - 1ull));
        for (uint32_t u = 0; u < t; u++) pos += (uint32_t)__popcll(s_kept[u]);
        if (pos >= p.first && pos - p.first < n_out) s_src[pos - p.first] = j;
    }
    __syncthreads();
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_src[r]; });
    if (p.sim_out)
        for (uint32_t r = tid; r < n_out; r += BLOCK) p.sim_out[(size_t)q * p.k + r] = s_sim[s_src[r]];
    if (tid == 0) {
        p.n_hits_out[q] = (int32_t)n_out;
        if (p.n_kept_out) p.n_kept_out[q] = (int32_t)n_kept;
    }
}

// windows of up to 128 rows: one wave, two tiles; longer ones: four waves, up to sixteen tiles (the cut of k_collapse_hits)
constexpr int DD_SMALL = 64, DD_SMALL_PER = 2, DD_LARGE = 256, DD_LARGE_PER = 4;
static_assert(DD_LARGE * DD_LARGE_PER >= SS_MAX_TOPK, "k_dedup_hits holds a whole window's state in LDS");

int32_t dedup_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t min_match, int32_t first,
                   int32_t k, ss_hit* hits_out, int32_t* n_hits_out, uint32_t* similar_out, int32_t* n_kept_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, "ss_dedup_hits", "k_in", n_q, k_in, k, first, "min_match", min_match));
    SS_TRY(hw::check_page_arrays(ctx, "ss_dedup_hits", n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    const ss_index* const body = s->body;
    if (!body->has_signatures) return ctx->fail(SS_ERR_STATE, "ss_dedup_hits: the body table has no signatures (ss_index_build_signatures)");
    if (min_match > body->sig_slots)
        return ctx->fail(SS_ERR_INVALID, "ss_dedup_hits: min_match = %d, the signatures have %d slots", min_match, body->sig_slots);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_dedup_hits", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)n_q, (size_t)k, hits_out, n_hits_out, n_kept_out, similar_out, sizeof(uint32_t), &o));
    DedupParams p{};
    p.sig = body->sig.p;
    p.n_docs = body->n_docs;
    p.n_slots = (uint32_t)body->sig_slots;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.sim_out = static_cast<uint32_t*>(o.extra);
    p.n_kept_out = o.n_kept;
    p.k_in = (uint32_t)k_in; p.min_match = (uint32_t)min_match; p.first = (uint32_t)first; p.k = (uint32_t)k;
    if (k_in <= DD_SMALL * DD_SMALL_PER)
        hipLaunchKernelGGL((k_dedup_hits<DD_SMALL, DD_SMALL_PER>), dim3((unsigned)n_q), dim3(DD_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_dedup_hits<DD_LARGE, DD_LARGE_PER>), dim3((unsigned)n_q), dim3(DD_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    return hw::rows_out_finish(s, o, w.staged);
}

}  // namespace

extern "C" {

int32_t ss_index_build_signatures(ss_index* idx, int32_t n_slots) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_slots > SS_MAX_SIG_SLOTS) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_index_build_signatures: n_slots = %d exceeds SS_MAX_SIG_SLOTS = %d", n_slots, SS_MAX_SIG_SLOTS);
    if (n_slots < 4 || n_slots % 4) return ctx->fail(SS_ERR_INVALID, "ss_index_build_signatures: n_slots = %d is not one of 4, 8, .., %d", n_slots, SS_MAX_SIG_SLOTS);
    if (!idx->has_doc_view) return ctx->fail(SS_ERR_STATE, "ss_index_build_signatures: the table has no doc view (ss_index_build_doc_view)");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    return build_signatures(idx, n_slots);
}

int32_t ss_index_drop_signatures(ss_index* idx) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->has_signatures) return ctx->fail(SS_ERR_STATE, "ss_index_drop_signatures: the table has no signatures");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    idx->drop_signatures();
    return SS_OK;
}

int32_t ss_index_read_signatures(ss_index* idx, uint64_t n, const uint32_t* docs, uint32_t* sig_out, int32_t* n_slots_out) {
    if (!idx) return SS_ERR_INVALID;
    ss_ctx* ctx = idx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!idx->has_signatures) return ctx->fail(SS_ERR_STATE, "ss_index_read_signatures: the table has no signatures (ss_index_build_signatures)");
    if (n && (!docs || !sig_out)) return ctx->fail(SS_ERR_INVALID, "ss_index_read_signatures: NULL argument");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    return hw::guarded(ctx, "ss_index_read_signatures", [&] { return read_signatures(idx, n, docs, sig_out, n_slots_out); });
}

int32_t ss_dedup_hits(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t min_match, int32_t first,
                      int32_t k, ss_hit* hits_out, int32_t* n_hits_out, uint32_t* similar_out, int32_t* n_kept_out) {
    return hw::guarded(s, "ss_dedup_hits", [&] { return dedup_impl(s, n_q, k_in, hits, n_hits, min_match, first, k, hits_out, n_hits_out, similar_out, n_kept_out); });
}

}  // extern "C"
