// lexicon.hip — the term lexicon: the words of forw[0] keyed by term id, resident on the device.  The word list by
// prefix (the reference's /wordlist/{pre}, cmd/server/server.go:54-85, a scan of the whole vocabulary per request there) and spelling
// suggestions (no reference counterpart).  A step of its own beside the scorer: no existing kernel is edited.
//
//   ss_lexicon_create          checks, then on the host (lexicon_plan.hpp): the sort order, the ids grouped by word length and the words
//                              of every group re-packed at one stride; all of it uploaded.
//   k_lexicon_gather_freq      freq in grouped order (create and ss_lexicon_set_freq).
//   k_lexicon_prefix           one wave per prefix: lower and upper bound of the prefix in the sort order (the wave compares 64 bytes
//                              at a time, unsigned), then the page.
//   k_lexicon_suggest<W>       one wave (a workgroup of 64) per (query word, chunk of "lexicon.chunk_terms" grouped words).  A lane owns
//                              one word at a time: a banded optimal-string-alignment DP of width 2 W + 1 in registers, two rows back for
//                              the swap, dead as soon as a whole band row exceeds W.  The query byte of a row is the same in every lane
//                              (v_readlane); the word's bytes arrive one dword per four rows.  Survivors get the key
//                              (dist << 32 | ~freq, id); the wave keeps its 64 best keys sorted, one per lane (bitonic sort of the new
//                              keys + one bitonic merge, shuffles only: no LDS, no atomics), and writes the first m.
//   k_lexicon_merge            one wave per query word merges its chunks' lists the same way and writes the row.
//   k_lexicon_complete_bounds  one wave per prefix: the two bounds of k_lexicon_prefix, written as {lb, ub}.
//   k_lexicon_complete         one wave per (prefix, part): the range [lb, ub) of every prefix is cut into P near-equal parts (P from the
//                              number of prefixes alone, lexicon_plan.hpp).  The wave streams its part of the frequencies in sort order (16 B
//                              per lane where the position is a multiple of 4, a ragged head and tail one dword per lane) and keeps
//                              its best keys (~freq << 32 | position) sorted, one per lane; a step none of whose keys is below the
//                              wave's m-th best so far costs one ballot: no sort, no merge.  Writes its first m keys.
//   k_lexicon_complete_merge   one wave per prefix merges the P lists and writes the row, n_out and n_match_out.
// Device outputs: the calls only enqueue on the context's stream.  Host outputs go through lexicon-owned device blocks and only the
// entries the definition names are copied back.
#include "common.hpp"
#include "lexicon_plan.hpp"

#include <algorithm>
#include <new>

namespace {

using ss::lex::MAX_WORD;
using ss::lex::N_STARTS;

constexpr int LX_TPB = 64;                                // one wave
constexpr int LX_TURNS = 3;                               // as ss_scorer::TURNS: the host runs at most this many calls ahead
constexpr uint64_t LX_INF_A = ~0ull;                      // key of "no candidate" (a real key's high word is below 2^34)
constexpr uint32_t LX_INF_ID = ~0u;
constexpr int LX_DEAD = 1000;                             // a DP cell outside the band or the matrix
constexpr int64_t LX_CHUNK_DEFAULT = 4096, LX_CHUNK_MAX = 1 << 20;

template <typename T>
inline hipError_t ensure(ss::DevBuf<T>& b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    return b.alloc(n + n / 2 + 16);                       // (releasing the old block waits for the device: ss::pool_free)
}

// The queries of a call go up through the pinned block of one of LX_TURNS turns, rewritten only after the wait for the turn's event,
// recorded behind the kernel that read its device copy: the call never waits for its own copy.
struct LexTurn {
    ss::PinBuf h_q;
    ss::DevBuf<uint32_t> d_q;
    ss::Event ev;
};

}  // namespace

struct ss_lexicon {
    ss_ctx* ctx = nullptr;
    uint64_t n_terms = 0, n_bytes = 0;
    uint32_t n_grouped = 0;                               // words of at most SS_MAX_WORD_BYTES bytes
    uint32_t start[N_STARTS] = {};                        // host copy of d_start (the chunk plan of a suggest call is made on the CPU)
    ss::DevBuf<uint32_t> d_off;                           // [n_terms + 1] word starts
    ss::DevBuf<uint8_t> d_bytes;
    ss::DevBuf<uint32_t> d_order;                         // [n_terms] the sort order
    ss::DevBuf<uint32_t> d_ofreq;                         // [n_terms] freq in sort order: d_ofreq[pos] = freq[d_order[pos]]
    ss::DevBuf<uint32_t> d_gterm, d_gfreq, d_gwords;      // grouped by (length, id): ids, freq, the words at the group's stride
    ss::DevBuf<uint32_t> d_start;                         // [N_STARTS]
    ss::DevBuf<uint64_t> d_base;                          // [N_STARTS]
    LexTurn turn[LX_TURNS];
    int next_turn = 0;
    // the chunks' lists of a suggest call: written and read on the context's stream only (grow-only)
    ss::DevBuf<uint64_t> d_part_a;
    ss::DevBuf<uint32_t> d_part_id, d_part_n;
    // the parts' lists and the bounds of a complete call, the same way
    ss::DevBuf<uint64_t> d_cpl_key;
    ss::DevBuf<uint32_t> d_cpl_bounds;
    // device blocks of HOST outputs (grow-only; a call that uses one waits before it returns)
    ss::DevBuf<uint32_t> d_out_terms, d_out_freq;
    ss::DevBuf<int32_t> d_out_dist, d_out_n;
    ss::DevBuf<uint64_t> d_out_match;
};

namespace {

__device__ __forceinline__ bool key_less(uint64_t a1, uint32_t id1, uint64_t a2, uint32_t id2) {
    return a1 != a2 ? a1 < a2 : id1 < id2;
}
// the wave's 64 keys, one per lane, ascending by lane afterwards (bitonic network; equal keys are padding and may swap freely)
__device__ __forceinline__ void wave_sort(uint64_t& a, uint32_t& id, uint32_t lane) {
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint64_t pa = __shfl_xor(a, (int)j, 64);
            const uint32_t pid = __shfl_xor(id, (int)j, 64);
            const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
            if (take_min == key_less(pa, pid, a, id)) { a = pa; id = pid; }
        }
}
// best and fresh both ascending by lane: best becomes the 64 smallest of the 128, ascending
__device__ __forceinline__ void wave_merge(uint64_t& a, uint32_t& id, uint64_t na, uint32_t nid, uint32_t lane) {
    const uint64_t ra = __shfl(na, 63 - (int)lane, 64);
    const uint32_t rid = __shfl(nid, 63 - (int)lane, 64);
    if (key_less(ra, rid, a, id)) { a = ra; id = rid; }   // a bitonic sequence of the 64 smallest
    for (uint32_t j = 32; j > 0; j >>= 1) {
        const uint64_t pa = __shfl_xor(a, (int)j, 64);
        const uint32_t pid = __shfl_xor(id, (int)j, 64);
        if (((lane & j) == 0) == key_less(pa, pid, a, id)) { a = pa; id = pid; }
    }
}

__global__ __launch_bounds__(256) void k_lexicon_gather_freq(const uint32_t* __restrict__ gterm, const uint32_t* __restrict__ freq,
                                                             uint32_t* __restrict__ gfreq, uint32_t n) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) gfreq[g] = freq[gterm[g]];
}

// ---- prefix -----------------------------------------------------------------------------------------------------------------------
struct PrefixParams {
    const uint32_t* off;                                  // [n_terms + 1]
    const uint8_t* bytes;
    const uint32_t* order;                                // [n_terms]
    const uint32_t* q;                                    // the call's table: {offset, length} [n_q] | prefix bytes
    uint32_t n_terms, n_q, k;
    int64_t first;
    uint32_t* terms_out;                                  // [n_q][k]
    int32_t* n_out;                                       // [n_q]
    uint64_t* n_match_out;                                // [n_q] or NULL
};

// the word at sort position `pos`, cut to the prefix's length, against the prefix: -1 below, 0 the word starts with it, +1 above
// (the whole wave calls it with the same pos)
__device__ __forceinline__ int prefix_cmp(const PrefixParams& p, uint32_t pos, const uint8_t* pre, uint32_t lp, uint32_t lane) {
    const uint32_t t = p.order[pos];
    const uint32_t wo = p.off[t], wl = p.off[t + 1] - wo;
    const uint32_t n = wl < lp ? wl : lp;
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        const uint32_t i = k0 + lane;
        const uint32_t wb = i < n ? p.bytes[(size_t)wo + i] : 0u;
        const uint32_t pb = i < n ? pre[i] : 0u;
        const uint64_t diff = __ballot(wb != pb);
        if (diff) {
            const int l = __ffsll((unsigned long long)diff) - 1;
            return __shfl(wb, l, 64) < __shfl(pb, l, 64) ? -1 : 1;
        }
    }
    return wl >= lp ? 0 : -1;                             // a proper prefix of the prefix sorts before it
}

__global__ __launch_bounds__(LX_TPB) void k_lexicon_prefix(PrefixParams p) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t lp = p.q[2 * q + 1];
    const uint8_t* pre = reinterpret_cast<const uint8_t*>(p.q + 2 * (size_t)p.n_q) + p.q[2 * q];
    uint32_t lo = 0, hi = p.n_terms;                      // first position whose word is not below the prefix
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix_cmp(p, mid, pre, lp, lane) < 0) lo = mid + 1; else hi = mid;
    }
    const uint32_t lb = lo;
    hi = p.n_terms;                                       // first position whose word is above every word with the prefix
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix_cmp(p, mid, pre, lp, lane) <= 0) lo = mid + 1; else hi = mid;
    }
    const uint64_t n_match = lo - lb;
    const uint64_t first = (uint64_t)p.first;             // (>= 0: checked on the host)
    const uint32_t cnt = first >= n_match ? 0u : (uint32_t)(n_match - first < (uint64_t)p.k ? n_match - first : (uint64_t)p.k);
    for (uint32_t r = lane; r < cnt; r += 64) p.terms_out[(size_t)q * p.k + r] = p.order[lb + (uint32_t)first + r];
    if (lane == 0) {
        p.n_out[q] = (int32_t)cnt;
        if (p.n_match_out) p.n_match_out[q] = n_match;
    }
}

// ---- complete ---------------------------------------------------------------------------------------------------------------------
struct CompleteParams {
    PrefixParams lex;                                     // the lexicon, the call's table and the outputs as k_lexicon_prefix takes them (k = m)
    const uint32_t* ofreq;                                // [n_terms] freq in sort order
    uint32_t* bounds;                                     // [n_q] {lb, ub}
    uint64_t* part_key;                                   // [n_q][P][m] the parts' best keys, ascending, LX_INF_A behind the last
    uint32_t* freq_out;                                   // [n_q][m] or NULL
    uint32_t P, min_freq;
};

// the two searches of k_lexicon_prefix: [*lb, *ub) = the sort positions whose word starts with prefix q
__device__ __forceinline__ void prefix_bounds(const PrefixParams& p, uint32_t q, uint32_t lane, uint32_t* lb, uint32_t* ub) {
    const uint32_t lp = p.q[2 * q + 1];
    const uint8_t* pre = reinterpret_cast<const uint8_t*>(p.q + 2 * (size_t)p.n_q) + p.q[2 * q];
    uint32_t lo = 0, hi = p.n_terms;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix_cmp(p, mid, pre, lp, lane) < 0) lo = mid + 1; else hi = mid;
    }
    *lb = lo;
    hi = p.n_terms;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix_cmp(p, mid, pre, lp, lane) <= 0) lo = mid + 1; else hi = mid;
    }
    *ub = lo;
}

__global__ __launch_bounds__(LX_TPB) void k_lexicon_complete_bounds(CompleteParams p) {
    uint32_t lb, ub;
    prefix_bounds(p.lex, blockIdx.x, threadIdx.x, &lb, &ub);
    if (threadIdx.x == 0) {
        p.bounds[2 * (size_t)blockIdx.x] = lb;
        p.bounds[2 * (size_t)blockIdx.x + 1] = ub;
    }
}

// The wave's list of a complete call: its best keys ascending by lane, and `thr`, the m-th of them (LX_INF_A while there are fewer):
// a key that is not below thr cannot be in the row.  Keys are distinct (the position is part of the key), so the id word of
// wave_sort / wave_merge only repeats the key's low word.
struct CompleteList {
    uint64_t best = LX_INF_A, thr = LX_INF_A;
    uint32_t best_id = LX_INF_ID;
    // one key per lane (LX_INF_A: none); the whole wave calls it
    __device__ __forceinline__ void offer(uint64_t na, uint32_t m, uint32_t lane) {
        if (na >= thr) na = LX_INF_A;
        if (!__any(na != LX_INF_A)) return;
        uint32_t nid = na != LX_INF_A ? (uint32_t)na : LX_INF_ID;
        wave_sort(na, nid, lane);
        wave_merge(best, best_id, na, nid, lane);
        thr = __shfl(best, (int)m - 1, 64);
    }
};
__device__ __forceinline__ uint64_t complete_key(uint32_t freq, uint32_t pos, uint32_t min_freq) {
    return freq >= min_freq ? ((uint64_t)~freq << 32) | (uint64_t)pos : LX_INF_A;
}

__global__ __launch_bounds__(LX_TPB) void k_lexicon_complete(CompleteParams p) {
    const uint32_t wi = blockIdx.x, lane = threadIdx.x, m = p.lex.k;
    const uint32_t q = wi / p.P, part = wi - q * p.P;
    const uint32_t lb = p.bounds[2 * (size_t)q], ub = p.bounds[2 * (size_t)q + 1];
    uint32_t begin, end32;
    ss::lex::complete_part(lb, ub, p.P, part, &begin, &end32);
    // (positions as 64-bit values: begin + 3 and pos + 256 may pass 2^32 in a lexicon of nearly 2^32 terms)
    uint64_t pos = begin;
    const uint64_t end = end32;
    CompleteList list;
    uint64_t al = (pos + 3) & ~3ull;                      // the ragged head: up to the first position that is a multiple of 4
    if (al > end) al = end;
    if (pos < al) {
        const uint64_t x = pos + lane;
        list.offer(x < al ? complete_key(p.ofreq[x], (uint32_t)x, p.min_freq) : LX_INF_A, m, lane);
        pos = al;
    }
    for (; pos + 256 <= end; pos += 256) {                // 1 KiB per step: lane l holds positions pos + 4 l .. pos + 4 l + 3
        const uint32_t x = (uint32_t)pos + 4u * lane;
        const uint4 f = *reinterpret_cast<const uint4*>(p.ofreq + pos + 4u * lane);
        // the lane's largest freq at its first position is a lower bound of its four keys
        const uint32_t fmax = max(max(f.x, f.y), max(f.z, f.w));
        if (!__any(complete_key(fmax, x, p.min_freq) < list.thr)) continue;
        list.offer(complete_key(f.x, x, p.min_freq), m, lane);
        list.offer(complete_key(f.y, x + 1u, p.min_freq), m, lane);
        list.offer(complete_key(f.z, x + 2u, p.min_freq), m, lane);
        list.offer(complete_key(f.w, x + 3u, p.min_freq), m, lane);
    }
    for (; pos < end; pos += 64) {                        // the tail: fewer than 256 positions
        const uint64_t x = pos + lane;
        list.offer(x < end ? complete_key(p.ofreq[x], (uint32_t)x, p.min_freq) : LX_INF_A, m, lane);
    }
    if (lane < m) p.part_key[(size_t)wi * m + lane] = list.best;
}

__global__ __launch_bounds__(LX_TPB) void k_lexicon_complete_merge(CompleteParams p) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x, m = p.lex.k;
    const uint64_t* keys = p.part_key + (size_t)q * p.P * m;
    const uint32_t n = p.P * m;                           // (at most 256 * 64)
    CompleteList list;
    for (uint32_t e = 0; e < n; e += 64) list.offer(e + lane < n ? keys[e + lane] : LX_INF_A, m, lane);
    const bool keep = lane < m && list.best != LX_INF_A;
    const uint64_t kept = __ballot(keep);
    if (keep) {
        p.lex.terms_out[(size_t)q * m + lane] = p.lex.order[(uint32_t)list.best];
        if (p.freq_out) p.freq_out[(size_t)q * m + lane] = ~(uint32_t)(list.best >> 32);
    }
    if (lane == 0) {
        p.lex.n_out[q] = (int32_t)__popcll((unsigned long long)kept);
        if (p.lex.n_match_out) p.lex.n_match_out[q] = (uint64_t)(p.bounds[2 * (size_t)q + 1] - p.bounds[2 * (size_t)q]);
    }
}

// ---- suggest ----------------------------------------------------------------------------------------------------------------------
struct SuggestParams {
    const uint32_t *gterm, *gfreq, *gwords, *start;       // the grouped layout (lexicon_plan.hpp)
    const uint64_t* base;
    const uint32_t* qinfo;                                // the call's table: {byte offset, length, lo, hi} [n_q] | cbase [n_q + 1] | query bytes
    const uint32_t* cbase;                                // cbase[q] = the chunks of the queries before q
    const uint8_t* qbytes;
    uint64_t* part_a;                                     // [chunks][m] the chunks' best keys, ascending
    uint32_t* part_id;
    uint32_t* part_n;                                     // [chunks] how many of them are keys
    uint32_t n_q, chunk, m, min_freq;
    uint32_t* terms_out;                                  // [n_q][m]
    int32_t* dist_out;                                    // [n_q][m] or NULL
    int32_t* n_out;                                       // [n_q]
};

template <int W>
__global__ __launch_bounds__(LX_TPB) void k_lexicon_suggest(SuggestParams p) {
    constexpr int B = 2 * W + 1;                          // band cells of a row: columns i - W .. i + W
    const uint32_t wi = blockIdx.x, lane = threadIdx.x;
    uint32_t q = 0, qh = p.n_q;                           // the last query whose chunks begin at or before this one
    while (qh - q > 1) {
        const uint32_t mid = q + ((qh - q) >> 1);
        if (p.cbase[mid] <= wi) q = mid; else qh = mid;
    }
    const uint32_t la = p.qinfo[4 * q + 1], lo = p.qinfo[4 * q + 2], hi = p.qinfo[4 * q + 3];
    const uint32_t c0 = lo + (wi - p.cbase[q]) * p.chunk; // (< hi: the host made ceil((hi - lo) / chunk) chunks)
    const uint32_t c1 = hi - c0 < p.chunk ? hi : c0 + p.chunk;
    const int aq = lane < la ? (int)p.qbytes[p.qinfo[4 * q] + lane] : 0;      // lane i holds byte i of the query word (la <= 64)
    // the length groups of the range: L0 .. L0 + n_len - 1, at most B of them
    const uint32_t l0 = la > (uint32_t)W ? la - (uint32_t)W : 0u;
    const uint32_t l1 = la + (uint32_t)W < MAX_WORD ? la + (uint32_t)W : MAX_WORD;
    uint32_t gs[B];
    uint64_t gb[B];
#pragma unroll
    for (int x = 0; x < B; x++) {
        const uint32_t L = l0 + (uint32_t)x <= l1 ? l0 + (uint32_t)x : l1;
        gs[x] = p.start[L];
        gb[x] = p.base[L];
    }
    uint64_t best_a = LX_INF_A;
    uint32_t best_id = LX_INF_ID;
    for (uint32_t base = c0; base < c1; base += 64) {     // (c1 - c0 <= 2^20: no wrap short of 2^32 - 64 grouped words; the host refuses more)
        const uint32_t g = base + lane;
        bool alive = g < c1;
        uint32_t lb = l0, gs_b = gs[0];
        uint64_t gb_b = gb[0];
#pragma unroll
        for (int x = 1; x < B; x++)
            if (l0 + (uint32_t)x <= l1 && g >= gs[x]) { lb = l0 + (uint32_t)x; gs_b = gs[x]; gb_b = gb[x]; }
        const uint32_t freq = alive ? p.gfreq[g] : 0u;
        alive = alive && freq >= p.min_freq;
        const uint64_t wb = gb_b + (uint64_t)(g - gs_b) * ((lb + 3u) >> 2);
        // ---- banded DP: row r cell c is column r - W + c; prev = row i - 1, prev2 = row i - 2
        int prev[B], prev2[B], cur[B];
        uint32_t win[B + 1];                              // win[x] = word byte i - W - 2 + x at row i
#pragma unroll
        for (int c = 0; c < B; c++) {
            const int col = c - W;
            prev[c] = col >= 0 && (uint32_t)col <= lb ? col : LX_DEAD;
            prev2[c] = LX_DEAD;
            cur[c] = LX_DEAD;
        }
#pragma unroll
        for (int x = 0; x <= B; x++) win[x] = 0x100u;
        uint32_t cw = 0;
        auto push = [&](uint32_t nb) {                    // the word's byte nb (the same nb in every lane, ascending from 0)
            if ((nb & 3u) == 0) cw = alive && nb < lb ? p.gwords[wb + (nb >> 2)] : 0u;
#pragma unroll
            for (int x = 0; x < B; x++) win[x] = win[x + 1];
            win[B] = (cw >> (8u * (nb & 3u))) & 0xFFu;
        };
        for (uint32_t nb = 0; nb < (uint32_t)W; nb++) push(nb);
        for (uint32_t i = 1; i <= la; i++) {
            if (!__any(alive)) break;
            push(i + (uint32_t)W - 1u);
            const int ai = __builtin_amdgcn_readlane(aq, (int)i - 1);
            const int ai2 = i >= 2 ? __builtin_amdgcn_readlane(aq, (int)i - 2) : 0x200;
            int row_min = LX_DEAD;
#pragma unroll
            for (int c = 0; c < B; c++) {
                const int j = (int)i - W + c;
                int v;
                if (j < 0 || j > (int)lb) v = LX_DEAD;
                else if (j == 0) v = (int)i;
                else {
                    const int bj = (int)win[c + 1], bj2 = (int)win[c];
                    v = prev[c] + (ai != bj ? 1 : 0);
                    if (c + 1 < B) v = min(v, prev[c + 1] + 1);
                    if (c >= 1) v = min(v, cur[c - 1] + 1);
                    if (j >= 2 && ai == bj2 && ai2 == bj) v = min(v, prev2[c] + 1);
                }
                cur[c] = v;
                row_min = min(row_min, v);
            }
            if (row_min > W) alive = false;               // no later row comes back under W: a row's minimum never decreases
#pragma unroll
            for (int c = 0; c < B; c++) { prev2[c] = prev[c]; prev[c] = cur[c]; }
        }
        int d = LX_DEAD;
        const int cf = (int)lb - (int)la + W;             // column lb of row la (0 .. 2 W: the groups of the range)
#pragma unroll
        for (int c = 0; c < B; c++)
            if (c == cf) d = prev[c];
        const bool cand = alive && d <= W;
        // ---- the wave's best keys
        uint64_t na = cand ? ((uint64_t)(uint32_t)d << 32) | (uint64_t)(uint32_t)~freq : LX_INF_A;
        uint32_t nid = cand ? p.gterm[g] : LX_INF_ID;
        const uint64_t ta = __shfl(best_a, (int)p.m - 1, 64); // worse than the m-th best so far: cannot be in the row
        const uint32_t tid = __shfl(best_id, (int)p.m - 1, 64);
        if (!key_less(na, nid, ta, tid)) { na = LX_INF_A; nid = LX_INF_ID; }
        if (__any(na != LX_INF_A)) {
            wave_sort(na, nid, lane);
            wave_merge(best_a, best_id, na, nid, lane);
        }
    }
    const bool keep = lane < p.m && best_a != LX_INF_A;
    const uint64_t kept = __ballot(keep);
    if (keep) {
        p.part_a[(size_t)wi * p.m + lane] = best_a;
        p.part_id[(size_t)wi * p.m + lane] = best_id;
    }
    if (lane == 0) p.part_n[wi] = (uint32_t)__popcll((unsigned long long)kept);
}

__global__ __launch_bounds__(LX_TPB) void k_lexicon_merge(SuggestParams p) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint64_t e0 = (uint64_t)p.cbase[q] * p.m, e1 = (uint64_t)p.cbase[q + 1] * p.m;
    uint64_t best_a = LX_INF_A;
    uint32_t best_id = LX_INF_ID;
    for (uint64_t e = e0; e < e1; e += 64) {
        const uint64_t x = e + lane;
        uint64_t na = LX_INF_A;
        uint32_t nid = LX_INF_ID;
        if (x < e1) {
            const uint64_t ch = x / p.m;
            if ((uint32_t)(x - ch * p.m) < p.part_n[ch]) { na = p.part_a[x]; nid = p.part_id[x]; }
        }
        if (__any(na != LX_INF_A)) {
            wave_sort(na, nid, lane);
            wave_merge(best_a, best_id, na, nid, lane);
        }
    }
    const bool keep = lane < p.m && best_a != LX_INF_A;
    const uint64_t kept = __ballot(keep);
    if (keep) {
        p.terms_out[(size_t)q * p.m + lane] = best_id;
        if (p.dist_out) p.dist_out[(size_t)q * p.m + lane] = (int32_t)(best_a >> 32);
    }
    if (lane == 0) p.n_out[q] = (int32_t)__popcll((unsigned long long)kept);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------

int32_t upload_freq(ss_lexicon* lx, const uint32_t* freq) {
    ss_ctx* ctx = lx->ctx;
    hipStream_t st = ctx->stream;
    if (!lx->n_terms) return SS_OK;
    if (!freq) {
        if (lx->n_grouped) SS_HIP(ctx, hipMemsetAsync(lx->d_gfreq.p, 0, (size_t)lx->n_grouped * sizeof(uint32_t), st));
        SS_HIP(ctx, hipMemsetAsync(lx->d_ofreq.p, 0, (size_t)lx->n_terms * sizeof(uint32_t), st));
        return SS_OK;
    }
    ss::DevBuf<uint32_t> tmp;
    SS_HIP(ctx, tmp.alloc((size_t)lx->n_terms));
    SS_HIP(ctx, hipMemcpyAsync(tmp.p, freq, (size_t)lx->n_terms * sizeof(uint32_t), hipMemcpyDefault, st));
    if (lx->n_grouped) {
        hipLaunchKernelGGL(k_lexicon_gather_freq, dim3(ss::div_up(lx->n_grouped, 256)), dim3(256), 0, st, lx->d_gterm.p, tmp.p, lx->d_gfreq.p,
                           lx->n_grouped);
        SS_HIP(ctx, hipGetLastError());
    }
    // ... and in sort order, for the completions: the same gather with the sort order as its index
    hipLaunchKernelGGL(k_lexicon_gather_freq, dim3(ss::div_up((uint32_t)lx->n_terms, 256)), dim3(256), 0, st, lx->d_order.p, tmp.p,
                       lx->d_ofreq.p, (uint32_t)lx->n_terms);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, hipStreamSynchronize(st));                // the caller's array has been read, and tmp goes
    return SS_OK;
}

int32_t create_impl(ss_ctx* ctx, uint64_t n_terms, const uint64_t* word_ptr, const uint8_t* bytes, const uint32_t* freq, ss_lexicon** out) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out || !word_ptr) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_create: NULL argument");
    if (n_terms >= (1ull << 32)) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_create: %llu terms, must be below 2^32", (unsigned long long)n_terms);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> h_ptr((size_t)n_terms + 1);
    SS_HIP(ctx, ss::copy_in(st, h_ptr.data(), word_ptr, h_ptr.size() * sizeof(uint64_t)));
    if (!ss::lex::word_ptr_ok(h_ptr.data(), n_terms)) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_create: word_ptr must start at 0 and never decrease");
    const uint64_t n_bytes = h_ptr[(size_t)n_terms];
    if (n_bytes >= (1ull << 32)) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_create: %llu bytes, must be below 2^32", (unsigned long long)n_bytes);
    if (n_bytes && !bytes) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_create: bytes is NULL");
    std::vector<uint8_t> h_bytes((size_t)n_bytes);
    SS_HIP(ctx, ss::copy_in(st, h_bytes.data(), bytes, (size_t)n_bytes));
    std::vector<uint32_t> order, h_off((size_t)n_terms + 1);
    ss::lex::build_order(n_terms, h_ptr.data(), h_bytes.data(), order);
    ss::lex::Groups grp;
    ss::lex::build_groups(n_terms, h_ptr.data(), h_bytes.data(), grp);
    for (size_t t = 0; t <= (size_t)n_terms; t++) h_off[t] = (uint32_t)h_ptr[t];
    ss_lexicon* lx = new ss_lexicon();
    lx->ctx = ctx;
    lx->n_terms = n_terms;
    lx->n_bytes = n_bytes;
    lx->n_grouped = grp.start[ss::lex::N_GROUPS];
    std::memcpy(lx->start, grp.start, sizeof(lx->start));
    auto up = [&](auto& buf, const auto& vec) -> hipError_t {
        hipError_t e = buf.alloc(vec.size());
        if (e == hipSuccess && !vec.empty()) e = hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st);
        return e;
    };
    hipError_t e = up(lx->d_off, h_off);
    if (e == hipSuccess) e = up(lx->d_bytes, h_bytes);
    if (e == hipSuccess) e = up(lx->d_order, order);
    if (e == hipSuccess) e = up(lx->d_gterm, grp.gterm);
    if (e == hipSuccess) e = up(lx->d_gwords, grp.gwords);
    if (e == hipSuccess) e = lx->d_gfreq.alloc(grp.gterm.size());
    if (e == hipSuccess) e = lx->d_ofreq.alloc(order.size());
    if (e == hipSuccess) e = lx->d_start.alloc(N_STARTS);
    if (e == hipSuccess) e = lx->d_base.alloc(N_STARTS);
    if (e == hipSuccess) e = hipMemcpyAsync(lx->d_start.p, grp.start, sizeof(grp.start), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(lx->d_base.p, grp.base, sizeof(grp.base), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);    // the host vectors go when this function returns
    int32_t rc = SS_OK;
    if (e != hipSuccess) rc = ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "ss_lexicon_create: %s", hipGetErrorString(e));
    if (rc == SS_OK) rc = upload_freq(lx, freq);
    if (rc == SS_OK && !freq && lx->n_terms) {
        if (hipStreamSynchronize(st) != hipSuccess) rc = ctx->fail(SS_ERR_HIP, "ss_lexicon_create: wait failed");
    }
    if (rc != SS_OK) {
        (void)hipGetLastError();
        delete lx;
        return rc;
    }
    *out = lx;
    return SS_OK;
}

// what both calls do with their pointer array and bytes: ptr [n_q + 1] to the host, checked; the bytes it spans to `bytes_out`
int32_t fetch_words(ss_ctx* ctx, const char* entry, const char* name, int32_t n_q, const uint32_t* ptr, const uint8_t* bytes,
                    std::vector<uint32_t>& h_ptr, std::vector<uint8_t>& h_bytes) {
    h_ptr.resize((size_t)n_q + 1);
    SS_HIP(ctx, ss::copy_in(ctx->stream, h_ptr.data(), ptr, h_ptr.size() * sizeof(uint32_t)));
    if (!ss::lex::call_ptr_ok(h_ptr.data(), (uint64_t)n_q)) return ctx->fail(SS_ERR_INVALID, "%s: %s_ptr not non-decreasing", entry, name);
    const size_t nb = (size_t)h_ptr[(size_t)n_q] - h_ptr[0];
    if (nb && !bytes) return ctx->fail(SS_ERR_INVALID, "%s: %s_bytes is NULL", entry, name);
    h_bytes.resize(nb);
    SS_HIP(ctx, ss::copy_in(ctx->stream, h_bytes.data(), nb ? bytes + h_ptr[0] : nullptr, nb));
    return SS_OK;
}

int32_t prefix_impl(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr, const uint8_t* p_bytes, int64_t first, int32_t k,
                    uint32_t* terms_out, int32_t* n_out, uint64_t* n_match_out) {
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0 || !p_ptr || !terms_out || !n_out) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_prefix: NULL argument or n_q < 0");
    if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_prefix: k = %d, must be >= 1", k);
    if (first < 0) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_prefix: first = %lld, must be >= 0", (long long)first);
    if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_prefix: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr;
    std::vector<uint8_t> h_bytes;
    SS_TRY(fetch_words(ctx, "ss_lexicon_prefix", "p", n_q, p_ptr, p_bytes, h_ptr, h_bytes));
    const bool dev_t = ss::on_device(terms_out), dev_n = ss::on_device(n_out), dev_m = !n_match_out || ss::on_device(n_match_out);
    // ---- the call's table in the pinned block of the next turn: {offset, length} [n_q] | prefix bytes
    LexTurn& turn = lx->turn[lx->next_turn];
    SS_HIP(ctx, turn.ev.wait());                          // the call LX_TURNS calls ago has read this turn's blocks
    const size_t q_words = 2 * nq + (h_bytes.size() + 3) / 4;
    SS_HIP(ctx, turn.h_q.ensure(q_words * sizeof(uint32_t)));
    uint32_t* const hq = turn.h_q.as<uint32_t>();
    for (size_t q = 0; q < nq; q++) {
        hq[2 * q] = h_ptr[q] - h_ptr[0];
        hq[2 * q + 1] = h_ptr[q + 1] - h_ptr[q];
    }
    if (!h_bytes.empty()) std::memcpy(hq + 2 * nq, h_bytes.data(), h_bytes.size());
    SS_HIP(ctx, ensure(turn.d_q, q_words));
    if (!dev_t) SS_HIP(ctx, ensure(lx->d_out_terms, nq * (size_t)k));
    if (!dev_n) SS_HIP(ctx, ensure(lx->d_out_n, nq));
    if (!dev_m) SS_HIP(ctx, ensure(lx->d_out_match, nq));
    lx->next_turn = (lx->next_turn + 1) % LX_TURNS;
    // ---- the pipeline
    SS_HIP(ctx, hipMemcpyAsync(turn.d_q.p, hq, q_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    PrefixParams p{};
    p.off = lx->d_off.p; p.bytes = lx->d_bytes.p; p.order = lx->d_order.p;
    p.q = turn.d_q.p;
    p.n_terms = (uint32_t)lx->n_terms; p.n_q = (uint32_t)n_q; p.k = (uint32_t)k;
    p.first = first;
    p.terms_out = dev_t ? terms_out : lx->d_out_terms.p;
    p.n_out = dev_n ? n_out : lx->d_out_n.p;
    p.n_match_out = !n_match_out ? nullptr : dev_m ? n_match_out : lx->d_out_match.p;
    hipLaunchKernelGGL(k_lexicon_prefix, dim3((unsigned)n_q), dim3(LX_TPB), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    if (dev_t && dev_n && dev_m) return SS_OK;            // ordered on the ctx stream; nothing comes back, nothing is waited for
    // ---- staged: wait; a host terms_out gets exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq);
    std::vector<uint32_t> h_t(dev_t ? 0 : nq * (size_t)k);
    std::vector<uint64_t> h_m(dev_m ? 0 : nq);
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), p.n_out, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_t) SS_HIP(ctx, hipMemcpyAsync(h_t.data(), p.terms_out, h_t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!dev_m) SS_HIP(ctx, hipMemcpyAsync(h_m.data(), p.n_match_out, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_out, h_n.data(), nq * sizeof(int32_t));
    if (!dev_m) std::memcpy(n_match_out, h_m.data(), nq * sizeof(uint64_t));
    if (!dev_t)
        for (size_t q = 0; q < nq; q++) {
            const size_t n = (size_t)std::min(std::max(h_n[q], 0), k);
            if (n) std::memcpy(terms_out + q * (size_t)k, h_t.data() + q * (size_t)k, n * sizeof(uint32_t));
        }
    return SS_OK;
}

int32_t complete_impl(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr, const uint8_t* p_bytes, uint32_t min_freq, int32_t m,
                      uint32_t* terms_out, uint32_t* freq_out, int32_t* n_out, uint64_t* n_match_out) {
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0 || !p_ptr || !terms_out || !n_out) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_complete: NULL argument or n_q < 0");
    if (m < 1) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_complete: m = %d, must be >= 1", m);
    if (m > SS_MAX_COMPLETE) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_complete: m = %d exceeds SS_MAX_COMPLETE = %d", m, SS_MAX_COMPLETE);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr;
    std::vector<uint8_t> h_bytes;
    SS_TRY(fetch_words(ctx, "ss_lexicon_complete", "p", n_q, p_ptr, p_bytes, h_ptr, h_bytes));
    // parts per prefix from n_q alone: the scratch is n_q * P * m keys (at most about COMPLETE_WAVES * m unless P is forced)
    const uint32_t P = ss::lex::complete_parts((uint64_t)n_q, ctx->opt("lexicon.complete_parts", 0));
    if (nq * P >= (1ull << 31))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_complete: the batch makes 2^31 (prefix, part) pairs or more: lower \"lexicon.complete_parts\" or split it");
    const bool dev_t = ss::on_device(terms_out), dev_n = ss::on_device(n_out), dev_f = !freq_out || ss::on_device(freq_out),
               dev_m = !n_match_out || ss::on_device(n_match_out);
    // ---- the call's table in the pinned block of the next turn, as ss_lexicon_prefix lays it out: {offset, length} [n_q] | prefix bytes
    LexTurn& turn = lx->turn[lx->next_turn];
    SS_HIP(ctx, turn.ev.wait());                          // the call LX_TURNS calls ago has read this turn's blocks
    const size_t q_words = 2 * nq + (h_bytes.size() + 3) / 4;
    SS_HIP(ctx, turn.h_q.ensure(q_words * sizeof(uint32_t)));
    uint32_t* const hq = turn.h_q.as<uint32_t>();
    for (size_t q = 0; q < nq; q++) {
        hq[2 * q] = h_ptr[q] - h_ptr[0];
        hq[2 * q + 1] = h_ptr[q + 1] - h_ptr[q];
    }
    if (!h_bytes.empty()) std::memcpy(hq + 2 * nq, h_bytes.data(), h_bytes.size());
    SS_HIP(ctx, ensure(turn.d_q, q_words));
    SS_HIP(ctx, ensure(lx->d_cpl_key, nq * P * (size_t)m));
    SS_HIP(ctx, ensure(lx->d_cpl_bounds, 2 * nq));
    if (!dev_t) SS_HIP(ctx, ensure(lx->d_out_terms, nq * (size_t)m));
    if (!dev_f) SS_HIP(ctx, ensure(lx->d_out_freq, nq * (size_t)m));
    if (!dev_n) SS_HIP(ctx, ensure(lx->d_out_n, nq));
    if (!dev_m) SS_HIP(ctx, ensure(lx->d_out_match, nq));
    lx->next_turn = (lx->next_turn + 1) % LX_TURNS;
    // ---- the pipeline
    SS_HIP(ctx, hipMemcpyAsync(turn.d_q.p, hq, q_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CompleteParams p{};
    p.lex.off = lx->d_off.p; p.lex.bytes = lx->d_bytes.p; p.lex.order = lx->d_order.p;
    p.lex.q = turn.d_q.p;
    p.lex.n_terms = (uint32_t)lx->n_terms; p.lex.n_q = (uint32_t)n_q; p.lex.k = (uint32_t)m;
    p.lex.terms_out = dev_t ? terms_out : lx->d_out_terms.p;
    p.lex.n_out = dev_n ? n_out : lx->d_out_n.p;
    p.lex.n_match_out = !n_match_out ? nullptr : dev_m ? n_match_out : lx->d_out_match.p;
    p.ofreq = lx->d_ofreq.p;
    p.bounds = lx->d_cpl_bounds.p;
    p.part_key = lx->d_cpl_key.p;
    p.freq_out = !freq_out ? nullptr : dev_f ? freq_out : lx->d_out_freq.p;
    p.P = P; p.min_freq = min_freq;
    const dim3 waves((unsigned)(nq * P)), rows((unsigned)n_q), block(LX_TPB);
    hipLaunchKernelGGL(k_lexicon_complete_bounds, rows, block, 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lexicon_complete, waves, block, 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lexicon_complete_merge, rows, block, 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    if (dev_t && dev_n && dev_f && dev_m) return SS_OK;   // ordered on the ctx stream; nothing comes back, nothing is waited for
    // ---- staged: wait; host rows get exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq);
    std::vector<uint32_t> h_t(dev_t ? 0 : nq * (size_t)m), h_f(dev_f ? 0 : nq * (size_t)m);
    std::vector<uint64_t> h_m(dev_m ? 0 : nq);
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), p.lex.n_out, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_t) SS_HIP(ctx, hipMemcpyAsync(h_t.data(), p.lex.terms_out, h_t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!dev_f) SS_HIP(ctx, hipMemcpyAsync(h_f.data(), p.freq_out, h_f.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!dev_m) SS_HIP(ctx, hipMemcpyAsync(h_m.data(), p.lex.n_match_out, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_out, h_n.data(), nq * sizeof(int32_t));
    if (!dev_m) std::memcpy(n_match_out, h_m.data(), nq * sizeof(uint64_t));
    for (size_t q = 0; q < nq; q++) {
        const size_t n = (size_t)std::min(std::max(h_n[q], 0), m);
        if (!n) continue;
        if (!dev_t) std::memcpy(terms_out + q * (size_t)m, h_t.data() + q * (size_t)m, n * sizeof(uint32_t));
        if (!dev_f) std::memcpy(freq_out + q * (size_t)m, h_f.data() + q * (size_t)m, n * sizeof(uint32_t));
    }
    return SS_OK;
}

int32_t suggest_impl(ss_lexicon* lx, int32_t n_q, const uint32_t* w_ptr, const uint8_t* w_bytes, int32_t max_dist, uint32_t min_freq,
                     int32_t m, uint32_t* terms_out, int32_t* dist_out, int32_t* n_out) {
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    if (n_q < 0 || !w_ptr || !terms_out || !n_out) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_suggest: NULL argument or n_q < 0");
    if (m < 1) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_suggest: m = %d, must be >= 1", m);
    if (max_dist < 0) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_suggest: max_dist = %d, must be >= 0", max_dist);
    if (m > SS_MAX_SUGGEST) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_suggest: m = %d exceeds SS_MAX_SUGGEST = %d", m, SS_MAX_SUGGEST);
    if (max_dist > SS_MAX_EDIT_DIST)
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_suggest: max_dist = %d exceeds SS_MAX_EDIT_DIST = %d", max_dist, SS_MAX_EDIT_DIST);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nq = (size_t)n_q;
    std::vector<uint32_t> h_ptr;
    std::vector<uint8_t> h_bytes;
    SS_TRY(fetch_words(ctx, "ss_lexicon_suggest", "w", n_q, w_ptr, w_bytes, h_ptr, h_bytes));
    const uint32_t chunk = (uint32_t)std::min(std::max(ctx->opt("lexicon.chunk_terms", LX_CHUNK_DEFAULT), (int64_t)1), LX_CHUNK_MAX);
    // the chunk plan: query q takes chunks cbase[q] .. cbase[q + 1] of its grouped range [lo, hi)
    std::vector<uint32_t> plan(4 * nq + nq + 1);
    uint32_t* const cbase = plan.data() + 4 * nq;
    uint64_t total = 0;
    for (size_t q = 0; q < nq; q++) {
        uint32_t lo, hi;
        ss::lex::suggest_range(lx->start, (uint64_t)h_ptr[q + 1] - h_ptr[q], (uint32_t)max_dist, &lo, &hi);
        plan[4 * q] = h_ptr[q] - h_ptr[0];
        plan[4 * q + 1] = h_ptr[q + 1] - h_ptr[q];
        plan[4 * q + 2] = lo;
        plan[4 * q + 3] = hi;
        cbase[q] = (uint32_t)total;
        total += ss::lex::n_chunks(lo, hi, chunk);
        if (total >= (1ull << 31))
            return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_suggest: the batch makes 2^31 (query word, chunk) pairs or more: raise \"lexicon.chunk_terms\" or split it");
    }
    cbase[nq] = (uint32_t)total;
    if ((uint64_t)lx->n_grouped > 0xFFFFFFFFull - 64) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_lexicon_suggest: too many words");
    const bool dev_t = ss::on_device(terms_out), dev_n = ss::on_device(n_out), dev_d = !dist_out || ss::on_device(dist_out);
    // ---- the call's table in the pinned block of the next turn: {offset, length, lo, hi} [n_q] | cbase [n_q + 1] | query bytes
    LexTurn& turn = lx->turn[lx->next_turn];
    SS_HIP(ctx, turn.ev.wait());                          // the call LX_TURNS calls ago has read this turn's blocks
    const size_t q_words = plan.size() + (h_bytes.size() + 3) / 4;
    SS_HIP(ctx, turn.h_q.ensure(q_words * sizeof(uint32_t)));
    uint32_t* const hq = turn.h_q.as<uint32_t>();
    std::memcpy(hq, plan.data(), plan.size() * sizeof(uint32_t));
    if (!h_bytes.empty()) std::memcpy(hq + plan.size(), h_bytes.data(), h_bytes.size());
    SS_HIP(ctx, ensure(turn.d_q, q_words));
    SS_HIP(ctx, ensure(lx->d_part_a, (size_t)total * (size_t)m));
    SS_HIP(ctx, ensure(lx->d_part_id, (size_t)total * (size_t)m));
    SS_HIP(ctx, ensure(lx->d_part_n, (size_t)total));
    if (!dev_t) SS_HIP(ctx, ensure(lx->d_out_terms, nq * (size_t)m));
    if (!dev_d) SS_HIP(ctx, ensure(lx->d_out_dist, nq * (size_t)m));
    if (!dev_n) SS_HIP(ctx, ensure(lx->d_out_n, nq));
    lx->next_turn = (lx->next_turn + 1) % LX_TURNS;
    // ---- the pipeline
    SS_HIP(ctx, hipMemcpyAsync(turn.d_q.p, hq, q_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SuggestParams p{};
    p.gterm = lx->d_gterm.p; p.gfreq = lx->d_gfreq.p; p.gwords = lx->d_gwords.p; p.start = lx->d_start.p; p.base = lx->d_base.p;
    p.qinfo = turn.d_q.p;
    p.cbase = turn.d_q.p + 4 * nq;
    p.qbytes = reinterpret_cast<const uint8_t*>(turn.d_q.p + plan.size());
    p.part_a = lx->d_part_a.p; p.part_id = lx->d_part_id.p; p.part_n = lx->d_part_n.p;
    p.n_q = (uint32_t)n_q; p.chunk = chunk; p.m = (uint32_t)m; p.min_freq = min_freq;
    p.terms_out = dev_t ? terms_out : lx->d_out_terms.p;
    p.dist_out = !dist_out ? nullptr : dev_d ? dist_out : lx->d_out_dist.p;
    p.n_out = dev_n ? n_out : lx->d_out_n.p;
    if (total) {
        const dim3 grid((unsigned)total), block(LX_TPB);
        switch (max_dist) {
            case 0: hipLaunchKernelGGL(k_lexicon_suggest<0>, grid, block, 0, st, p); break;
            case 1: hipLaunchKernelGGL(k_lexicon_suggest<1>, grid, block, 0, st, p); break;
            case 2: hipLaunchKernelGGL(k_lexicon_suggest<2>, grid, block, 0, st, p); break;
            default: hipLaunchKernelGGL(k_lexicon_suggest<3>, grid, block, 0, st, p); break;
        }
        SS_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_lexicon_merge, dim3((unsigned)n_q), dim3(LX_TPB), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.ev.record(st));                      // the turn's pinned block and its device copy are read until here
    if (dev_t && dev_n && dev_d) return SS_OK;            // ordered on the ctx stream; nothing comes back, nothing is waited for
    // ---- staged: wait; host rows get exactly the entries the kernel wrote
    std::vector<int32_t> h_n(nq);
    std::vector<uint32_t> h_t(dev_t ? 0 : nq * (size_t)m);
    std::vector<int32_t> h_d(dev_d ? 0 : nq * (size_t)m);
    SS_HIP(ctx, hipMemcpyAsync(h_n.data(), p.n_out, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!dev_t) SS_HIP(ctx, hipMemcpyAsync(h_t.data(), p.terms_out, h_t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!dev_d) SS_HIP(ctx, hipMemcpyAsync(h_d.data(), p.dist_out, h_d.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (!dev_n) std::memcpy(n_out, h_n.data(), nq * sizeof(int32_t));
    for (size_t q = 0; q < nq; q++) {
        const size_t n = (size_t)std::min(std::max(h_n[q], 0), m);
        if (!n) continue;
        if (!dev_t) std::memcpy(terms_out + q * (size_t)m, h_t.data() + q * (size_t)m, n * sizeof(uint32_t));
        if (!dev_d) std::memcpy(dist_out + q * (size_t)m, h_d.data() + q * (size_t)m, n * sizeof(int32_t));
    }
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_lexicon_create(ss_ctx* ctx, uint64_t n_terms, const uint64_t* word_ptr, const uint8_t* bytes, const uint32_t* freq, ss_lexicon** out) {
    if (!ctx) return SS_ERR_INVALID;
    try {
        return create_impl(ctx, n_terms, word_ptr, bytes, freq, out);
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "ss_lexicon_create: host allocation failed");
    }
}

int32_t ss_lexicon_set_freq(ss_lexicon* lx, const uint32_t* freq) {
    if (!lx) return SS_ERR_INVALID;
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    // (on the context's stream: behind every suggest call enqueued so far, in front of every later one)
    return upload_freq(lx, freq);
}

int32_t ss_lexicon_get_info(const ss_lexicon* lx, uint64_t* n_terms, uint64_t* n_bytes) {
    if (!lx) return SS_ERR_INVALID;
    if (n_terms) *n_terms = lx->n_terms;
    if (n_bytes) *n_bytes = lx->n_bytes;
    return SS_OK;
}

int32_t ss_lexicon_read_order(ss_lexicon* lx, uint32_t* order_out) {
    if (!lx) return SS_ERR_INVALID;
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!order_out) return ctx->fail(SS_ERR_INVALID, "ss_lexicon_read_order: order_out is NULL");
    if (!lx->n_terms) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    SS_HIP(ctx, hipMemcpyAsync(order_out, lx->d_order.p, (size_t)lx->n_terms * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SS_OK;
}

int32_t ss_lexicon_destroy(ss_lexicon* lx) {
    if (!lx) return SS_ERR_INVALID;
    ss_ctx* ctx = lx->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete lx;
    return SS_OK;
}

int32_t ss_lexicon_prefix(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr, const uint8_t* p_bytes, int64_t first, int32_t k,
                          uint32_t* terms_out, int32_t* n_out, uint64_t* n_match_out) {
    if (!lx) return SS_ERR_INVALID;
    try {
        return prefix_impl(lx, n_q, p_ptr, p_bytes, first, k, terms_out, n_out, n_match_out);
    } catch (const std::bad_alloc&) {
        return lx->ctx->fail(SS_ERR_OOM, "ss_lexicon_prefix: host allocation failed");
    }
}

int32_t ss_lexicon_complete(ss_lexicon* lx, int32_t n_q, const uint32_t* p_ptr, const uint8_t* p_bytes, uint32_t min_freq, int32_t m,
                            uint32_t* terms_out, uint32_t* freq_out, int32_t* n_out, uint64_t* n_match_out) {
    if (!lx) return SS_ERR_INVALID;
    try {
        return complete_impl(lx, n_q, p_ptr, p_bytes, min_freq, m, terms_out, freq_out, n_out, n_match_out);
    } catch (const std::bad_alloc&) {
        return lx->ctx->fail(SS_ERR_OOM, "ss_lexicon_complete: host allocation failed");
    }
}

int32_t ss_lexicon_suggest(ss_lexicon* lx, int32_t n_q, const uint32_t* w_ptr, const uint8_t* w_bytes, int32_t max_dist, uint32_t min_freq,
                           int32_t m, uint32_t* terms_out, int32_t* dist_out, int32_t* n_out) {
    if (!lx) return SS_ERR_INVALID;
    try {
        return suggest_impl(lx, n_q, w_ptr, w_bytes, max_dist, min_freq, m, terms_out, dist_out, n_out);
    } catch (const std::bad_alloc&) {
        return lx->ctx->fail(SS_ERR_OOM, "ss_lexicon_suggest: host allocation failed");
    }
}

}  // extern "C"
