// score.hip — batched OR-query cosine scorer + PageRank blend + top-k for gfx950 (MI355X).
//
// Replaces, per query (retrieval/main_retrieve.go:50-103):
//   getFromInverted  :204-247   fetch body+title postings of every query token
//   aggregation      :61-69     OR-union by doc, weights appended per token (duplicates count twice)
//   genAggrDocs      :170-187   TitleRank = sum float64(w_title), BodyRank = sum float64(w_body)
//   computeFinalRank get_metadata.go:31-69
//                               Body  /= mag_body  * sqrt(queryLength)   (:53,:57)
//                               Title /= mag_title * sqrt(queryLength)   (:58)
//                               NaN -> 0                                 (:61-66)
//                               sqd   = sum_t topicProbs[t]*PR[doc][t]   (:39-42)
//                               Final = (0.33*sqd+0.38*Title+0.29*Body)*100 (:69)
//   appendSort + cut util.go:48-54, main_retrieve.go:99-103  descending FinalRank, first k
//
// Device design (HBM-bound streaming of 8-byte posting records — exactly SURVEY.md §8d's 8 bytes per posting):
//   * scoring layout: one 8-byte record per posting {doc u32, impact f32}, impact = float32 UPPER bound of
//     w / magnitude(doc, field).  The float32 weights and float64 magnitudes stay in the index's own arrays and
//     are only read for documents that can still enter the top-k.
//   * the host plans (score_call.hip; it keeps df per term): duplicates -> multiplicities, unknown terms dropped, each query's
//     doc range cut into slices, longest first; one 512-thread workgroup per (query, slice).
//   * k_score_slices builds the slice's window plan in LDS (window = a doc range holding <= CAP records; every
//     record of a doc lies in one window), then streams the windows, window j+1's records in flight while window
//     j is processed.  Per window TWO stages:
//       1. FILTER (every record; one LDS integer atomic, one LDS read, one barrier per window, no probing, no keys):
//          c = impact * coef(list), in fixed point and rounded up, is added into slot hash(doc) of a small table
//          ("sketch": collisions only make the sum larger); after the barrier every record reads its slot back: the
//          value is an upper bound of its document's FinalRank.  If it is below the running threshold the record is
//          dropped.  Three tables rotate so that clearing the slots a window touched needs no second barrier.
//       2. EXACT (survivors only, batched): surviving records are appended to a pending list {doc, index in
//          list, list}; when the list fills (or the slice ends) all threads gather the survivors' float32
//          weights and float64 magnitudes from the index (one round of HBM latency for the whole batch), aggregate
//          them per document in an LDS hash table (float32 addends in float64: exact, order-free), compute the
//          reference's float64 arithmetic literally, and feed the running top-k (exact keys, bitonic compaction).
//     The running threshold starts at a bound known before any posting is read: the index keeps, per term and
//     field, the k'-th largest impact for k' = 1,2,4..1024, and k' >= k postings of ONE list are k' distinct
//     documents whose FinalRank is at least their own contribution.
//     Inputs outside the filter's assumptions (negative or non-finite weights, priors or probabilities, zero
//     magnitudes under non-zero weights, queryLength <= 0) switch the filter off for the call: every record
//     survives and stage 2 alone decides — same results, no separate code path.
//   * k_merge_topk: one workgroup per query merges its slices' top-k lists, re-derives
//     title/body/pagerank of the k winners by binary search and writes ss_hit rows.
//   Ties: ascending doc id (Q10); NaN finals last.
#include "scorer.hpp"

namespace {

// ---- K4: score one (query, doc-range slice) --------------------------------------
struct ScoreLds {                     // byte offsets into the dynamic LDS block
    size_t s_rec, l_rec, l_w, sc64, cd_key, cd_doc, ht_key, ht_rec, sk, tbl, l_mult, l_field, f_cur, f_nxt, l_coef, sc32, sel, sel64, off, total;
};
__host__ __device__ inline ScoreLds score_lds_layout(int cb) {
    ScoreLds o{};
    size_t p = 0;
    o.s_rec = p;   p += (size_t)PC * 16;            // pending survivors {doc, index, list, -}; rewritten in place as {addend f64, magnitude f64}
    o.l_rec = p;   p += (size_t)MAXL * 8;
    o.l_w = p;     p += (size_t)MAXL * 8;
    o.sc64 = p;    p += 4 * 8;
    o.cd_key = p;  p += (size_t)cb * 8;
    o.cd_doc = p;  p += (size_t)cb * 4;
    o.ht_key = p;  p += (size_t)HT * 4;
    o.ht_rec = p;  p += (size_t)HT * 4;
    o.sk = p;      p += (size_t)3 * SK * 4;
    o.tbl = p;     p += (size_t)TBL_CAP * 4;
    o.l_mult = p;  p += (size_t)MAXL * 4;
    o.l_field = p; p += (size_t)MAXL * 4;
    o.f_cur = p;   p += (size_t)MAXL * 4;
    o.f_nxt = p;   p += (size_t)MAXL * 4;
    o.l_coef = p;  p += (size_t)MAXL * 4;
    o.sc32 = p;    p += 16 * 4;
    o.sel = p;     p += (256 + 8) * 4;              // topk_select_inl: histogram + scalars
    o.sel64 = p;   p += 4 * 8;
    o.off = p;     p += (size_t)OFF_CAP * 2;
    o.total = (p + 15) & ~(size_t)15;
    return o;
}

// The workgroup's LDS arrays as typed pointers (passed by reference into force-inlined helpers: after inlining they
// are plain SSA values derived from the LDS block, so every access stays a ds_* instruction).
struct SliceLds {
    double2* s_rec;      // [PC] exact stage: {addend (summed: BodyRank/TitleRank of the doc), magnitude}
    uint4* pend;         // [PC] the same bytes while pending: {doc, index in list, list, -}
    uint64_t* l_rec;     // [MAXL] address of the list's first record
    uint64_t* l_w;       // [MAXL] address of the list's first float32 weight
    uint32_t* ht_key;    // [HT]
    uint32_t* ht_rec;    // [HT] first body record (low 16 bits) and first title record (high 16) of the slot's doc
    uint32_t* sk;        // [3][SK] filter tables (fixed point)
    uint32_t* tbl;       // [TBL_CAP] cursor of list l at the start of window j: tbl[j*L+l]
    uint32_t* l_mult;    // [MAXL] multiplicity of the term in the query
    uint32_t* l_field;   // [MAXL] 0 = body, 1 = title
    uint32_t* f_cur;     // [MAXL] oversize fallback: sub-window start
    uint32_t* f_nxt;     // [MAXL] oversize fallback: sub-window end
    float* l_coef;       // [MAXL] filter coefficient in fixed-point units: upper bound of (38|29)*mult/sqrt(queryLength) * scale
    uint16_t* off;       // [OFF_CAP] offset of list l inside window j: off[j*OS+l], count at [j*OS+OS-1]
    uint32_t* overflow;  // shared scalar
    uint32_t* sel;       // [256 + 8] scratch of topk_select_inl
    uint64_t* sel64;     // [4]
};

// generic window loop (L > LCH lists): records of one window as raw 8-byte vectors (one global_load_dwordx2 per posting)
// with their list, index in the list and filter coefficient; the list of record i by binary search in the window's offsets
__device__ __forceinline__ void load_window(const SliceLds& S, int j, int L, int OS, int tid,
                                            u32x2 (&rec)[PPT], uint32_t (&rl)[PPT], uint32_t (&ri)[PPT], float (&rc)[PPT]) {
    const uint32_t* tbl_j = S.tbl + j * L;
    const uint16_t* off_j = S.off + j * OS;
    const uint32_t n = off_j[OS - 1];
#pragma unroll
    for (int r = 0; r < PPT; r++) {
        const uint32_t i = tid + r * TPB;
        rl[r] = EMPTY;
        if (i < n) {
            int lo = 0, hi = L;            // largest l with off[l] <= i
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off_j[mid] <= i) lo = mid; else hi = mid;
            }
            ri[r] = tbl_j[lo] + (i - off_j[lo]);
            rec[r] = load_rec(S.l_rec[lo], ri[r]);
            rl[r] = lo;
            rc[r] = S.l_coef[lo];
        }
    }
}

// ---- exact stage -----------------------------------------------------------------------------------------------
// score ONE doc of the exact stage's table (get_metadata.go:31-69) — the thread that claimed the doc's slot owns it —
// reset its slot and offer it to the running top-k.  All threads call (slot = EMPTY: nothing to score): the admit
// loop's barrier is workgroup-wide.
__device__ __forceinline__ void score_owned(const SliceLds& S, const TopK& tk, const SliceQuery& Q, const ScoreParams& p, int tid,
                                            uint32_t doc, uint32_t slot) {
    uint32_t e_doc = EMPTY;
    uint64_t e_key = 0;
    if (slot != EMPTY) {
        e_doc = doc;
        const bool allowed = doc_allowed(Q.mask, doc);
        const uint32_t fr = S.ht_rec[slot];
        // no posting of a field => its sum is 0 and 0/(m*q) is 0 (or NaN -> 0) for every m
        double2 rb = make_double2(0.0, 1.0), rt = make_double2(0.0, 1.0);
        const uint32_t ib = fr & 0xFFFFu, it = fr >> 16;
        if (ib != NOREC) rb = S.s_rec[ib];
        if (it != NOREC) rt = S.s_rec[it];
        S.ht_key[slot] = EMPTY;
        S.ht_rec[slot] = EMPTY;
        const double B = rb.x, T = rt.x, mb = rb.y, mt = rt.y;
        const uint64_t thr0 = *tk.thr;
        const float thr_f = *tk.thr_f;
        // cheap float estimate first; skipped only if the estimate, with a 1e-4 relative margin, is clearly below the
        // threshold; anything non-finite falls through to the exact path.
        // v_rcp_f32 (1 ulp) instead of an IEEE division: the 1e-4 margin below covers it; 0*inf = NaN falls through
        const float ea = 38.0f * ((float)T * __builtin_amdgcn_rcpf((float)mt * Q.qmag_f)), eb = 29.0f * ((float)B * __builtin_amdgcn_rcpf((float)mb * Q.qmag_f)),
                    ec = 33.0f * Q.sqd_ub_f;
        // a doc outside the query's allow-list never enters the running top-k: the threshold comes from allowed docs only
        if (!allowed || (ea + eb + ec) + (fabsf(ea) + fabsf(eb) + fabsf(ec)) * 1e-4f + 1e-30f < thr_f) {
            e_doc = EMPTY;
        } else {
            double title, body, fin;
            if (Q.probs) {
                // the prior row (128 B) is only fetched if the doc can still make the top-k:
                // every operation of final_rank is monotone in sqd, so sqd_ub bounds the score
                final_rank(T, B, mt, mb, Q.qmag, Q.sqd_ub, title, body, fin);
                if (fkey(fin) >= thr0 || fin != fin) final_rank(T, B, mt, mb, Q.qmag, topic_dot(p.prior, Q.probs, p.k_topics, e_doc), title, body, fin);
                else e_doc = EMPTY;
            } else {
                final_rank(T, B, mt, mb, Q.qmag, 0.0, title, body, fin);
            }
            e_key = fkey(fin);
        }
    }
    // threshold filter into the candidate buffer; overflow -> compact and retry
    for (;;) {
        const uint64_t thr = *tk.thr;
        if (e_doc != EMPTY) {
            if (e_key >= thr) {
                const uint32_t i = atomicAdd(tk.count, 1u);
                if (i < tk.cb) { tk.key[i] = e_key; tk.doc[i] = e_doc; e_doc = EMPTY; }
                else *S.overflow = 1;
            } else {
                e_doc = EMPTY;
            }
        }
        lds_barrier();
        if (!*S.overflow) break;
        topk_cut(tk, p.k, S.sel, S.sel64);   // raises thr; count back to <= k (unordered: radix selection where one entry per thread fits)
        if (tid == 0) *S.overflow = 0;
        lds_barrier();
    }
}

// The pending survivors pend[0, n) -> per-document sums -> FinalRank -> running top-k.  All threads call with the
// same n (<= PC).  On return the pending list is empty and the hash table clean.
__device__ __forceinline__ void flush_pending(const SliceLds& S, const TopK& tk, const SliceQuery& Q, const ScoreParams& p, int tid, uint32_t n) {
    DIAG_ADD(2, 1);
    DIAG_ADD(3, n);
    DIAG_NOW(t_f0);
    uint32_t pdoc[PPX], pl[PPX], own[PPX];
    float pw[PPX];
    double pm[PPX];
#pragma unroll
    for (int r = 0; r < PPX; r++) {
        const uint32_t i = tid + r * TPB;
        pl[r] = EMPTY;
        if (i < n) {
            const uint4 e = S.pend[i];
            pdoc[r] = e.x;
            pl[r] = e.z;
            // one round of memory latency for the whole batch: the survivor's float32 weight and its doc's float64 magnitude
            pw[r] = load_w(S.l_w[e.z], e.y);
            pm[r] = (S.l_field[e.z] ? p.t_mag : p.b_mag)[e.x];
        }
    }
    lds_barrier();                                  // every pending entry has been read: the bytes may be rewritten
    // accumulate per doc (main_retrieve.go:61-69,170-187); float32 addends in float64: exact, any order.
    // A table slot names, per field, the FIRST record of its doc (one 32-bit CAS on the packed word); the rare later
    // records of the same (doc, field) add their addend into the first one's.
#pragma unroll
    for (int r = 0; r < PPX; r++) {
        const uint32_t l = pl[r];
        own[r] = EMPTY;
        if (l != EMPTY) {
            const uint32_t i = tid + r * TPB;
            uint32_t h = (((pdoc[r] * 2654435761u) >> 20) * (uint32_t)(HT / 256)) >> 4;      // 12 hash bits -> [0, HT)
            for (;;) {
                const uint32_t prev = atomicCAS(&S.ht_key[h], EMPTY, pdoc[r]);
                if (prev == EMPTY) own[r] = h;     // this thread claimed the doc's slot: it will score the doc
                if (prev == EMPTY || prev == pdoc[r]) break;
                h = h + 1 == HT ? 0 : h + 1;
            }
            const uint32_t field = S.l_field[l];        // 0 = body (low half), 1 = title (high half)
            const double v = (double)pw[r] * (double)S.l_mult[l];
            S.s_rec[i] = make_double2(v, pm[r]);
            asm volatile("" ::: "memory");         // program order: parked before it can be named (LDS runs a wave's operations in order)
            uint32_t old = S.ht_rec[h], first;
            for (;;) {
                first = field ? old >> 16 : old & 0xFFFFu;
                if (first != NOREC) break;
                const uint32_t want = field ? (old & 0xFFFFu) | (i << 16) : (old & 0xFFFF0000u) | i;
                const uint32_t prev = atomicCAS(&S.ht_rec[h], old, want);
                if (prev == old) break;            // first stays NOREC: this record is the first of its (doc, field)
                old = prev;
            }
            if (first != NOREC) atomicAdd(&S.s_rec[first].x, v);
        }
    }
    lds_barrier();
#pragma unroll
    for (int r = 0; r < PPX; r++) score_owned(S, tk, Q, p, tid, pdoc[r], own[r]);
    DIAG_NOW(t_f1);
    DIAG_ADD(8, t_f1 - t_f0);
}

// ---- oversize window (a list is locally much denser than planned): bisect its doc range until a piece fits and hand
//      every record of the piece to the exact stage.  Rare; no filter.  The pending list must be empty on entry. ----
__device__ __forceinline__ void oversize_window(const SliceLds& S, const TopK& tk, const SliceQuery& Q, const ScoreParams& p, int tid, int L,
                                                int j, int n_win, const SliceDesc& sd, uint32_t drv, uint64_t drv_addr) {
    if (tid < L) S.f_cur[tid] = S.tbl[j * L + tid];
    uint32_t flo = j == 0 ? sd.dlo : load_doc(drv_addr, S.tbl[j * L + drv]);
    const uint32_t fend = j + 1 == n_win ? sd.dhi : load_doc(drv_addr, S.tbl[(j + 1) * L + drv]);
    __syncthreads();
    for (;;) {
        uint32_t fhi = fend;
        uint32_t cnt;
        for (;;) {
            if (tid < L) {
                S.f_nxt[tid] = fhi == fend ? S.tbl[(j + 1) * L + tid]
                                           : lower_bound_addr(S.l_rec[tid], S.f_cur[tid], S.tbl[(j + 1) * L + tid], fhi);
            }
            __syncthreads();
            cnt = 0;
            for (int l = 0; l < L; l++) cnt += S.f_nxt[l] - S.f_cur[l];
            if (cnt <= (uint32_t)CAP) break;
            // a single doc has at most L <= 132 postings, so the bisection ends
            fhi = flo + (uint32_t)(((uint64_t)fhi - flo) >> 1);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < PPT; r++) {
            const uint32_t i = tid + r * TPB;
            if (i < cnt) {
                uint32_t run = 0;
                int l = 0;
                for (; l < L; l++) {
                    const uint32_t len = S.f_nxt[l] - S.f_cur[l];
                    if (i < run + len) break;
                    run += len;
                }
                const uint32_t idx = S.f_cur[l] + (i - run);
                S.pend[i] = make_uint4(load_doc(S.l_rec[l], idx), idx, (uint32_t)l, 0u);
            }
        }
        lds_barrier();
        flush_pending(S, tk, Q, p, tid, cnt);
        bool done = true;
        for (int l = 0; l < L; l++) done = done && S.f_nxt[l] == S.tbl[(j + 1) * L + l];
        __syncthreads();
        if (done) break;
        if (tid < L) S.f_cur[tid] = S.f_nxt[tid];
        flo = fhi;
        __syncthreads();
    }
}

// ---- chunked windows (L <= LCH): a wave loads 64 consecutive records of ONE list per chunk ---------------------------
// Everything that depends on the list — record address, filter coefficient, how many lanes hold a record — is then
// wave-uniform and lives in scalar registers; a lane spends ~10 vector instructions per record.  A window is at most
// MAXCH chunks (sum over the lists of ceil(len/64)); its row in S.off holds the cumulative chunk counts (one byte per list).
struct ChunkRef { uint32_t l, start, cnt; };     // list, index of the chunk's first record in the list, records (0: no chunk)
struct WaveLists { uint32_t rec_lo, rec_hi; float coef; };   // lane l < L keeps list l's record address and filter coefficient
struct WinRow { uint32_t cum, t0, t1, n_ch; };   // lane l <= L: cumulative chunk count before list l, the list's cursors at both window ends

// one row of the window plan, read lane-parallel (lanes past L repeat lane L: no divergence)
__device__ __forceinline__ WinRow win_row(const SliceLds& S, int L, int j, int n_win, int lane) {
    const int li = min(lane, L);
    const int jr = min(j, n_win - 1);      // windows past the end: read the last row (stays in bounds), report no chunks
    const uint8_t* row = reinterpret_cast<const uint8_t*>(S.off) + jr * OSC;
    WinRow w;
    w.cum = row[li];
    w.t0 = S.tbl[jr * L + li];           // lane L reads one entry past the row's lists: the next row's first cursor (unused)
    w.t1 = S.tbl[(jr + 1) * L + min(li, L - 1)];
    w.n_ch = j < n_win ? (uint32_t)__builtin_amdgcn_readlane((int)w.cum, L) : 0u;
    return w;
}

__device__ __forceinline__ ChunkRef chunk_of(const WinRow& w, int L, uint32_t c, int lane) {
    ChunkRef cr{0u, 0u, 0u};
    if (c < w.n_ch && w.n_ch <= (uint32_t)MAXCH) {
        // list = the last one whose cumulative count is <= c (cum_0 = 0; lists without chunks repeat their predecessor's count)
        const unsigned long long m = __ballot(lane < L && w.cum <= c);
        const int l = __builtin_amdgcn_readfirstlane(__popcll(m) - 1);
        const uint32_t rem = c - (uint32_t)__builtin_amdgcn_readlane((int)w.cum, l);
        cr.l = (uint32_t)l;
        cr.start = (uint32_t)__builtin_amdgcn_readlane((int)w.t0, l) + rem * 64u;
        cr.cnt = min(64u, (uint32_t)__builtin_amdgcn_readlane((int)w.t1, l) - cr.start);
    }
    return cr;
}

// Requests window j's records into ring slot S_.  ALWAYS CPW loads per wave — lanes past the chunk's end repeat its last
// record, chunk slots without a chunk (and windows past the end) read a harmless dummy word — so that the number of loads
// in flight behind any slot is a compile-time constant and the wait in front of chunk_add is a counted s_waitcnt vmcnt(N),
// not a drain.  Address = wave-uniform list base + 32-bit lane offset (global_load saddr form: no 64-bit vector math).
template <int S_>
__device__ __forceinline__ void chunk_issue(const WinRow& w, const WaveLists& wl, int L, int wave, int lane, uint64_t dummy,
                                            u32x2 (&rec)[DEPTH][CPW], uint32_t (&cnt)[DEPTH][CPW], float (&cf)[DEPTH][CPW]) {
#pragma unroll
    for (int r = 0; r < CPW; r++) {
        const ChunkRef cr = chunk_of(w, L, (uint32_t)(wave + r * WAVES), lane);
        cnt[S_][r] = cr.cnt;
        uint64_t base = dummy;
        uint32_t voff = 0;
        cf[S_][r] = 0.f;
        if (cr.cnt) {
            base = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)wl.rec_hi, (int)cr.l) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane((int)wl.rec_lo, (int)cr.l);
            cf[S_][r] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(wl.coef), (int)cr.l));
            voff = (cr.start + min((uint32_t)lane, cr.cnt - 1u)) * (uint32_t)sizeof(Rec);
        }
        rec[S_][r] = *(gptr_u2)(base + voff);
    }
}


// filter slot of a doc: doc ids inside a window are a narrow range, so folding the id's low bits spreads them
__device__ __forceinline__ uint32_t fx_slot(uint32_t doc) { return (doc ^ (doc >> SS_SK_BITS)) & (uint32_t)(SK - 1); }

template <int S_>
__device__ __forceinline__ void chunk_add(uint32_t* sk_cur, int lane, const u32x2 (&rec)[DEPTH][CPW], const uint32_t (&cnt)[DEPTH][CPW],
                                          const float (&cf)[DEPTH][CPW], uint32_t (&h)[CPW]) {
#pragma unroll
    for (int r = 0; r < CPW; r++) {
        h[r] = EMPTY;
        if (cnt[S_][r]) {                                        // wave-uniform
            if ((uint32_t)lane < cnt[S_][r]) {
                h[r] = fx_slot(rec[S_][r].x);
                atomicAdd(&sk_cur[h[r]], fx_share(__uint_as_float(rec[S_][r].y), cf[S_][r]));
            }
        }
    }
}

template <int S_>
__device__ __forceinline__ void chunk_filter(const SliceLds& S, const uint32_t (&u)[CPW], uint32_t* sk_prv, uint32_t* surv_cnt_cur, int L, int j, int n_win, int wave, int lane,
                                             uint32_t thr_fx, uint32_t pbase, const u32x2 (&rec)[DEPTH][CPW],
                                             const uint32_t (&h)[CPW], uint32_t (&hprev)[CPW]) {
#pragma unroll
    for (int r = 0; r < CPW; r++) {
        const bool surv = h[r] != EMPTY && u[r] >= thr_fx;
        if (hprev[r] != EMPTY) sk_prv[hprev[r]] = 0u;
        hprev[r] = h[r];
        const unsigned long long m = __ballot(surv);
        if (m) {
            // rare: which list and where — looked up again instead of being carried through the pipeline
            const WinRow w = win_row(S, L, j, n_win, lane);
            const ChunkRef cr = chunk_of(w, L, (uint32_t)(wave + r * WAVES), lane);
            const int leader = __ffsll((long long)m) - 1;
            uint32_t b = 0;
            if (lane == leader) b = atomicAdd(surv_cnt_cur, (uint32_t)__popcll(m));
            b = (uint32_t)__shfl((int)b, leader, 64);
            if (surv) {
                const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
                S.pend[pbase + b + (uint32_t)__popcll(m & below)] = make_uint4(rec[S_][r].x, cr.start + (uint32_t)lane, cr.l, 0u);
            }
        }
    }
}

// NT = threads of the calling workgroup.  FUSED: called by the last slice of the query to finish inside k_score_slices — the
// slices' lists were stored write-through and are read with sc1 loads (no fence; see the hand-off at the end of
// k_score_slices).
// FLAT: the query's slices (k_score_wave) appended their candidates to ONE list per query (qc_cnt[q] entries from
// slice_base[q] * k on); otherwise every slice owns k entries and so_cnt[s] says how many it filled.
constexpr int MERGE_T = 16;     // >= the wave kernel's lists per query (score_wave_max_lists)
size_t merge_lds_bytes(int k, int cb);
template <int NT, bool FUSED, bool FLAT = false>
__device__ __forceinline__ void merge_query(const ScoreParams& p, const uint32_t q, unsigned char* smem, const int cbm) {
    double* accT = reinterpret_cast<double*>(smem);                    // [k]
    double* accB = accT + p.k;                                         // [k]
    double* mgT = accB + p.k;                                          // [k]
    double* mgB = mgT + p.k;                                           // [k]
    uint64_t* cd_key = reinterpret_cast<uint64_t*>(mgB + p.k);         // [cb]
    uint64_t* sc64 = cd_key + cbm;                                     // [1]
    uint32_t* cd_doc = reinterpret_cast<uint32_t*>(sc64 + 1);          // [cb]
    uint32_t* sc32 = cd_doc + cbm;                                     // [4]
    uint64_t* tm_p0 = reinterpret_cast<uint64_t*>(sc32 + 4);           // [MERGE_T] FLAT: the terms' combined lists and multiplicities,
    uint64_t* tm_p1 = tm_p0 + MERGE_T;                                 //           fetched while the candidates are on their way
    uint32_t* tm_mult = reinterpret_cast<uint32_t*>(tm_p1 + MERGE_T);
    TopK tk{cd_key, cd_doc, &sc32[0], &sc64[0], reinterpret_cast<float*>(&sc32[2]), 0ull, -INFINITY, (uint32_t)cbm};
    const int tid = threadIdx.x;
    const int k = p.k;
    if (tid == 0) { sc32[0] = 0; sc32[1] = 0; sc64[0] = 0ull; }
    DIAG_NOWX(t_g0);
    __syncthreads();
    if (FLAT) {
        const uint32_t n = p.qc_cnt[q];
        DIAG_ADD(18, n);
        DIAG_ADD(17, 1);
        const size_t base = (size_t)p.slice_base[q] * k;
        uint32_t* overflow = &sc32[1];
        // two candidates per thread and pass, both loads issued before either is used (no branch around them: a lane without a
        // candidate re-reads entry 0): ~300 candidates per query at config 3 are ONE round of memory latency, not two
        uint64_t key[2];
        uint32_t doc[2];
        bool have[2];
        auto load_pass = [&](uint32_t i0) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const uint32_t i = i0 + (uint32_t)r * NT + tid;
                have[r] = i < n;
                const size_t ii = base + (have[r] ? i : 0u);
                key[r] = p.so_key[ii];
                doc[r] = p.so_doc[ii];
            }
        };
        load_pass(0);
        // what the explain stage needs of the query's terms is requested now, behind the first candidates: these loads (two
        // dependent levels) run beside them instead of after the sort
        {
            const uint32_t tq0 = p.q_off[q], tnd = p.q_off[q + 1] - tq0;
            if ((uint32_t)tid < min(tnd, (uint32_t)MERGE_T)) {
                const uint32_t term = p.dterm[tq0 + tid];
                tm_p0[tid] = p.c_ptr[term];
                tm_p1[tid] = p.c_ptr[term + 1];
                tm_mult[tid] = p.dmult[tq0 + tid];
            }
        }
        __syncthreads();
        if (tid == 0) p.qc_cnt[q] = 0u;                                  // every thread has its copy: zero again for the next batch (no memset between batches)
        for (uint32_t i0 = 0; i0 < n;) {
            for (;;) {
                const uint64_t thr = *tk.thr;
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    if (have[r]) {
                        if (key[r] >= thr) {
                            const uint32_t j = atomicAdd(tk.count, 1u);
                            if (j < tk.cb) { tk.key[j] = key[r]; tk.doc[j] = doc[r]; have[r] = false; }
                            else *overflow = 1;
                        } else {
                            have[r] = false;
                        }
                    }
                }
                __syncthreads();
                if (!*overflow) break;
                topk_compact_net(tk, k);
                if (tid == 0) *overflow = 0;
                __syncthreads();
            }
            i0 += 2 * NT;
            if (i0 < n) load_pass(i0);
        }
    } else
    for (uint32_t s = p.slice_base[q]; s < p.slice_base[q + 1]; s++) {
        const uint32_t n = FUSED ? __hip_atomic_load(&p.so_cnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.so_cnt[s];   // <= k, and cb >= 2k: room after a compaction
        if (sc32[0] + n > tk.cb) topk_compact(tk, k);
        __syncthreads();
        const uint64_t thr = *tk.thr;
        for (uint32_t i = tid; i < n; i += NT) {
            const uint64_t key = FUSED ? __hip_atomic_load(&p.so_key[(size_t)s * k + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.so_key[(size_t)s * k + i];
            if (key >= thr) {
                const uint32_t j = atomicAdd(tk.count, 1u);
                tk.key[j] = key;
                tk.doc[j] = FUSED ? __hip_atomic_load(&p.so_doc[(size_t)s * k + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.so_doc[(size_t)s * k + i];
            }
        }
        __syncthreads();
    }
    if (FLAT) topk_compact_net(tk, k);
    else topk_compact(tk, k);
    const uint32_t n_out = sc32[0];

    // explain: TitleRank/BodyRank of the winners, re-derived from the posting lists
    DIAG_NOWX(t_m0);
    DIAG_ADD(15, t_m0 - t_g0);
    for (uint32_t i = tid; i < n_out; i += NT) { accT[i] = 0.0; accB[i] = 0.0; mgT[i] = 1.0; mgB[i] = 1.0; }
    __syncthreads();
    const uint32_t t0 = p.q_off[q], nd = p.q_off[q + 1] - t0;
    const bool has_phrase = p.ph_off && p.ph_off[q + 1] > p.ph_off[q];
    const uint32_t L = 2 * nd + (has_phrase ? 4u : 0u);
    if (FLAT) {
        // k_score_wave's queries have their combined lists: ONE search per (winner, term) finds the doc's body and title posting
        // side by side, and it runs through the skip index (4 bytes per 64 postings: cache-resident) and then inside one 512-byte
        // block, instead of two interpolation searches over the whole lists (the merge's searches were 58 of its 98 us)
        for (uint32_t task = tid; task < n_out * nd; task += NT) {
            const uint32_t i = task / nd, l = task % nd;
            const uint64_t p0 = tm_p0[l], p1 = tm_p1[l];
            if (p1 == p0) continue;
            const uint32_t d = cd_doc[i];
            const uint32_t g0 = (uint32_t)(p0 >> 6), g1 = (uint32_t)((p1 - 1) >> 6);
            // blocks g0+1 .. g1 start inside the list: the doc's first posting lies in the block before the first entry >= d,
            // or — if that entry IS d — at the very start of the next one: search [block start, next block start + 2)
            const uint32_t gb = g0 + (g1 > g0 ? skip_lower_bound<false>(p.c_skip, g0 + 1, g1 + 1, d) : 0u);
            uint64_t lo = max(p0, (uint64_t)gb << 6), hi = min(p1, ((uint64_t)(gb + 1) << 6) + 2);
            const uint64_t list_addr = (uint64_t)p.c_rec;
            // a plain binary search (seven dependent probes): the merge is bound by the NUMBER of scattered loads its 300 searches
            // per query issue, not by their latency — an 8-ary search in two steps (15 probes) made the explain 37 % slower
            while (lo < hi) {                                        // first position with doc >= d
                const uint64_t mid = (lo + hi) >> 1;
                if ((load_doc(list_addr, mid) & 0x7FFFFFFFu) < d) lo = mid + 1; else hi = mid;
            }
            const double mult = (double)tm_mult[l];
            for (uint64_t pos = lo; pos < min(p1, lo + 2); pos++) {  // body first, then title, of the same doc
                const uint32_t rd = load_doc(list_addr, pos);
                if ((rd & 0x7FFFFFFFu) != d) break;
                const int field = (int)(rd >> 31);
                const double v = (double)p.c_w[pos] * mult;
                const double mag = (field ? p.t_mag : p.b_mag)[d];
                if (field) { atomicAdd(&accT[i], v); mgT[i] = mag; }
                else { atomicAdd(&accB[i], v); mgB[i] = mag; }
            }
        }
    } else
    for (uint32_t task = tid; task < n_out * L; task += NT) {
        const uint32_t i = task / L, l = task % L;
        const int field = l & 1;
        uint64_t addr, waddr;
        uint32_t len;
        double mult;
        if (l < 2 * nd) {
            const uint32_t term = p.dterm[t0 + (l >> 1)];
            const uint64_t* ptr = field ? p.t_ptr : p.b_ptr;
            addr = (uint64_t)((field ? p.t_rec : p.b_rec) + ptr[term]);
            waddr = (uint64_t)((field ? p.t_w : p.b_w) + ptr[term]);
            len = (uint32_t)(ptr[term + 1] - ptr[term]);
            mult = (double)p.dmult[t0 + (l >> 1)];
        } else {
            addr = (uint64_t)(x_rec_of(p, (int)(l - 2 * nd)) + p.x_off[q]);
            waddr = (uint64_t)(x_w_of(p, (int)(l - 2 * nd)) + p.x_off[q]);
            len = p.x_cnt[(size_t)q * 4 + (l - 2 * nd)];
            mult = 1.0;
        }
        const uint32_t d = cd_doc[i];
        const uint32_t pos = lower_bound_interp(addr, 0, len, d);
        if (pos < len && load_doc(addr, pos) == d) {
            const double v = (double)load_w(waddr, pos) * mult;
            const double mag = (field ? p.t_mag : p.b_mag)[d];
            if (field) { atomicAdd(&accT[i], v); mgT[i] = mag; }
            else { atomicAdd(&accB[i], v); mgB[i] = mag; }
        }
    }
    __syncthreads();
    DIAG_NOWX(t_m1);
    DIAG_ADD(14, t_m1 - t_m0);
    const double qmag = p.qmag[q];
    const double* probs = (p.probs && p.prior) ? p.probs + (size_t)q * p.k_topics : nullptr;
    for (uint32_t i = tid; i < (uint32_t)k; i += NT) {
        ss_hit h;
        h.doc = 0; h._pad = 0; h.title = 0.0; h.body = 0.0; h.pagerank = 0.0; h.final = 0.0;
        if (i < n_out) {
            const uint32_t d = cd_doc[i];
            const double sqd = probs ? topic_dot(p.prior, probs, p.k_topics, d) : 0.0;
            double title, body, fin;
            final_rank(accT[i], accB[i], mgT[i], mgB[i], qmag, sqd, title, body, fin);
            h.doc = d; h.title = title; h.body = body; h.pagerank = sqd; h.final = fin;
        }
        p.hits[(size_t)q * k + i] = h;
    }
    if (tid == 0) p.n_hits[q] = (int32_t)n_out;
    DIAG_NOWX(t_m2);
    DIAG_ADD(16, t_m2 - t_m1);
}


// MASKED: the instantiation for calls in which some query has an allow-list (ss_score_topk_masked); the other one has no trace of it
template <bool MASKED>
__global__ __launch_bounds__(TPB, (TPB / 256) * SS_WGS_PER_CU) void k_score_slices(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ScoreLds lo_ = score_lds_layout(p.cb);
    uint64_t* sc64 = reinterpret_cast<uint64_t*>(smem + lo_.sc64);        // [0]: thr
    uint64_t* cd_key = reinterpret_cast<uint64_t*>(smem + lo_.cd_key);    // [cb]
    uint32_t* cd_doc = reinterpret_cast<uint32_t*>(smem + lo_.cd_doc);    // [cb]
    uint32_t* sc32 = reinterpret_cast<uint32_t*>(smem + lo_.sc32);        // [16] scalars
    SliceLds S;
    S.s_rec = reinterpret_cast<double2*>(smem + lo_.s_rec);
    S.pend = reinterpret_cast<uint4*>(smem + lo_.s_rec);
    S.l_rec = reinterpret_cast<uint64_t*>(smem + lo_.l_rec);
    S.l_w = reinterpret_cast<uint64_t*>(smem + lo_.l_w);
    S.ht_key = reinterpret_cast<uint32_t*>(smem + lo_.ht_key);
    S.ht_rec = reinterpret_cast<uint32_t*>(smem + lo_.ht_rec);
    S.sk = reinterpret_cast<uint32_t*>(smem + lo_.sk);
    S.tbl = reinterpret_cast<uint32_t*>(smem + lo_.tbl);
    S.l_mult = reinterpret_cast<uint32_t*>(smem + lo_.l_mult);
    S.l_field = reinterpret_cast<uint32_t*>(smem + lo_.l_field);
    S.f_cur = reinterpret_cast<uint32_t*>(smem + lo_.f_cur);
    S.f_nxt = reinterpret_cast<uint32_t*>(smem + lo_.f_nxt);
    S.l_coef = reinterpret_cast<float*>(smem + lo_.l_coef);
    S.off = reinterpret_cast<uint16_t*>(smem + lo_.off);
    S.overflow = &sc32[1];
    S.sel = reinterpret_cast<uint32_t*>(smem + lo_.sel);
    S.sel64 = reinterpret_cast<uint64_t*>(smem + lo_.sel64);

    uint32_t& cand_count = sc32[0];
    float* thr_f_s = reinterpret_cast<float*>(&sc32[2]);
    uint32_t* surv_cnt = &sc32[4];                  // [3] survivors appended by window j: surv_cnt[j % 3]
    uint32_t* thr0_bits = &sc32[8];                 // slice set-up: max of the lists' bounds (non-negative floats order like their bits)
    uint32_t* coef_max_bits = &sc32[9];             // slice set-up: largest filter coefficient of the query's lists

    const int tid = threadIdx.x, lane = tid & 63;
    DIAG_NOW(t_k0);
#ifdef SS_DIAG
    const unsigned long long t_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t slice_id = p.order[blockIdx.x];
    const SliceDesc sd = p.slices[slice_id];
    const uint32_t q = sd.q;
    const uint32_t t0 = p.q_off[q], nd = p.q_off[q + 1] - t0;
    const bool has_phrase = p.ph_off && p.ph_off[q + 1] > p.ph_off[q];
    const int L = (int)(2 * nd) + (has_phrase ? 4 : 0);
    SliceQuery Q;
    Q.qmag = p.qmag[q];
    Q.probs = (p.probs && p.prior) ? p.probs + (size_t)q * p.k_topics : nullptr;
    Q.sqd_ub = Q.probs ? p.sqd_ub[q] : 0.0;
    Q.sqd_ub_f = Q.probs ? __double2float_ru(Q.sqd_ub) : 0.0f;
    Q.qmag_f = (float)Q.qmag;
    const int32_t mask_id = MASKED ? p.q_mask[q] : -1;
    Q.mask = mask_id >= 0 ? p.masks + (size_t)mask_id * p.mask_words : nullptr;
    // filter: upper bound of the prior's share of FinalRank, 0.33*sqd*100 (get_metadata.go:69), with the filter's margin
    const float r_ub = Q.probs ? __double2float_ru(33.0 * Q.sqd_ub * (1.0 + 0x1p-12)) : 0.0f;
    const bool exact_all = p.exact_all != 0;

    for (int i = tid; i < HT; i += TPB) { S.ht_key[i] = EMPTY; S.ht_rec[i] = EMPTY; }
    for (int i = tid; i < 3 * SK; i += TPB) S.sk[i] = 0u;
    if (tid == 0) { cand_count = 0; *S.overflow = 0; sc64[0] = 0ull; *thr_f_s = -INFINITY; surv_cnt[0] = surv_cnt[1] = surv_cnt[2] = 0; *thr0_bits = 0; *coef_max_bits = 0; }

    // ---- slice set-up: where every list enters and leaves the slice's doc range ----
    uint32_t* t_lo = S.tbl;                 // row 0 of the table
    uint32_t* t_hi = S.f_nxt;               // parked here until n_win is known
    __syncthreads();
    if (tid < L) {
        const int field = tid & 1;                     // 0 = body, 1 = title (also for the phrase lists)
        uint64_t addr, waddr;
        uint32_t len, mult;
        float kth = 0.0f;
        if (tid < (int)(2 * nd)) {
            const uint32_t term = p.dterm[t0 + (tid >> 1)];
            const uint64_t* ptr = field ? p.t_ptr : p.b_ptr;
            const uint64_t p0 = ptr[term];
            addr = (uint64_t)((field ? p.t_rec : p.b_rec) + p0);
            waddr = (uint64_t)((field ? p.t_w : p.b_w) + p0);
            len = (uint32_t)(ptr[term + 1] - p0);
            mult = p.dmult[t0 + (tid >> 1)];
            kth = (field ? p.t_kth : p.b_kth)[(size_t)term * KTH_N + p.kth_j];
        } else {
            // phrase contributions are appended once, after the terms (main_retrieve.go:73-78)
            const int x = tid - (int)(2 * nd);
            addr = (uint64_t)(x_rec_of(p, x) + p.x_off[q]);
            waddr = (uint64_t)(x_w_of(p, x) + p.x_off[q]);
            len = p.x_cnt[(size_t)q * 4 + x];
            mult = 1;
        }
        S.l_rec[tid] = addr;
        S.l_w[tid] = waddr;
        S.l_mult[tid] = mult;
        S.l_field[tid] = field;
        S.f_cur[tid] = len;
        // FinalRank's share of one record is (38|29) * mult * (w/mag) / sqrt(queryLength) (get_metadata.go:57-58,69).
        // Filter coefficient: rounded up with a 2^-12 margin that covers every float rounding of the filter's sums;
        // threshold floor: the same rounded down, times the list's k'-th largest impact (k' >= k distinct documents
        // score at least their own contribution when every other addend is >= 0).
        const double share = (field ? 38.0 : 29.0) * (double)mult / Q.qmag;
        const float coef = __double2float_ru(share * (1.0 + 0x1p-12));
        S.l_coef[tid] = coef;
        if (coef > 0.0f && coef < INFINITY) atomicMax(coef_max_bits, __float_as_uint(coef));
        // (no floor under an allow-list: the k' best postings of a list need not be k' docs the query may return)
        if (!exact_all && !Q.mask && kth > 0.0f) {
            const float floor_l = __double2float_rd(share * (1.0 - 0x1p-12) * (double)kth);
            if (floor_l > 0.0f) atomicMax(thr0_bits, __float_as_uint(floor_l));
        }
    }
    __syncthreads();
    DIAG_NOW(t_s1);
    DIAG_ADD(6, t_s1 - t_k0);
    if (tid < 2 * L) {                      // the two bounds of a list by two threads: independent search chains
        const int l = tid >> 1;
        if (tid & 1) t_hi[l] = sd.dhi == 0xFFFFFFFFu ? S.f_cur[l] : lower_bound_interp(S.l_rec[l], 0, S.f_cur[l], sd.dhi);
        else t_lo[l] = sd.dlo == 0 ? 0u : lower_bound_interp(S.l_rec[l], 0, S.f_cur[l], sd.dlo);
    }
    __syncthreads();
    DIAG_NOW(t_s2);
    DIAG_ADD(7, t_s2 - t_s1);
    // fixed-point scale of the filter: the largest coefficient (an impact of 1.0 in that list) = FX_ONE units
    const float coef_max = __uint_as_float(*coef_max_bits);
    const float fx_scale = coef_max > 0.0f ? (float)FX_ONE / coef_max : 1.0f;
    const float thr0_f = __uint_as_float(*thr0_bits);
    const uint64_t thr0_key = thr0_f > 0.0f ? fkey((double)thr0_f) : 0ull;
    if (tid < L) S.l_coef[tid] = S.l_coef[tid] * fx_scale * (1.0f + 0x1p-20f);     // filter coefficients in fixed-point units from here on
    const TopK tk{cd_key, cd_doc, &sc32[0], &sc64[0], thr_f_s, thr0_key, thr0_f > 0.0f ? thr0_f : -INFINITY, (uint32_t)p.cb};
    if (tid == 0 && thr0_f > 0.0f) { sc64[0] = thr0_key; *thr_f_s = thr0_f; }
    // every thread: total, driver (longest list in the slice), number of windows
    uint32_t tot = 0, drv = 0, drv_len = 0;
    for (int l = 0; l < L; l++) {
        const uint32_t len = t_hi[l] - t_lo[l];
        tot += len;
        if (len > drv_len) { drv_len = len; drv = l; }
    }
    const bool chunked = L <= LCH;
    int n_win = 0;
    if (tot) {
        if (chunked) {
            // mean 13.5 of the MAXCH = 16 chunks per window: every non-empty list wastes half a chunk per window on
            // average, and the counts fluctuate (sigma ~0.6 chunks); more than MAXCH falls back to the oversize path
            int l_ne = 0;
            for (int l = 0; l < L; l++) l_ne += t_hi[l] != t_lo[l];
            const uint32_t tgt = (uint32_t)max(192, (MAXCH * 64 * 27) / 32 - 34 * l_ne);
            n_win = (int)((tot + tgt - 1) / tgt);
            n_win = min(n_win, min(MAX_WIN, min(TBL_CAP / L - 1, (int)(OFF_CAP * 2 / OSC))));
        } else {
            n_win = (int)((tot + TARGET - 1) / TARGET);
            n_win = min(n_win, min(MAX_WIN, min(TBL_CAP / L - 1, OFF_CAP / (L + 1))));
        }
        n_win = max(n_win, 1);
    }
    const int OS = L + 1;                   // generic loop: row stride of `off`; the window's record count sits in the row's last entry
    // window j covers docs [b_j, b_{j+1}), b_j = doc of the driver's record at j/n_win of its run:
    // all cursors are known up front (no per-window serial planning; windows fill evenly because
    // the other lists simply contribute whatever falls into the driver's doc range)
    const uint64_t drv_addr = S.l_rec[drv];
    for (int idx = tid; idx < (n_win - 1) * L; idx += TPB) {
        const int j = idx / L + 1, l = idx - (j - 1) * L;
        const uint32_t b = load_doc(drv_addr, t_lo[drv] + (uint64_t)j * drv_len / n_win);
        S.tbl[j * L + l] = lower_bound_interp(S.l_rec[l], t_lo[l], t_hi[l], b);
    }
    __syncthreads();
    if (tid < L && n_win) S.tbl[n_win * L + tid] = t_hi[tid];
    __syncthreads();
    if (chunked) {
        uint8_t* off8 = reinterpret_cast<uint8_t*>(S.off);
        for (int j = tid; j < n_win; j += TPB) {
            uint32_t cum = 0, recs = 0;
            for (int l = 0; l < L; l++) {
                off8[j * OSC + l] = (uint8_t)min(cum, 255u);
                const uint32_t len = S.tbl[(j + 1) * L + l] - S.tbl[j * L + l];
                cum += (len + 63u) >> 6;
                recs += len;
            }
            off8[j * OSC + L] = (uint8_t)min(cum, 255u);      // > MAXCH: oversize window
            off8[j * OSC + L + 1] = (uint8_t)min((recs + 7u) >> 3, 255u);   // records / 8, rounded up (<= MAXCH * 64 / 8 = 128 for a regular window)
        }
    } else {
        for (int j = tid; j < n_win; j += TPB) {
            uint32_t run = 0;
            for (int l = 0; l < OS - 1; l++) {
                S.off[j * OS + l] = (uint16_t)min(run, 0xFFFFu);
                run += S.tbl[(j + 1) * L + l] - S.tbl[j * L + l];
            }
            S.off[j * OS + OS - 1] = (uint16_t)min(run, 0xFFFFu);      // > CAP: oversize window
        }
    }
    __syncthreads();

    DIAG_NOW(t_k1);
    DIAG_ADD(0, 1);
    DIAG_ADD(1, n_win);
    DIAG_ADD(5, tot);
    DIAG_ADD(9, t_k1 - t_k0);
    // ---- the windows ----
    // the threshold in the filter's units: it only moves when the exact stage runs (recomputed after every flush)
    uint32_t thr_fx = exact_all ? 0u : fx_threshold(*thr_f_s, r_ub, fx_scale);
    uint32_t pbase = 0;                     // pending survivors of the windows before this one (same value in every thread)
    int cur = 0, prv = 2;                   // j % 3, (j - 1) % 3
    if (chunked && n_win > 0) {
        const int wave = tid >> 6;
        WaveLists wl{0u, 0u, 0.f};
        if (lane < L) {
            const uint64_t a = S.l_rec[lane];
            wl.rec_lo = (uint32_t)a;
            wl.rec_hi = (uint32_t)(a >> 32);
            wl.coef = S.l_coef[lane];
        }
        u32x2 rec[DEPTH][CPW];
        uint32_t cnt[DEPTH][CPW];
        float cf[DEPTH][CPW];
        uint32_t hprev[CPW];
#pragma unroll
        for (int r = 0; r < CPW; r++) {
            hprev[r] = EMPTY;
#pragma unroll
            for (int d = 0; d < DEPTH; d++) { rec[d][r] = u32x2{0u, 0u}; cnt[d][r] = 0; cf[d][r] = 0.f; }
        }
        const uint8_t* off8 = reinterpret_cast<const uint8_t*>(S.off);
        // windows 0 .. DEPTH-1 go in flight before the loop; window j + DEPTH is requested at the end of step j.
        // The loop is unrolled by DEPTH so that ring slots and filter tables are compile-time constants; the window
        // count is padded to a multiple of DEPTH with empty windows (no records, same instruction sequence).
        const uint64_t dummy = (uint64_t)p.q_off;      // 8 readable bytes for lanes without a record
        chunk_issue<0>(win_row(S, L, 0, n_win, lane), wl, L, wave, lane, dummy, rec, cnt, cf);
        chunk_issue<1>(win_row(S, L, 1, n_win, lane), wl, L, wave, lane, dummy, rec, cnt, cf);
        chunk_issue<2>(win_row(S, L, 2, n_win, lane), wl, L, wave, lane, dummy, rec, cnt, cf);
#define SS_CHUNK_STEP(S_, JJ)                                                                                              \
        {                                                                                                                  \
            const int j_ = (JJ);                                                                                           \
            constexpr int nxt_ = (S_ + 1) % 3, prv_ = (S_ + 2) % 3;                                                        \
            const uint32_t n_ch = j_ < n_win ? off8[j_ * OSC + L] : 0u;                                                    \
            const uint32_t n_rec = j_ < n_win ? 8u * off8[j_ * OSC + L + 1] : 0u;                                          \
            const bool normal = n_ch <= (uint32_t)MAXCH;                                                                   \
            uint32_t* sk_cur = S.sk + S_ * SK;                                                                             \
            uint32_t* sk_prv = S.sk + prv_ * SK;                                                                           \
            uint32_t h[CPW], u[CPW];                                                                                       \
            /* stage 1a: every record adds its share into its doc's slot (waits for THIS window's records only) */        \
            DIAG_NOWL(t_a0_);                                                                                              \
            chunk_add<S_>(sk_cur, lane, rec, cnt, cf, h);                                                                  \
            DIAG_NOWL(t_a1_);                                                                                              \
            lds_barrier();                                                                                                 \
            DIAG_NOWL(t_a2_);                                                                                              \
            DIAG_ADDL(12, t_a1_ - t_a0_);                                                                                   \
            DIAG_ADDL(13, t_a2_ - t_a1_);                                                                                   \
            /* ONE round of LDS latency for everything the rest of the step needs: the survivor count of the previous */  \
            /* window (complete now, stable until its counter is re-used), this window's slots, the plan row of the   */  \
            /* window that is requested next                                                                          */  \
            const uint32_t sc_ = surv_cnt[prv_];                                                                           \
            _Pragma("unroll") for (int r = 0; r < CPW; r++) u[r] = sk_cur[h[r] & (uint32_t)(SK - 1)];                      \
            const WinRow row_ = win_row(S, L, j_ + DEPTH, n_win, lane);                                                    \
            pbase += sc_;                                                                                                  \
            if (tid == 0) surv_cnt[nxt_] = 0;                                                                              \
            if (!normal || pbase + n_rec > (uint32_t)PC) {                                                                 \
                if (pbase) flush_pending(S, tk, Q, p, tid, pbase);                                                         \
                pbase = 0;                                                                                                 \
                if (!normal) oversize_window(S, tk, Q, p, tid, L, j_, n_win, sd, drv, drv_addr);                           \
                thr_fx = exact_all ? 0u : fx_threshold(*thr_f_s, r_ub, fx_scale);                                          \
            }                                                                                                              \
            /* stage 1b: the slot bounds the doc's FinalRank from above; below the threshold -> drop.  Then the records */ \
            /* of window j + DEPTH are requested into the registers this window has just released.                    */ \
            chunk_filter<S_>(S, u, sk_prv, &surv_cnt[S_], L, j_, n_win, wave, lane, thr_fx, pbase, rec, h, hprev);         \
            chunk_issue<S_>(row_, wl, L, wave, lane, dummy, rec, cnt, cf);                                                 \
        }
        for (int j = 0; j < n_win; j += DEPTH) {
            SS_CHUNK_STEP(0, j)
            SS_CHUNK_STEP(1, j + 1)
            SS_CHUNK_STEP(2, j + 2)
        }
#undef SS_CHUNK_STEP
        prv = 2;                                // the padded window count is a multiple of 3: the last step used counter 2
    } else if (!chunked) {
        u32x2 rec[PPT];
        uint32_t rl[PPT], ri[PPT];
        float rc[PPT];
#pragma unroll
        for (int r = 0; r < PPT; r++) { rl[r] = EMPTY; ri[r] = 0; rc[r] = 0.f; rec[r] = u32x2{0u, 0u}; }
        uint32_t hprev[PPT];                // filter slots this thread touched in the previous window (EMPTY: none)
#pragma unroll
        for (int r = 0; r < PPT; r++) hprev[r] = EMPTY;
        bool have = false;                  // window j's records are in flight / in registers
        for (int j = 0; j < n_win; j++) {
            const uint32_t n = S.off[j * OS + OS - 1];
            const int nxt = cur == 2 ? 0 : cur + 1;
            const bool normal = n <= (uint32_t)CAP;
            if (normal && !have) load_window(S, j, L, OS, tid, rec, rl, ri, rc);     // first window, or the one after an oversize window
            have = false;
            uint32_t h[PPT];
            u32x2 mine[PPT];
            uint32_t ml[PPT], mi[PPT];
            uint32_t* sk_cur = S.sk + cur * SK;
            if (normal) {
                // stage 1a: every record adds its share into its doc's slot (waits for window j's records)
#pragma unroll
                for (int r = 0; r < PPT; r++) {
                    h[r] = EMPTY;
                    if (rl[r] != EMPTY) {
                        h[r] = fx_slot(rec[r].x);
                        atomicAdd(&sk_cur[h[r]], fx_share(__uint_as_float(rec[r].y), rc[r]));
                    }
                    mine[r] = rec[r]; ml[r] = rl[r]; mi[r] = ri[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < PPT; r++) { h[r] = EMPTY; ml[r] = EMPTY; mi[r] = 0; mine[r] = u32x2{0u, 0u}; }
            }
            lds_barrier();
            // survivors of window j-1 are all appended now; their count is stable until window j+2 re-uses the counter
            pbase += surv_cnt[prv];
            if (tid == 0) surv_cnt[nxt] = 0;
            if (!normal || pbase + n > (uint32_t)PC) {
                if (pbase) flush_pending(S, tk, Q, p, tid, pbase);
                pbase = 0;
                if (!normal) oversize_window(S, tk, Q, p, tid, L, j, n_win, sd, drv, drv_addr);
                thr_fx = exact_all ? 0u : fx_threshold(*thr_f_s, r_ub, fx_scale);
            }
            // put the next window's loads in flight
            if (j + 1 < n_win && S.off[(j + 1) * OS + OS - 1] <= CAP) {
                load_window(S, j + 1, L, OS, tid, rec, rl, ri, rc);
                have = true;
            }
            // stage 1b: the slot now bounds the doc's FinalRank from above; below the threshold -> drop.
            // (An oversize window has no records here: only the previous window's slots are cleared.)
            uint32_t* sk_prv = S.sk + prv * SK;
#pragma unroll
            for (int r = 0; r < PPT; r++) {
                bool surv = false;
                if (ml[r] != EMPTY) surv = sk_cur[h[r]] >= thr_fx;
                if (hprev[r] != EMPTY) sk_prv[hprev[r]] = 0u;
                hprev[r] = h[r];
                const unsigned long long m = __ballot(surv);
                if (m) {
                    const int leader = __ffsll((long long)m) - 1;
                    uint32_t b = 0;
                    if (lane == leader) b = atomicAdd(&surv_cnt[cur], (uint32_t)__popcll(m));
                    b = (uint32_t)__shfl((int)b, leader, 64);
                    if (surv) {
                        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
                        S.pend[pbase + b + (uint32_t)__popcll(m & below)] = make_uint4(mine[r].x, mi[r], ml[r], 0u);
                    }
                }
            }
            prv = cur;
            cur = nxt;
        }
    }
    lds_barrier();
    pbase += surv_cnt[prv];
    if (pbase) flush_pending(S, tk, Q, p, tid, pbase);
    DIAG_NOW(t_k2);
    DIAG_ADD(10, t_k2 - t_k1);

    topk_cut(tk, p.k, S.sel, S.sel64);  // (the slice's list goes to the merge unordered: merge_query filters and sorts what it gathers)
    const uint32_t n_out = cand_count;
    if (!p.q_ticket) {
        for (uint32_t i = tid; i < n_out; i += TPB) {
            p.so_key[(size_t)slice_id * p.k + i] = cd_key[i];
            p.so_doc[(size_t)slice_id * p.k + i] = cd_doc[i];
        }
        if (tid == 0) p.so_cnt[slice_id] = n_out;
    } else {
        // Fused merge: the slice's list goes out write-through (sc1), every wave drains its stores, one lane takes the
        // query's ticket; the slice that arrives last merges the query right here while other workgroups are still
        // scoring — no second launch, no fence (the readers use sc1 loads; MI355X_MICROARCH.md, hand-off forms).
        for (uint32_t i = tid; i < n_out; i += TPB) {
            __hip_atomic_store(&p.so_key[(size_t)slice_id * p.k + i], cd_key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&p.so_doc[(size_t)slice_id * p.k + i], cd_doc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) __hip_atomic_store(&p.so_cnt[slice_id], n_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        uint32_t* last_flag = reinterpret_cast<uint32_t*>(smem);   // the slice's LDS is free from here on
        if (tid == 0) {
            const uint32_t n_sl = p.slice_base[sd.q + 1] - p.slice_base[sd.q];
            const uint32_t prev = __hip_atomic_fetch_add(&p.q_ticket[sd.q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = prev == n_sl - 1;
            if (last) __hip_atomic_store(&p.q_ticket[sd.q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
            *last_flag = last ? 1u : 0u;
        }
        __syncthreads();
        const bool last = *last_flag != 0;
        __syncthreads();
        if (last) merge_query<TPB, true>(p, sd.q, smem, p.cb);
    }
    DIAG_NOW(t_k3);
    DIAG_ADD(11, t_k3 - t_k0);
#ifdef SS_DIAG
    if (tid == 0 && blockIdx.x < 4096) {
        g_slice[blockIdx.x][0] = t_r0;
        g_slice[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
        g_slice[blockIdx.x][2] = (unsigned long long)n_win;
        g_slice[blockIdx.x][3] = tot;
    }
#endif
}

// ---- K6: quoted-phrase matching (retrieval/phrase.go:11-170, util.go:162-203) --------------------
// One workgroup per query with a phrase.  Candidates = the docs of the phrase's rarest term (its body
// postings, then its title-only postings); a thread takes one candidate doc and
//   * looks the doc up in the body and title lists of every phrase term (binary search): the doc must have
//     an entry for EVERY term position, in body or title (phrase.go:63);
//   * per field: every term must be present in that field, the float32 weights are summed in phrase
//     order (phrase.go:59,69,73,83,90) and the position lists, shifted by the term's index
//     (getPosTerm :145,:157: listPos[i] -= float32(pos)), must have a common value (intersect,
//     util.go:179-203; bit-exact float32 equality as in the reference);
//   * matches leave as scoring records {doc, impact of the float32 sum} + the sum itself, in doc order (ordered
//     compaction), i.e. as ordinary doc-sorted lists that k_score_slices merges like any term list
//     (main_retrieve.go:73-78).
constexpr int PH_TPB = 256;
constexpr int PH_MAX = 16;       // phrase terms (SS_MAX_PHRASE_TERMS)

__device__ __forceinline__ bool positions_chain(const uint64_t* const* pos_ptr2, const float* const* pos2, int field,
                                                const int32_t* my_post, int m) {
    // S = A_0; S = S ∩ (A_i - i) for i = 1..m-1; non-empty?
    const uint64_t* pp = pos_ptr2[field];
    const float* ps = pos2[field];
    const uint64_t a_beg = pp[my_post[0]], a_end = pp[my_post[0] + 1];
    for (uint64_t a = a_beg; a < a_end; a++) {
        const float v = ps[a] - 0.0f;
        bool alive = true;
        for (int i = 1; i < m && alive; i++) {
            const uint64_t b_beg = pp[my_post[i * PH_TPB]], b_end = pp[my_post[i * PH_TPB] + 1];
            bool found = false;
            for (uint64_t b = b_beg; b < b_end; b++)
                if (ps[b] - (float)i == v) { found = true; break; }
            alive = found;
        }
        if (alive) return true;
    }
    return false;
}

// float32 upper bound of w / mag for the filter; 0 where the weight is 0 (0/0 = NaN -> 0 in the reference too)
__device__ __forceinline__ float impact_of(float w, double mag) {
    if (w == 0.0f) return 0.0f;
    return __double2float_ru((double)w / mag);
}

__global__ __launch_bounds__(PH_TPB) void k_phrase_match(ScoreParams p) {
    __shared__ int32_t s_pb[PH_MAX * PH_TPB];     // body posting index of term i for this thread's doc, -1 = none
    __shared__ int32_t s_pt[PH_MAX * PH_TPB];
    __shared__ uint32_t s_wave[2][PH_TPB / 64];
    __shared__ uint32_t s_base[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint4 part = p.ph_parts[blockIdx.x];
    const uint32_t q = part.x;
    const int pass = (int)part.y;
    const uint32_t f0 = p.ph_off[q], m = p.ph_off[q + 1] - f0;
    const uint32_t drv_term = p.ph_terms[f0 + p.ph_drv[q]];
    const uint64_t* pos_ptr2[2] = {p.b_pos_ptr, p.t_pos_ptr};
    const float* pos2[2] = {p.b_pos, p.t_pos};
    int32_t* my_pb = s_pb + tid;
    int32_t* my_pt = s_pt + tid;
    if (tid < 2) s_base[tid] = 0;
    __syncthreads();
    // pass 0: driver's body postings; pass 1: driver's title postings whose doc has no driver body posting
    const uint64_t l0 = pass == 0 ? p.b_ptr[drv_term] : p.t_ptr[drv_term];
    const uint64_t c0 = l0 + part.z, c1 = c0 + part.w;
    const Rec* crec = pass == 0 ? p.b_rec : p.t_rec;
    const uint32_t out0 = p.x_off[q] + part.z;    // the part's matches go out compactly from its first candidate's slot
    for (uint64_t cb = c0; cb < c1; cb += PH_TPB) {
        const uint64_t ci = cb + tid;
        bool body_ok = false, title_ok = false;
        float sum_b = 0.0f, sum_t = 0.0f;
        uint32_t d = 0;
        if (ci < c1) {
            d = crec[ci].doc;
            bool all = true, body_all = true, title_all = true;
            if (pass == 1) {
                const uint64_t b0 = p.b_ptr[drv_term], b1 = p.b_ptr[drv_term + 1];
                const uint64_t pos = lower_bound_rec_interp(p.b_rec, b0, b1, d);
                if (pos < b1 && p.b_rec[pos].doc == d) all = false;       // already handled in pass 0
            }
            for (uint32_t i = 0; i < m && all; i++) {
                const uint32_t term = p.ph_terms[f0 + i];
                const uint64_t b0 = p.b_ptr[term], b1 = p.b_ptr[term + 1];
                const uint64_t t0 = p.t_ptr[term], t1 = p.t_ptr[term + 1];
                const uint64_t pb = lower_bound_rec_interp(p.b_rec, b0, b1, d);
                const uint64_t pt = lower_bound_rec_interp(p.t_rec, t0, t1, d);
                const bool hb = pb < b1 && p.b_rec[pb].doc == d, ht = pt < t1 && p.t_rec[pt].doc == d;
                my_pb[i * PH_TPB] = hb ? (int32_t)pb : -1;
                my_pt[i * PH_TPB] = ht ? (int32_t)pt : -1;
                if (!hb && !ht) all = false;                      // phrase.go:63
                if (hb) sum_b += p.b_w[pb]; else body_all = false;          // phrase.go:69,80-84
                if (ht) sum_t += p.t_w[pt]; else title_all = false;         // phrase.go:73,87-91
            }
            if (all) {
                if (body_all) body_ok = positions_chain(pos_ptr2, pos2, 0, my_pb, (int)m);
                if (title_all) title_ok = positions_chain(pos_ptr2, pos2, 1, my_pt, (int)m);
            }
        }
        // ordered compaction of the matches of this chunk (keeps the lists doc-sorted)
        const unsigned long long mb = __ballot(body_ok), mt = __ballot(title_ok);
        if (lane == 0) { s_wave[0][wave] = (uint32_t)__popcll(mb); s_wave[1][wave] = (uint32_t)__popcll(mt); }
        __syncthreads();
        uint32_t ob = s_base[0], ot = s_base[1];
        for (int w2 = 0; w2 < wave; w2++) { ob += s_wave[0][w2]; ot += s_wave[1][w2]; }
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        if (body_ok) {
            const uint32_t o = out0 + ob + (uint32_t)__popcll(mb & below);
            const int x = pass == 0 ? 0 : 2;
            Rec r;
            r.doc = d; r.imp = impact_of(sum_b, p.b_mag[d]);
            x_rec_of(p, x)[o] = r;
            x_w_of(p, x)[o] = sum_b;
        }
        if (title_ok) {
            const uint32_t o = out0 + ot + (uint32_t)__popcll(mt & below);
            const int x = pass == 0 ? 1 : 3;
            Rec r;
            r.doc = d; r.imp = impact_of(sum_t, p.t_mag[d]);
            x_rec_of(p, x)[o] = r;
            x_w_of(p, x)[o] = sum_t;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t tb = 0, tt = 0;
            for (int w2 = 0; w2 < PH_TPB / 64; w2++) { tb += s_wave[0][w2]; tt += s_wave[1][w2]; }
            s_base[0] += tb;
            s_base[1] += tt;
        }
        __syncthreads();
    }
    if (tid < 2) p.ph_pcnt[(size_t)blockIdx.x * 2 + tid] = s_base[tid];
}

// Per query: the parts' match runs, each compact from its own offset, are moved down into one contiguous doc-sorted list
// per result kind (in part order = doc order), and the four counts are written.  Only matches move.
__global__ __launch_bounds__(PH_TPB) void k_phrase_close(ScoreParams p) {
    const uint32_t q = blockIdx.x;
    const int tid = threadIdx.x;
    uint32_t run[4] = {0u, 0u, 0u, 0u};
    const uint32_t base = p.x_off[q];
    for (uint32_t pi = p.ph_pbase[q]; pi < p.ph_pbase[q + 1]; pi++) {
        const uint4 part = p.ph_parts[pi];
        for (int kind = 0; kind < 2; kind++) {
            const int x = (int)part.y * 2 + kind;
            const uint32_t n = p.ph_pcnt[(size_t)pi * 2 + kind];
            const uint32_t src = base + part.z, dst = base + run[x];
            if (n && src != dst) {
                Rec* xr = x_rec_of(p, x);
                float* xw = x_w_of(p, x);
                // dst < src and the ranges may overlap: a chunk is read whole before it is written
                for (uint32_t i0 = 0; i0 < n; i0 += PH_TPB) {
                    const uint32_t i = i0 + (uint32_t)tid;
                    Rec r{};
                    float w = 0.f;
                    if (i < n) { r = xr[src + i]; w = xw[src + i]; }
                    __syncthreads();
                    if (i < n) { xr[dst + i] = r; xw[dst + i] = w; }
                    __syncthreads();
                }
            }
            run[x] += n;
        }
    }
    if (tid < 4) p.x_cnt[(size_t)q * 4 + tid] = run[tid];
}

size_t score_lds_bytes(int cb) { return score_lds_layout(cb).total; }

// ---- K5: merge a query's slices, explain the winners ------------------------------
__global__ __launch_bounds__(TPB_M) void k_merge_topk(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (p.q_fast && p.q_fast[blockIdx.x]) return;          // k_merge_flat's (bit 0) or k_score_small's (bit 1): their hits come from there
    merge_query<TPB_M, false>(p, blockIdx.x, smem, p.cb);
}
// the queries scored by k_score_wave: one candidate list per query
#ifndef SS_TPB_MF
#define SS_TPB_MF 320
#endif
constexpr int TPB_MF = SS_TPB_MF;   // 320: the 300 explain searches of a 3-term query at k = 100 are one pass (ms per batch at 256 / 320 / 384 / 512 threads: 0.405 / 0.399 / 0.410 / 0.420)
__global__ __launch_bounds__(TPB_MF) void k_merge_flat(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    merge_query<TPB_MF, false, true>(p, p.merge_q[blockIdx.x], smem, p.cb_flat);
}

size_t merge_lds_bytes(int k, int cb) { return (size_t)k * 32 + (size_t)cb * 12 + 8 + 16 + 16 + (size_t)MERGE_T * 20; }

// scoring layout: {doc, float32 upper bound of w/mag[doc]} per posting; flags: bit 0 = a weight is negative or not finite,
// bit 1 = a magnitude is not a positive finite number under a non-zero weight (the filter's assumptions, see k_score_slices)
__global__ void k_pack_recs(const uint32_t* __restrict__ doc, const float* __restrict__ w, const double* __restrict__ mag,
                            uint64_t n, Rec* __restrict__ out, uint32_t* __restrict__ flags) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t f = 0;
    for (; i < n; i += stride) {
        Rec r;
        r.doc = doc[i];
        const float wi = w[i];
        const double m = mag[r.doc];
        if (!(wi >= 0.0f) || isinf(wi)) f |= 1u;
        if (wi != 0.0f && (!(m > 0.0) || isinf(m))) f |= 2u;
        r.imp = impact_of(wi, m);
        out[i] = r;
    }
    if (__ballot(f != 0)) {
        for (int o = 32; o > 0; o >>= 1) f |= (uint32_t)__shfl_xor((int)f, o, 64);
        if ((threadIdx.x & 63) == 0) atomicOr(flags, f);
    }
}

// Combined lists for k_score_wave: the title and body postings of a term merged into ONE doc-sorted list (body before title
// on the same doc), field in bit 31 of the doc word.  c_ptr[t] = t_ptr[t] + b_ptr[t]; c_w[i] = the posting's float32 weight, copied
// from its table (the exact stage reads it by the record's position: one load, where an index into the table's own list cost a
// second, dependent one per survivor).  One thread per posting of one table: its place is its own
// index plus the number of the OTHER field's postings of the term that come before it.  A block finds the terms its
// postings span with two binary searches; each posting then finds its term inside that short range.
constexpr int CM_TPB = 256, CM_PT = 8, CM_CHUNK = CM_TPB * CM_PT;
__global__ __launch_bounds__(CM_TPB) void k_merge_lists(const uint64_t* __restrict__ my_ptr, const Rec* __restrict__ my_rec, uint64_t n_my,
                                                        const uint64_t* __restrict__ ot_ptr, const Rec* __restrict__ ot_rec, uint64_t n_terms,
                                                        int my_field, const float* __restrict__ my_w, Rec* __restrict__ c_rec, float* __restrict__ c_w) {
    __shared__ uint64_t s_t[2];
    const uint64_t base = (uint64_t)blockIdx.x * CM_CHUNK;
    if (base >= n_my) return;
    const uint64_t last = min(base + CM_CHUNK, n_my) - 1;
    if (threadIdx.x < 2) {
        const uint64_t target = threadIdx.x == 0 ? base : last;      // largest t with my_ptr[t] <= target
        uint64_t lo = 0, hi = n_terms;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (my_ptr[mid] <= target) lo = mid; else hi = mid;
        }
        s_t[threadIdx.x] = lo;
    }
    __syncthreads();
    const uint64_t t_lo = s_t[0], t_hi = s_t[1];
    for (int j = 0; j < CM_PT; j++) {
        const uint64_t i = base + (uint64_t)j * CM_TPB + threadIdx.x;
        if (i > last) break;
        uint64_t lo = t_lo, hi = t_hi + 1;                            // my_ptr[lo] <= i < my_ptr[hi]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (my_ptr[mid] <= i) lo = mid; else hi = mid;
        }
        const uint64_t t = lo;
        const Rec r = my_rec[i];
        // postings of the other field before this one: body (field 0) goes first on the same doc
        const uint64_t o0 = ot_ptr[t], o1 = ot_ptr[t + 1];
        const uint64_t before = lower_bound_rec(ot_rec, o0, o1, my_field == 0 ? r.doc : r.doc + 1u) - o0;
        const uint64_t pos = my_ptr[t] + o0 + (i - my_ptr[t]) + before;       // c_ptr[t] = my_ptr[t] + ot_ptr[t]
        Rec c = r;
        c.doc = r.doc | ((uint32_t)my_field << 31);
        // a title posting's impact is stored times 38/29 (rounded up twice): ONE filter coefficient per list then serves both
        // fields in k_score_wave's inner loop (get_metadata.go:69 weighs title 0.38, body 0.29) — still an upper bound
        if (my_field) {
            const float v = r.imp * 1.3103449f;                          // 1.3103449f > 38/29; then two ulps up: above the real product
            // (never past +Inf: the bit patterns behind it are NaNs, whose share fx_share counts as ONE unit — for a title impact
            //  beyond FLT_MAX / 1.31 the filter then dropped the very documents that win; +Inf saturates to FX_CLAMP and survives)
            c.imp = v > 0.0f ? __uint_as_float(min(__float_as_uint(v) + 2u, 0x7F800000u)) : v;
        }
        c_rec[pos] = c;
        c_w[pos] = my_w[i];
    }
}
// pad behind the combined records ({doc 0x7FFFFFFF body, impact 0}: in no window) and the skip index: c_skip[g] = doc of record 64*g
__global__ void k_combined_finish(Rec* __restrict__ c_rec, uint64_t n, uint32_t* __restrict__ c_skip) {
    const uint64_t n_pad = ((n + 63) & ~(uint64_t)63) + 64;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i >= n) { Rec r; r.doc = 0x7FFFFFFFu; r.imp = 0.0f; c_rec[i] = r; }
        if ((i & 63) == 0) c_skip[i >> 6] = c_rec[i].doc & 0x7FFFFFFFu;
    }
}
__global__ void k_add_ptr_u64(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// k'-th largest impact of every term's list for k' = 2^0 .. 2^10 (0 where the list is shorter), as LOWER bounds:
// a 4096-bin histogram over [2^-8, 1) (9 mantissa bits per binade: 0.2 % resolution; smaller impacts share bin 0,
// whose edge is 0), suffix-summed from the top; the bin edge at which the count reaches k' is the bound.
constexpr int KH_TPB = 256;
constexpr int KH_BINS = 4096;
constexpr uint32_t KH_B0 = 0x3B800000u;               // bits of 2^-8
__global__ __launch_bounds__(KH_TPB) void k_kth_impact(const uint64_t* __restrict__ term_ptr, const Rec* __restrict__ rec,
                                                        float* __restrict__ kth /*[T][KTH_N], zeroed*/) {
    __shared__ uint32_t s_hist[KH_BINS];
    __shared__ uint32_t s_part[KH_TPB];
    const uint64_t t = blockIdx.x;
    const uint64_t beg = term_ptr[t], end = term_ptr[t + 1];
    if (end == beg) return;
    for (int b = threadIdx.x; b < KH_BINS; b += KH_TPB) s_hist[b] = 0;
    __syncthreads();
    for (uint64_t i = beg + threadIdx.x; i < end; i += KH_TPB) {
        // stored impacts are rounded UP from w/mag: step down two float ulps for a lower bound
        const float lb = rec[i].imp * (1.0f - 0x1p-21f);
        const uint32_t xb = __float_as_uint(lb);
        uint32_t b = 0;
        if (lb > 0.0f && xb >= KH_B0) b = min((xb - KH_B0) >> 14, (uint32_t)(KH_BINS - 1));
        if (lb > 0.0f) atomicAdd(&s_hist[b], 1u);                    // NaN and non-positive impacts count for nothing
    }
    __syncthreads();
    // thread x owns bins [16x, 16x+16): its sum, then the number of postings in bins ABOVE its range
    constexpr int PER = KH_BINS / KH_TPB;
    uint32_t own = 0;
    for (int b = 0; b < PER; b++) own += s_hist[threadIdx.x * PER + b];
    s_part[threadIdx.x] = own;
    __syncthreads();
    uint32_t above = 0;
    for (int x = threadIdx.x + 1; x < KH_TPB; x++) above += s_part[x];
    uint32_t run = above;
    for (int b = PER - 1; b >= 0; b--) {
        const uint32_t bin = threadIdx.x * PER + b;
        const uint32_t c = s_hist[bin];
        if (c) {
            for (int j = 0; j < KTH_N; j++) {
                const uint32_t kk = 1u << j;
                if (run < kk && kk <= run + c) kth[t * KTH_N + j] = bin == 0 ? 0.0f : __uint_as_float(KH_B0 + (bin << 14));
            }
        }
        run += c;
    }
}

// rank [K][N] topic-major -> prior [N][K] node-major
__global__ void k_transpose_prior(const double* __restrict__ in, uint64_t n, int K, double* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (uint64_t)K) return;
    const uint64_t doc = i / K;
    const int t = (int)(i % K);
    out[i] = in[(uint64_t)t * n + doc];
}
// per-topic max / min of the prior (for the score upper bound), read from the topic-major input: one contiguous,
// coalesced row per topic (blockIdx.y); a wave reduces with DPP shuffles, one atomic pair per wave
__global__ void k_prior_extrema(const double* __restrict__ rank_topic_major, uint64_t n, unsigned long long* __restrict__ mx,
                                unsigned long long* __restrict__ mn) {
    const int t = blockIdx.y;
    const double* row = rank_topic_major + (uint64_t)t * n;
    double a = -INFINITY, b = INFINITY;
    bool nan = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double v = row[i];
        if (v != v) nan = true;
        a = fmax(a, v);
        b = fmin(b, v);
    }
    if (nan) { a = INFINITY; b = -INFINITY; }
    unsigned long long ka = fkey(a), kb = fkey(b);
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long oa = __shfl_xor(ka, m), ob = __shfl_xor(kb, m);
        ka = oa > ka ? oa : ka;
        kb = ob < kb ? ob : kb;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&mx[t], ka);
        atomicMin(&mn[t], kb);
    }
}

double unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

}  // namespace

namespace ss {
hipError_t launch_score_slices(const void* params, unsigned first, unsigned n, bool masked, int* lds_attr, int* lds_attr_masked, hipStream_t st) {
    ScoreParams p = *reinterpret_cast<const ScoreParams*>(params);
    const int cb = p.cb;
    const size_t lds_score = score_lds_bytes(cb);
    hipError_t e = hipSuccess;
    if (masked && *lds_attr_masked < cb) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_slices<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_score);
        if (e != hipSuccess) return e;
        *lds_attr_masked = cb;
    }
    if (*lds_attr < cb) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_slices<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_score);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_topk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)merge_lds_bytes(SS_MAX_TOPK, cb));
        if (e != hipSuccess) return e;
        *lds_attr = cb;
    }
    p.order += first;
    if (masked) hipLaunchKernelGGL(k_score_slices<true>, dim3(n), dim3(TPB), lds_score, st, p);
    else hipLaunchKernelGGL(k_score_slices<false>, dim3(n), dim3(TPB), lds_score, st, p);
    return hipSuccess;
}
void launch_phrase(const void* params, unsigned n_parts, unsigned n_q, hipStream_t st) {
    const ScoreParams& p = *reinterpret_cast<const ScoreParams*>(params);
    if (n_parts) hipLaunchKernelGGL(k_phrase_match, dim3(n_parts), dim3(PH_TPB), 0, st, p);
    hipLaunchKernelGGL(k_phrase_close, dim3(n_q), dim3(PH_TPB), 0, st, p);
}
void launch_merge_topk(const void* params, unsigned n_q, hipStream_t st) {
    const ScoreParams& p = *reinterpret_cast<const ScoreParams*>(params);
    hipLaunchKernelGGL(k_merge_topk, dim3(n_q), dim3(TPB_M), merge_lds_bytes(p.k, p.cb), st, p);
}
void launch_merge_flat(const void* params, unsigned n_merge, hipStream_t st) {
    const ScoreParams& p = *reinterpret_cast<const ScoreParams*>(params);
    hipLaunchKernelGGL(k_merge_flat, dim3(n_merge), dim3(TPB_MF), merge_lds_bytes(p.k, p.cb_flat), st, p);
}
}  // namespace ss

extern "C" {

int32_t ss_scorer_create(ss_ctx* ctx, ss_index* title, ss_index* body, ss_scorer** out) {
    if (!ctx) return SS_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out) return ctx->fail(SS_ERR_INVALID, "ss_scorer_create: out is NULL");
    *out = nullptr;
    if (!title || !body) return ctx->fail(SS_ERR_INVALID, "ss_scorer_create: NULL index");
    if (title->ctx != ctx || body->ctx != ctx) return ctx->fail(SS_ERR_INVALID, "ss_scorer_create: index from another context");
    if (title->n_docs != body->n_docs || title->n_terms != body->n_terms)
        return ctx->fail(SS_ERR_INVALID, "ss_scorer_create: title/body tables disagree on n_docs or n_terms");
    if (!title->weighted || !body->weighted)
        return ctx->fail(SS_ERR_STATE, "ss_scorer_create: run ss_tfidf_build (or ss_index_set_weighted) on both tables first");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<ss_scorer> s(new (std::nothrow) ss_scorer());
    if (!s) return ctx->fail(SS_ERR_OOM, "ss_scorer_create: host OOM");
    s->ctx = ctx;
    s->title = title;
    s->body = body;
    s->n_docs = title->n_docs;
    s->n_terms = title->n_terms;
    SS_HIP(ctx, s->t_rec.alloc(title->n_post));
    SS_HIP(ctx, s->b_rec.alloc(body->n_post));
    SS_HIP(ctx, s->t_kth.alloc((size_t)s->n_terms * KTH_N));
    SS_HIP(ctx, s->b_kth.alloc((size_t)s->n_terms * KTH_N));
    ss::DevBuf<uint32_t> flags;
    SS_HIP(ctx, flags.alloc(1));
    SS_HIP(ctx, hipMemsetAsync(flags.p, 0, sizeof(uint32_t), ctx->stream));
    SS_HIP(ctx, hipMemsetAsync(s->t_kth.p, 0, std::max<size_t>(s->t_kth.bytes(), 4), ctx->stream));
    SS_HIP(ctx, hipMemsetAsync(s->b_kth.p, 0, std::max<size_t>(s->b_kth.bytes(), 4), ctx->stream));
    if (title->n_post)
        hipLaunchKernelGGL(k_pack_recs, dim3(std::min<unsigned>(ss::div_up(title->n_post, 256), 16384u)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)title->post_doc.p, (const float*)title->post_w.p, (const double*)title->mag.p,
                           title->n_post, s->t_rec.p, flags.p);
    if (body->n_post)
        hipLaunchKernelGGL(k_pack_recs, dim3(std::min<unsigned>(ss::div_up(body->n_post, 256), 16384u)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)body->post_doc.p, (const float*)body->post_w.p, (const double*)body->mag.p,
                           body->n_post, s->b_rec.p, flags.p);
    {
        // combined lists: only while doc ids leave bit 31 free and the table stays below 2^32 postings (the wave kernel's limits)
        const uint64_t pc = title->n_post + body->n_post;
        if (s->n_docs < (1ull << 31) && pc < (1ull << 32) - 128 && s->n_terms && ctx->opt("score.wave", 1) != 0) {
            const uint64_t pc_pad = ((pc + 63) & ~(uint64_t)63) + 64;
            SS_HIP(ctx, s->c_rec.alloc(pc_pad));
            SS_HIP(ctx, s->c_w.alloc(pc_pad));
            SS_HIP(ctx, s->c_skip.alloc(pc_pad / 64 + 1));
            SS_HIP(ctx, s->c_ptr.alloc(s->n_terms + 1));
            hipLaunchKernelGGL(k_add_ptr_u64, dim3(ss::div_up(s->n_terms + 1, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)title->term_ptr.p,
                               (const uint64_t*)body->term_ptr.p, s->n_terms + 1, s->c_ptr.p);
            if (body->n_post)
                hipLaunchKernelGGL(k_merge_lists, dim3(ss::div_up(body->n_post, CM_CHUNK)), dim3(CM_TPB), 0, ctx->stream, (const uint64_t*)body->term_ptr.p,
                                   (const Rec*)s->b_rec.p, body->n_post, (const uint64_t*)title->term_ptr.p, (const Rec*)s->t_rec.p, s->n_terms, 0,
                                   (const float*)body->post_w.p, s->c_rec.p, s->c_w.p);
            if (title->n_post)
                hipLaunchKernelGGL(k_merge_lists, dim3(ss::div_up(title->n_post, CM_CHUNK)), dim3(CM_TPB), 0, ctx->stream, (const uint64_t*)title->term_ptr.p,
                                   (const Rec*)s->t_rec.p, title->n_post, (const uint64_t*)body->term_ptr.p, (const Rec*)s->b_rec.p, s->n_terms, 1,
                                   (const float*)title->post_w.p, s->c_rec.p, s->c_w.p);
            hipLaunchKernelGGL(k_combined_finish, dim3(std::min<unsigned>(ss::div_up(pc_pad, 256), 16384u)), dim3(256), 0, ctx->stream, s->c_rec.p, pc, s->c_skip.p);
            s->has_combined = true;
            s->c_pad_block = ((pc + 63) & ~(uint64_t)63) / 64;
        }
    }
    if (s->n_terms) {
        hipLaunchKernelGGL(k_kth_impact, dim3((unsigned)s->n_terms), dim3(KH_TPB), 0, ctx->stream, (const uint64_t*)title->term_ptr.p,
                           (const Rec*)s->t_rec.p, s->t_kth.p);
        hipLaunchKernelGGL(k_kth_impact, dim3((unsigned)s->n_terms), dim3(KH_TPB), 0, ctx->stream, (const uint64_t*)body->term_ptr.p,
                           (const Rec*)s->b_rec.p, s->b_kth.p);
    }
    SS_HIP(ctx, hipGetLastError());
    uint32_t h_flags = 0;
    SS_HIP(ctx, ss::fetch(ctx, ctx->stream, &h_flags, flags.p, sizeof(uint32_t)));
    s->clean = h_flags == 0;
    if (ctx->opt("score.exact_all", 0) != 0) s->clean = false;   // tests: force the filter off
    title->users++;
    body->users++;
    *out = s.release();
    return SS_OK;
}

int32_t ss_scorer_destroy(ss_scorer* s) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) (void)hipStreamSynchronize(ws);
#if defined(SSW_PHASES) && !defined(SS_DIAG)
    ss::score_wave_diag_dump();
#endif
    ss::score_small_report();               // (prints only in the -DSSS_PHASES build of score_small.hip)
#ifdef SS_DIAG
    ss::score_wave_diag_dump();
    {
        unsigned long long h[24];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag), sizeof(h)) == hipSuccess) {
            const char* names[19] = {"slices", "windows", "flushes", "flushed_records", "compactions", "records", "cyc_setup_lists", "cyc_setup_bounds", "cyc_flush", "cyc_setup", "cyc_windows", "cyc_total", "cyc_win_add", "cyc_win_barrier", "cyc_merge_explain", "cyc_merge_gather", "cyc_merge_final", "merges", "merge_candidates"};
            fprintf(stderr, "[ss diag] k_score_slices (thread 0 of every slice):");
            for (int i = 0; i < 19; i++) fprintf(stderr, " %s=%llu", names[i], h[i]);
            fprintf(stderr, "\n");
        }
        static unsigned long long hs[4096][4];
        if (hipMemcpyFromSymbol(hs, HIP_SYMBOL(g_slice), sizeof(hs)) == hipSuccess) {
            if (FILE* f = fopen("gpurun_out/ss_diag_slices.csv", "w")) {
                fprintf(f, "launch,start,end,windows,records\n");
                for (int i = 0; i < 4096; i++)
                    if (hs[i][1]) fprintf(f, "%d,%llu,%llu,%llu,%llu\n", i, hs[i][0], hs[i][1], hs[i][2], hs[i][3]);
                fclose(f);
            }
        }
    }
#endif
    s->title->users--;
    s->body->users--;
    delete s;
    return SS_OK;
}

int32_t ss_scorer_set_prior(ss_scorer* s, int32_t k_topics, const double* rank) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (k_topics < 0 || k_topics > SS_MAX_TOPICS) return ctx->fail(SS_ERR_INVALID, "ss_scorer_set_prior: bad k_topics");
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (every k_score_wave on the wave stream has a merge behind it on this one)
    if (k_topics == 0 || !rank) {
        s->prior.release();
        s->k_topics = 0;
        return SS_OK;
    }
    const uint64_t n = s->n_docs * (uint64_t)k_topics;
    ss::DevBuf<double> tmp;
    ss::DevBuf<unsigned long long> ext;
    SS_HIP(ctx, tmp.alloc(n));
    SS_HIP(ctx, ext.alloc(2 * (size_t)k_topics));
    SS_HIP(ctx, hipMemcpyAsync(tmp.p, rank, n * sizeof(double), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, s->prior.alloc(n));
    hipLaunchKernelGGL(k_transpose_prior, dim3(ss::div_up(n, 256)), dim3(256), 0, ctx->stream, (const double*)tmp.p, s->n_docs,
                       k_topics, s->prior.p);
    SS_HIP(ctx, hipMemsetAsync(ext.p, 0x00, k_topics * sizeof(unsigned long long), ctx->stream));                 // max keys
    SS_HIP(ctx, hipMemsetAsync(ext.p + k_topics, 0xFF, k_topics * sizeof(unsigned long long), ctx->stream));      // min keys
    hipLaunchKernelGGL(k_prior_extrema, dim3(std::min<unsigned>(ss::div_up(s->n_docs, 256), 1024u), k_topics), dim3(256), 0,
                       ctx->stream, (const double*)tmp.p, s->n_docs, ext.p, ext.p + k_topics);
    SS_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> h_ext(2 * (size_t)k_topics);
    SS_HIP(ctx, hipMemcpyAsync(h_ext.data(), ext.p, h_ext.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->prior_max.resize(k_topics);
    s->prior_min.resize(k_topics);
    for (int t = 0; t < k_topics; t++) {
        s->prior_max[t] = unkey(h_ext[t]);
        s->prior_min[t] = unkey(h_ext[k_topics + t]);
    }
    s->k_topics = k_topics;
    s->prior_clean = true;
    for (int t = 0; t < k_topics; t++)          // a NaN anywhere shows as max = +inf, min = -inf (k_prior_extrema)
        if (!(s->prior_min[t] >= 0.0) || !std::isfinite(s->prior_max[t])) s->prior_clean = false;
    return SS_OK;
}

int32_t ss_scorer_set_doc_masks(ss_scorer* s, int32_t n_masks, const uint32_t* words) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (n_masks < 0 || (n_masks > 0 && !words)) return ctx->fail(SS_ERR_INVALID, "ss_scorer_set_doc_masks: n_masks < 0 or words is NULL");
    // the scorer's outstanding batches (pipelined calls, tickets) read the old set: their kernels are on the context's stream or
    // a wave stream, every one of which is drained before the set is replaced
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    const uint64_t n_words = (s->n_docs + 31) / 32;
    if (n_masks == 0 || n_words == 0) {
        s->masks.release();
        s->n_masks = n_masks;                   // (n_docs = 0: ids 0 .. n_masks-1 stay valid, there is no doc to allow)
        s->mask_words = n_words;
        return SS_OK;
    }
    ss::DevBuf<uint32_t> nb;
    SS_HIP(ctx, nb.alloc((size_t)n_masks * n_words));
    SS_HIP(ctx, hipMemcpyAsync(nb.p, words, (size_t)n_masks * n_words * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->masks = std::move(nb);
    s->n_masks = n_masks;
    s->mask_words = n_words;
    return SS_OK;
}

}  // extern "C"
