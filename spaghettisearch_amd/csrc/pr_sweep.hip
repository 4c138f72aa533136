// pr_sweep.hip — k_pr_sweep<8|16, TS, LEAN>: the wave-item sweep of the padded lane-group widths, the product path for K >= 3 and the
// benchmark's headline kernel.  Exports ss::pr_sweep_launch and ss::pr_sweep_occupancy (and, in the SS_PR_WAVETIME
// variant build, ss::pr_dump_wave_times).
#include "pr_device.hpp"

#include <algorithm>

namespace {

// ---- gather ------------------------------------------------------------------
// T[row][t] addressed as table base (wave-uniform, scalar registers) + 32-bit byte offset: the contribution table of a rank
// stays below 4 GiB (n_nd * GW * 8 bytes, checked in ss_pr_create), so no 64-bit vector address arithmetic is needed
template <int GW>
__device__ __forceinline__ double tab_at(const double* __restrict__ T, uint32_t row, int t) {
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(T) + (size_t)((row * (uint32_t)GW + (uint32_t)t) * 8u));
}

// ---- the sweep, K >= 3 (GW = 8 / 16): k_pr_sweep -------------------------------------------------------------
// Every work item belongs to ONE wave (no block barriers on the way), control flow is wave-uniform, and every path
// is the same software pipeline: a lane group (GW lanes = the GW topic values of one table row) takes 16 in-edges
// per turn; the index words of turn i+1 are requested before the 16 whole-row gathers of turn i are issued, so a turn
// costs ONE memory latency.  Slots of a turn that hold no edge gather the table's all-zero row (p.zrow) and add an
// exact 0.0 — there are no per-edge predicates, flags or LDS traffic anywhere.  Row ends are known from the item:
//   V_SEG / V_ROWW   the wave's lane groups share one long row (cross-group butterfly at the end)
//   V_QUAD           one row per lane group, all rows of the item `nch` turns long (rows are in-degree sorted)
//   V_DEG<R>         R rows of exactly D <= 16/R in-edges per lane group and turn, at fixed slots
// Measured on the 10M/50M R-MAT, K=16 (MI355X): 1.41 ms per sweep for the block-per-item / flag-driven kernel this
// replaces; every class alone was latency-bound (0.60 + 0.53 + 0.57 + 0.16 ms).

// TS: the state holds teleport sets (ss_pr_set_teleport).  A kernel of its own, so that the reference's path carries no
// membership loads (a load under a branch in finish_row makes the compiler drain the loads in flight: s_waitcnt vmcnt(0)).
// LEAN: a sweep of a fixed-iteration run whose ranks and L1 change no caller can see (ss::pr_step decides which; TS = false only).
// It produces what the next sweep reads — the table, the contribution sum, the hub rows' contribution slots, the shared rows,
// the control block — from the same expressions in the same order, and nothing else: no old-rank load, no rank store, no L1
// arithmetic, and the waves walk p.woff_lean, which holds no item of a dangling row (such a row has no table row: its sum feeds
// only its rank).  The rank array and the published L1 change are stale behind it; the host runs the last two sweeps in front of
// anything a caller can read full.  A parameter and not a branch for the same reason as TS.
template <int GW, bool TS, bool LEAN>
struct SweepCtx {
    const PrParams& p;
    const double* __restrict__ T;
    double* __restrict__ Tw;
    double S, x0;
    bool act;
    int t, gbase, slot;
    double dsum, csum;
};

// edges of [epos, lim) that fall into a 16-slot turn starting at epos: saturating, so that a turn past the end has none
__device__ __forceinline__ uint32_t turn_fill(uint32_t epos, uint32_t lim) {
    return min((uint32_t)CH, __builtin_elementwise_sub_sat(lim, epos));
}

// the 16 index words of a lane group's turn: slot j = r*GW + t holds edge `epos + j` for j < n, the zero row otherwise
template <int GW>
__device__ __forceinline__ void idx_turn(const uint32_t* __restrict__ in_src, uint32_t epos, uint32_t n, uint32_t zrow, int t, uint32_t (&src)[CH / GW]) {
#pragma unroll
    for (int r = 0; r < CH / GW; r++) {
        const uint32_t j = (uint32_t)(r * GW + t);
        const uint32_t raw = NT_LOAD(&in_src[j < n ? epos + j : 0u]);       // unconditional load (edge 0 exists whenever an item has edges)
        src[r] = j < n ? (raw & SRC_MASK) : zrow;
    }
}
template <int GW>
__device__ __forceinline__ void gather_turn(const double* __restrict__ T, const uint32_t (&src)[CH / GW], int t, int gbase, double (&v)[CH]) {
#pragma unroll
    for (int j = 0; j < CH; j++) {
        const uint32_t sj = (uint32_t)__shfl((int)src[j / GW], gbase + (j % GW), 64);
        v[j] = tab_at<GW>(T, sj, t);
    }
}

// hub: the row was cut into pieces and is finished by whichever wave handed its piece in last, a different one from run to run — its
// two terms go to the row's own slot (PrParams::hubsum, added in row order by block_reduce_and_publish), not into this wave's sums,
// whose order of addition must not depend on who arrives when
template <int GW, bool TS, bool LEAN>
__device__ __forceinline__ void finish_row(SweepCtx<GW, TS, LEAN>& c, uint32_t lrow, double y, double xo, uint32_t od, double* hub = nullptr) {
    const PrParams& p = c.p;
    y += c.x0;
    const size_t xi = (size_t)lrow * GW + c.t;
    double tele = p.teleport;
    if constexpr (TS) tele = teleport_of(p, lrow, c.t);
    double xn = (y + tele) / c.S;                             // pagerank.go:117
    if constexpr (LEAN) {
        // every row of a lean walk is non-dangling, and a topic that is not active is one of the padding topics (a fixed-iteration
        // run freezes none): its ranks are the 0.0 they were set to, which the full sweep reads back as xo
        if (!c.act) xn = 0.0;
        const double cc = p.d * xn / (double)od;              // pagerank.go:136
        NT_STORE(cc, &c.Tw[xi]);
        if (hub) __hip_atomic_store(&hub[GW + c.t], cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else c.csum += cc;                                    // pagerank.go:137
        return;
    }
    if (c.act) {
        NT_STORE(xn, &p.x[xi]);
        if (!hub) c.dsum += fabs(xn - xo);                    // pagerank.go:118
    } else {
        xn = xo;                                              // converged topic: frozen
    }
    double cc = 0.0;
    if (lrow < p.sl_nd) {                                     // non-dangling row: next sweep's contribution
        cc = p.d * xn / (double)od;                           // pagerank.go:136
        NT_STORE(cc, &c.Tw[xi]);
        if (!hub) c.csum += cc;                               // pagerank.go:137
    }
    if (hub) {
        __hip_atomic_store(&hub[c.t], fabs(xn - xo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&hub[GW + c.t], cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// V_SEG / V_ROWW: the wave's items are long rows (or <= SEGW-edge pieces of the longest ones); turn i of an item
// gives lane group s the edges beg + 64*i + 16*s ...  The pipeline runs across the items: the last turn of one item
// requests the first index words of the next.
template <int GW, bool TS, bool LEAN>
__device__ __forceinline__ void long_rows(SweepCtx<GW, TS, LEAN>& c, const WorkItem* __restrict__ work, uint32_t i0, uint32_t i1, int lane) {
    constexpr int NS = 64 / GW;
    constexpr uint32_t TW = NS * CH;                          // edges per wave turn
    const PrParams& p = c.p;
    if (i0 >= i1) return;
    WorkItem cur = work[i0], nxt = work[i0 + 1];              // the table ends with two unused items: reading ahead is safe
    uint32_t src_n[CH / GW];
    {
        const uint32_t e0 = cur.beg + (uint32_t)c.slot * CH;
        idx_turn<GW>(p.in_src, e0, turn_fill(e0, cur.end), p.zrow, c.t, src_n);
    }
    for (uint32_t it = i0; it < i1; it++) {
        const WorkItem nn = work[it + 2];
        const uint32_t lrow = cur.row;
        // the row's old rank and out-degree: asked for now, used after the last turn
        double xo = 0.0;
        if constexpr (!LEAN) xo = NT_LOAD(&p.x[(size_t)lrow * GW + c.t]);
        const uint32_t od = lrow < p.sl_nd ? NT_LOAD(&p.outdeg[lrow]) : 1u;
        const uint32_t turns = (cur.end - cur.beg + TW - 1) / TW;
        const bool more = it + 1 < i1;
        double acc = 0.0;
        for (uint32_t i = 0; i < turns; i++) {
            uint32_t src[CH / GW];
#pragma unroll
            for (int r = 0; r < CH / GW; r++) src[r] = src_n[r];
            const bool last = i + 1 == turns;                 // scalar
            const uint32_t e1 = (last ? nxt.beg : cur.beg + (i + 1) * TW) + (uint32_t)c.slot * CH;
            const uint32_t lim = last ? (more ? nxt.end : 0u) : cur.end;
            idx_turn<GW>(p.in_src, e1, turn_fill(e1, lim), p.zrow, c.t, src_n);
            double v[CH];
            gather_turn<GW>(c.T, src, c.t, c.gbase, v);
#pragma unroll
            for (int j = 0; j < CH; j++) acc += v[j];
        }
        const double y = wave_sum_topic<GW>(acc);
        if (cur.kind == V_ROWW) {
            if (lane < GW) finish_row<GW>(c, lrow, y, xo, od);
        } else {
            // several waves (of any blocks) share this row: publish the piece's sum; the last to arrive adds the
            // pieces in order and finishes the row
            // (write-through stores, drained, then the ticket; the last arriver reads with sc1 loads: no fences — see
            // block_reduce_and_publish)
            if (lane < GW) __hip_atomic_store(&p.segpart[(size_t)(cur.sbase + cur.count) * GW + c.t], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned prev = 0;
            if (lane == 0) prev = __hip_atomic_fetch_add(&p.rowticket[cur.tix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = (unsigned)__builtin_amdgcn_readfirstlane((int)prev);
            if (prev == cur.nseg - 1) {
                if (lane == 0) __hip_atomic_store(&p.rowticket[cur.tix], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane < GW) {
                    double ys = 0.0;
                    for (uint32_t q = 0; q < cur.nseg; q++)
                        ys += __hip_atomic_load(&p.segpart[(size_t)(cur.sbase + q) * GW + c.t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    finish_row<GW>(c, lrow, ys, xo, od, p.hubsum + (size_t)cur.tix * 2 * GW);
                }
            }
        }
        cur = nxt;
        nxt = nn;
    }
}

// V_QUAD: an item = rows row .. row+count-1, lane group s takes rows row + q*NS + s (q = 0 .. nq-1, nq <= GW), every row
// is walked in nch (= item.nseg) turns (its own length decides how many slots of a turn are real).  The bounds and
// out-degrees of ALL rows of an item come in one request (lane t of group s holds row `row + t*NS + s`), one item ahead;
// the pipeline runs across row groups and items.
template <int GW, bool TS, bool LEAN>
__device__ __forceinline__ void quad_rows(SweepCtx<GW, TS, LEAN>& c, const WorkItem* __restrict__ work, uint32_t i0, uint32_t i1) {
    constexpr int NS = 64 / GW;
    const PrParams& p = c.p;
    if (i0 >= i1) return;
    const uint32_t myq = (uint32_t)c.t * NS + (uint32_t)c.slot;
    auto bounds = [&](const WorkItem& w, bool live, uint32_t& bv, uint32_t& ev, uint32_t& ov) __attribute__((always_inline)) {
        const bool have = live && myq < w.count;
        const uint32_t rq = live ? w.row + (have ? myq : 0u) : 0u;
        const uint32_t b = p.in_ptr[rq], e = p.in_ptr[rq + 1];
        bv = b;
        ev = have ? e : b;
        ov = rq < p.sl_nd ? NT_LOAD(&p.outdeg[rq]) : 1u;
    };
    WorkItem cur = work[i0], nxt = work[i0 + 1];
    uint32_t cb, ce, co, nb, ne, no;
    bounds(cur, true, cb, ce, co);
    bounds(nxt, i0 + 1 < i1, nb, ne, no);
    uint32_t it = i0, q = 0, ch = 0;                          // scalar: item, row group and turn inside it
    uint32_t nq = (cur.count + NS - 1) / NS, nch = cur.nseg;
    uint32_t src_n[CH / GW];
    {
        const uint32_t b0 = (uint32_t)__shfl((int)cb, c.gbase, 64), e0 = (uint32_t)__shfl((int)ce, c.gbase, 64);
        idx_turn<GW>(p.in_src, b0, turn_fill(b0, e0), p.zrow, c.t, src_n);
    }
    double acc = 0.0;
    while (it < i1) {
        uint32_t src[CH / GW];
#pragma unroll
        for (int r = 0; r < CH / GW; r++) src[r] = src_n[r];
        // the turn after this one: same row group, the next one, or the first of the next item
        uint32_t qn = q, cn = ch + 1;
        bool cross = false;
        if (cn == nch) {
            cn = 0;
            qn = q + 1;
            if (qn == nq) { qn = 0; cross = true; }
        }
        const bool live_n = !cross || it + 1 < i1;
        {
            const uint32_t b_n = (uint32_t)__shfl((int)(cross ? nb : cb), c.gbase + (int)qn, 64);
            const uint32_t e_n = (uint32_t)__shfl((int)(cross ? ne : ce), c.gbase + (int)qn, 64);
            const uint32_t ep = b_n + cn * CH;
            idx_turn<GW>(p.in_src, ep, live_n ? turn_fill(ep, e_n) : 0u, p.zrow, c.t, src_n);
        }
        const bool ends = ch + 1 == nch;                      // scalar: this turn completes the rows of group q
        const uint32_t lrow = cur.row + q * NS + (uint32_t)c.slot;
        const bool valid = q * NS + (uint32_t)c.slot < cur.count;
        double xo = 0.0;
        if constexpr (!LEAN)
            if (ends) xo = NT_LOAD(&p.x[(size_t)(valid ? lrow : cur.row) * GW + c.t]);
        double v[CH];
        gather_turn<GW>(c.T, src, c.t, c.gbase, v);
#pragma unroll
        for (int j = 0; j < CH; j++) acc += v[j];
        if (ends) {
            const uint32_t od = (uint32_t)__shfl((int)co, c.gbase + (int)q, 64);
            if (valid) finish_row<GW>(c, lrow, acc, xo, od);
            acc = 0.0;
        }
        q = qn;
        ch = cn;
        if (cross) {
            it++;
            cur = nxt;
            cb = nb; ce = ne; co = no;
            nq = (cur.count + NS - 1) / NS;
            nch = cur.nseg;
            nxt = work[it + 1];
            bounds(nxt, it + 1 < i1, nb, ne, no);
        }
    }
}

// V_DEG: an item = `count` rows of exactly D (= item.nseg) in-edges from `row` (their edges are contiguous from item.beg);
// a lane group takes R rows per turn, row r of the turn at slots r*DM .. r*DM+D-1 (DM = 16/R >= D)
template <int GW, int R, bool TS, bool LEAN>
__device__ __forceinline__ void deg_rows(SweepCtx<GW, TS, LEAN>& c, const WorkItem* __restrict__ work, uint32_t i0, uint32_t i1) {
    constexpr int NS = 64 / GW;
    constexpr int DM = CH / R;
    constexpr int IR = CH / GW;
    const PrParams& p = c.p;
    if (i0 >= i1) return;
    auto idx = [&](const WorkItem& w, bool live, uint32_t turn, uint32_t (&src)[IR]) __attribute__((always_inline)) {
        const uint32_t rb = (turn * NS + (uint32_t)c.slot) * R;           // first row (relative) of this lane group's turn
#pragma unroll
        for (int r = 0; r < IR; r++) {
            const uint32_t j = (uint32_t)(r * GW + c.t);
            const uint32_t rr = rb + j / DM, u = j % DM;
            const bool ok = live && u < w.nseg && rr < w.count;
            const uint32_t raw = NT_LOAD(&p.in_src[ok ? w.beg + rr * w.nseg + u : 0u]);
            src[r] = ok ? (raw & SRC_MASK) : p.zrow;
        }
    };
    WorkItem cur = work[i0], nxt = work[i0 + 1];
    uint32_t src_n[IR];
    idx(cur, true, 0, src_n);
    for (uint32_t it = i0; it < i1; it++) {
        const WorkItem nn = work[it + 2];
        const uint32_t row0 = cur.row, count = cur.count;
        const uint32_t turns = (count + NS * R - 1) / (NS * R);
        for (uint32_t i = 0; i < turns; i++) {
            uint32_t src[IR];
#pragma unroll
            for (int r = 0; r < IR; r++) src[r] = src_n[r];
            if (i + 1 < turns) idx(cur, true, i + 1, src_n);
            else idx(nxt, it + 1 < i1, 0, src_n);
            const uint32_t rb = (i * NS + (uint32_t)c.slot) * R;
            // old ranks and out-degrees of the R rows travel with the gathers
            double xo[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                xo[r] = 0.0;
                if constexpr (!LEAN) xo[r] = NT_LOAD(&p.x[(size_t)(row0 + (rb + r < count ? rb + r : 0u)) * GW + c.t]);
            }
            const uint32_t myr = row0 + (rb + (uint32_t)c.t < count ? rb + (uint32_t)c.t : 0u);
            const uint32_t odv = (c.t < R && myr < p.sl_nd) ? NT_LOAD(&p.outdeg[myr]) : 1u;
            double v[CH];
            gather_turn<GW>(c.T, src, c.t, c.gbase, v);
#pragma unroll
            for (int r = 0; r < R; r++) {
                double y = 0.0;
#pragma unroll
                for (int u = 0; u < DM; u++) y += v[r * DM + u];
                const uint32_t od = (uint32_t)__shfl((int)odv, c.gbase + r, 64);
                if (rb + r < count) finish_row<GW>(c, row0 + rb + r, y, xo[r], od);
            }
        }
        cur = nxt;
        nxt = nn;
    }
}

#ifndef SS_PR_MINW
#define SS_PR_MINW 1
#endif
#ifdef SS_PR_WAVETIME
// variant build (tools/build_variant.sh wt -DSS_PR_WAVETIME): when every wave of the last sweep started and ran out of items
// (100 MHz realtime counter), printed by ss_pr_destroy — how level the deal is in TIME, not in modelled turns
__device__ unsigned long long g_pr_wt[65536][2];
#endif
template <int GW, bool TS, bool LEAN>
__global__ __launch_bounds__(TPB, SS_PR_MINW) void k_pr_sweep(PrParams p) {
    static_assert(!(TS && LEAN), "the lean sweep exists without teleport sets only");
    constexpr int NS = 64 / GW;
    PrCtl* ctl = p.ctl;
    if (ctl->n_active == 0) return;   // every topic converged: the launch is a no-op
#ifdef SS_PR_WAVETIME
    unsigned long long wt0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wt0));
#endif
    const int sweep = ctl->sweep;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    SweepCtx<GW, TS, LEAN> c{p, p.tab_rd[sweep & 1], p.tab_wr[sweep & 1], 0.0, 0.0, false, lane % GW, lane - lane % GW, lane / GW, 0.0, 0.0};
    c.S = ctl->S[c.t];
    c.act = ctl->active[c.t] != 0;
    c.x0 = sweep == 0 ? p.x0[c.t] : 0.0;      // Q4: iteration 1 accumulates onto 1/n

    // The shared rows of the next sweep's table (p.share): what V_ZERO would store for a row of that out-degree, once per degree.
    // Written by the grid's first threads in front of their items and added to nothing, so no partial sum changes its order.
    if constexpr (!TS) {
        if (p.n_shared) {
            const double xz_out = c.act ? zero_row_rank(p, sweep, c.S, p.x0[c.t]) : ctl->xz[c.t];
            const uint32_t nel = p.n_shared * (uint32_t)GW;        // (element i belongs to topic i % GW = c.t: TPB is a multiple of GW)
            for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < nel; i += gridDim.x * TPB)
                c.Tw[(size_t)(p.zrow + 1) * GW + i] = p.d * xz_out / (double)p.sh_deg[i / GW];   // pagerank.go:136
        }
    }

    // This wave's items: work[off[k] .. off[k+1]) for class k.  The host dealt the items to the waves so that every wave
    // gets the same number of turns (ss_pr_create); one loop per class, so that the register allocator sees each
    // pipeline on its own instead of the union of all of them.
    const uint32_t* __restrict__ off = (LEAN ? p.woff_lean : p.woff) + (size_t)(blockIdx.x * WAVES + wave) * 8;
    // The ORDER in which a wave walks its classes matters more than anything tried on the deal (round 5: all 720 orders, 4 blocks per
    // CU, config 4): short rows first, long rows last — 2, 3, 5, 4, 0, 1 = rows of <= 2 in-edges, <= 4, edge-less, <= 8, long, mid —
    // 0.902-0.904 ms per sweep against 0.947 in the order the classes are numbered (worst order 0.961).  Round 4's "stagger" (the
    // resident blocks of a CU start at different positions of the order: option "pr.stagger", now off by default) had found a part
    // of this by accident — its best start vectors were the ones that began most blocks at the short rows —; on top of the best
    // orders no start vector gains anything (every vector of 1296 measured for the best four orders: the all-equal one wins).
    // The loop below walks the order; "pr.class_order" = six digits, "pr.stagger" as before.
    int rot = p.stagger_div ? (int)((blockIdx.x / p.stagger_div) % 6u) : 0;
    if (p.stagger_code) {                       // experiments ("pr.stagger" >= 10): round r starts at base-6 digit r of the code
        uint32_t cdv = p.stagger_code;
        for (uint32_t r = blockIdx.x / p.stagger_div; r > 0; r--) cdv /= 6u;
        rot = (int)(cdv % 6u);
    }
    for (int s6 = 0; s6 < 6; s6++) {
    const int cls = (int)((p.class_order >> (3 * ((s6 + rot) % 6))) & 7u);
    {
        // everything a class pipeline derives from the lane id is recomputed behind an opaque copy per round: hoisted out of this loop,
        // the per-lane invariants of all six pipelines were live at once (164 VGPRs = 3 waves per SIMD instead of 114 = 4)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        c.t = ln % GW;
        c.gbase = ln - ln % GW;
        c.slot = ln / GW;
    }
    switch (cls) {
    case 0: long_rows<GW>(c, p.work, off[0], off[1], lane); break;
    case 1: quad_rows<GW>(c, p.work, off[1], off[2]); break;
    case 2: deg_rows<GW, 2>(c, p.work, off[2], off[3]); break;
    case 3: deg_rows<GW, 4>(c, p.work, off[3], off[4]); break;
    case 4: deg_rows<GW, 8>(c, p.work, off[4], off[5]); break;
    default:
    for (uint32_t item = off[5]; item < off[6]; item++) {
        const WorkItem w = p.work[item];
        // V_ZERO: non-dangling rows without in-edges: their rank is the shared value xz, only the next contribution
        // d*xz/outdeg has to be written (dangling ones need nothing at all); 16 rows per lane group and item at most
        // (p.share: the table has no such rows — the contributions are only added up, in the same order)
        const bool store = TS || !p.share;
        const bool ts = TS && p.memb && ((p.ts_mask >> c.t) & 1u);
        const double xz_out = c.act ? (ts ? zero_row_rank_ts(p, sweep, c.S, p.x0[c.t], 0.0) : zero_row_rank(p, sweep, c.S, p.x0[c.t])) : ctl->xz[c.t];
        const double xz_inn = ts ? (c.act ? zero_row_rank_ts(p, sweep, c.S, p.x0[c.t], p.tin[c.t]) : ctl->xz_in[c.t]) : xz_out;
        uint32_t od[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t rr = (uint32_t)(i * NS + c.slot);
            od[i] = NT_LOAD(&p.outdeg[w.row + (rr < w.count ? rr : 0u)]);
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t rr = (uint32_t)(i * NS + c.slot);
            if (rr < w.count) {
                const uint32_t lrow = w.row + rr;
                const double xz = ts && ((p.memb[lrow] >> c.t) & 1u) ? xz_inn : xz_out;
                const double cc = p.d * xz / (double)od[i];                      // pagerank.go:136
                if (store) NT_STORE(cc, &c.Tw[(size_t)lrow * GW + c.t]);
                c.csum += cc;                                                     // pagerank.go:137
            }
        }
    }
    break;
    }
    }
#ifdef SS_PR_WAVETIME
    {
        unsigned long long wt1;
        asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wt1));
        const uint32_t wid = (blockIdx.x * WAVES + wave) & 65535u;
        if (lane == 0) { g_pr_wt[wid][0] = wt0; g_pr_wt[wid][1] = wt1; }
    }
#endif
    // (lean: the published L1 change is not one — no row adds to it, the cut rows' slots keep an older sweep's terms)
    block_reduce_and_publish<GW>(p, LEAN ? 0.0 : c.dsum, c.csum, c.Tw, false);
}

template __device__ void begin_caller_context<8, 16>(const PrParams&, double*);   // pr_device.hpp: keeps the helpers' code the parent file's

}  // namespace

namespace ss {
void pr_sweep_launch(ss_pr* pr, hipStream_t st, bool lean) {
    const bool ts = pr->prm.memb != nullptr;
    lean = lean && !ts && pr->prm.woff_lean;
    if (lean) pr->n_lean++;
    if (pr->gw == 8) {
        if (ts) hipLaunchKernelGGL((k_pr_sweep<8, true, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else if (lean) hipLaunchKernelGGL((k_pr_sweep<8, false, true>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else hipLaunchKernelGGL((k_pr_sweep<8, false, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
    } else {
        if (ts) hipLaunchKernelGGL((k_pr_sweep<16, true, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else if (lean) hipLaunchKernelGGL((k_pr_sweep<16, false, true>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else hipLaunchKernelGGL((k_pr_sweep<16, false, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
    }
}
int pr_sweep_occupancy(int gw) {
    int per_cu = 8;
    if (gw == 8) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_sweep<8, false, false>, TPB, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_sweep<16, false, false>, TPB, 0);
    return per_cu;
}

#ifdef SS_PR_WAVETIME
// variant build: when every wave of the last sweep started and ran out of items (k_pr_sweep's timestamps; called by ss_pr_destroy)
void pr_dump_wave_times(const ss_pr* pr) {
    if (pr->gw < 8) return;
    (void)hipDeviceSynchronize();
    const uint32_t nwv = std::min<uint32_t>(65536u, pr->nblocks * WAVES);
    std::vector<unsigned long long> h((size_t)nwv * 2);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_pr_wt), h.size() * sizeof(unsigned long long)) != hipSuccess || !nwv) return;
    unsigned long long t0 = ~0ull;
    for (uint32_t w = 0; w < nwv; w++) t0 = std::min(t0, h[2 * w]);
    std::vector<double> st(nwv), en(nwv);
    for (uint32_t w = 0; w < nwv; w++) { st[w] = (double)(h[2 * w] - t0) / 100.0; en[w] = (double)(h[2 * w + 1] - t0) / 100.0; }
    std::sort(st.begin(), st.end()); std::sort(en.begin(), en.end());
    if (FILE* f = open_dump("pr_wt.csv")) {
        fprintf(f, "wave,start_us,end_us\n");
        for (uint32_t w = 0; w < nwv; w++) fprintf(f, "%u,%.2f,%.2f\n", w, (double)(h[2 * w] - t0) / 100.0, (double)(h[2 * w + 1] - t0) / 100.0);
        fclose(f);
    }
    fprintf(stderr, "[pr wavetime] %u waves: start us median %.1f max %.1f | out of items us min %.1f p10 %.1f median %.1f p90 %.1f p99 %.1f max %.1f\n", nwv,
            st[nwv / 2], st[nwv - 1], en[0], en[nwv / 10], en[nwv / 2], en[nwv * 9 / 10], en[(size_t)nwv * 99 / 100], en[nwv - 1]);
}
#endif
}  // namespace ss
