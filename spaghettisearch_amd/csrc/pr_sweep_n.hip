// pr_sweep_n.hip — k_pr_sweep_n<1|2, TS>: the wave-item sweep for K <= 2, the product path there, and k_pr_multi_n<1|2, 1|2>, the
// same sweep with ss_pr_step's sweeps inside one launch (opt-in, measured slower: DESIGN.md K1c).  Exports ss::pr_sweep_n_launch,
// ss::pr_multi_n_launch and their occupancy queries.
#include "pr_device.hpp"

namespace {

// ---- the sweep for K <= 2, wave-owned items (round 4) ------------------------------------------------------------------------
// k_pr_sweep's lane group holds the GW topic values of ONE table row; with one or two topics that geometry either pads to eight
// (seven of eight lanes gather, add and DIVIDE for padding: config 2 was issue-bound at 7.6 % of the roofline) or shrinks the
// group to one or two lanes (nothing coalesces).  Here the lanes hold ROWS and EDGES instead: the table row is one double
// (K = 1) or one double2 (K = 2), a lane gathers it whole, and
//   V_DEG    rows of exactly D <= 8 in-edges (almost all rows of a power-law graph): one LANE per row — D index words, D gathers,
//            and every lane finishes a row of its own (the two float64 divisions of pagerank.go:117,136 run on 64 real rows);
//   V_QUAD   9 .. 256 in-edges: one row per 8-lane group, the lanes stride the row's edges, three-step butterfly at its end;
//   V_ROWW / V_SEG   long rows and 2048-edge pieces of the longest: the wave strides the edges, six-step butterfly;
//   V_ZERO   one lane per row.
// The items, their classes and the static deal to the waves are those of the 8-wide sweep (cut_items with 8-lane groups).  Nothing is
// software-pipelined: a lane holds a handful of registers, so eight waves per SIMD hide the latency instead.
// Summation order: a row's in-edges are added in a fixed order that depends only on the row's class — deterministic, and
// within the last bits of the other kernels' orders (parity gate 1e-6; iteration counts as the oracle's).
#ifndef SS_PRN_MINW
#define SS_PRN_MINW 6
#endif
template <int KW>
struct NVec { double v[KW]; };
// PS (k_pr_multi_n: several sweeps inside one launch): the table row was written by another CU earlier in this launch, so it is read
// with L1-bypassing sc1 loads (and stored write-through, tab_store below) instead of relying on a kernel boundary
template <int KW, int PS = 0>
__device__ __forceinline__ NVec<KW> ntab(const double* __restrict__ T, uint32_t row) {
    NVec<KW> r;
    if constexpr (PS == 1) {
        const double* q = reinterpret_cast<const double*>(reinterpret_cast<const char*>(T) + (size_t)(row * (8u * KW)));
#pragma unroll
        for (int k = 0; k < KW; k++) r.v[k] = __hip_atomic_load(q + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if constexpr (KW == 1) {
        r.v[0] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(T) + (size_t)(row * 8u));
    } else {
        const double2 t = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(T) + (size_t)(row * 16u));
        r.v[0] = t.x;
        r.v[1] = t.y;
    }
    return r;
}
template <int PS>
__device__ __forceinline__ void tab_store(double v, double* q) {
    if constexpr (PS == 1) __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else NT_STORE(v, q);
}
template <int KW, bool TS>
struct NCtx {
    const PrParams& p;
    const double* __restrict__ T;
    double* __restrict__ Tw;
    double S[KW], x0[KW], dsum[KW], csum[KW], tele[KW];
    bool act[KW];
    const double* __restrict__ xr;      // ranks before this sweep
    double* __restrict__ xw;            // ... and after it (the same array, except in the two-vector form: PrParams::x_alt)
};
// XS: also the row's RANK is stored write-through — the rows that are cut into pieces (V_SEG) are finished by whichever wave hands its
// piece in last, a different wave (and CU) from sweep to sweep, so inside k_pr_multi_n their ranks are handed from CU to CU like the table
// hub: a row cut into pieces, finished by whichever wave arrives last — its terms go to the row's own slot (PrParams::hubsum), not
// into this lane's sums (see k_pr_sweep's finish_row)
template <int KW, bool TS, int PS = 0, bool XS = false>
__device__ __forceinline__ void finish_n(NCtx<KW, TS>& c, uint32_t lrow, const NVec<KW>& y, const NVec<KW>& xo, uint32_t od, double* hub = nullptr) {
    const PrParams& p = c.p;
#pragma unroll
    for (int k = 0; k < KW; k++) {
        const double yk = y.v[k] + c.x0[k];
        double tele = c.tele[k];
        if constexpr (TS) tele = teleport_of(p, lrow, k);
        double xn = (yk + tele) / c.S[k];                         // pagerank.go:117
        const size_t xi = (size_t)lrow * KW + k;
        if (c.act[k]) {
            if constexpr (XS) __hip_atomic_store(&c.xw[xi], xn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else NT_STORE(xn, &c.xw[xi]);
            if (!hub) c.dsum[k] += fabs(xn - xo.v[k]);            // pagerank.go:118
        } else {
            xn = xo.v[k];                                         // converged topic: frozen
        }
        double cc = 0.0;
        if (lrow < p.sl_nd) {                                     // non-dangling row: next sweep's contribution
            cc = p.d * xn / (double)od;                           // pagerank.go:136
            tab_store<PS>(cc, &c.Tw[xi]);
            if (!hub) c.csum[k] += cc;                            // pagerank.go:137
        }
        if (hub) {
            __hip_atomic_store(&hub[k], fabs(xn - xo.v[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&hub[KW + k], cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
template <int KW>
__device__ __forceinline__ NVec<KW> load_x(const double* __restrict__ x, uint32_t lrow) {
    NVec<KW> r;
#pragma unroll
    for (int k = 0; k < KW; k++) r.v[k] = NT_LOAD(&x[(size_t)lrow * KW + k]);
    return r;
}

// rows of exactly D = w.nseg <= ND in-edges: lane l of pass r0 owns row r0 + l of the item
template <int KW, bool TS, int ND, int PS = 0>
__device__ __forceinline__ void deg_lane_rows(NCtx<KW, TS>& c, const WorkItem& w, int lane) {
    const PrParams& p = c.p;
    const uint32_t D = w.nseg;
    for (uint32_t r0 = 0; r0 < w.count; r0 += 64) {
        const uint32_t rr = r0 + (uint32_t)lane;
        const bool valid = rr < w.count;
        const uint32_t lrow = w.row + (valid ? rr : 0u);
        const uint32_t e0 = w.beg + (valid ? rr : 0u) * D;
        uint32_t src[ND];
#pragma unroll
        for (int u = 0; u < ND; u++) {
            const bool ok = valid && (uint32_t)u < D;
            const uint32_t raw = NT_LOAD(&p.in_src[ok ? e0 + (uint32_t)u : w.beg]);
            src[u] = ok ? (raw & SRC_MASK) : p.zrow;
        }
        const NVec<KW> xo = load_x<KW>(c.xr, lrow);
        const uint32_t od = lrow < p.sl_nd ? NT_LOAD(&p.outdeg[lrow]) : 1u;
        NVec<KW> v[ND];
#pragma unroll
        for (int u = 0; u < ND; u++) v[u] = ntab<KW, PS>(c.T, src[u]);
        NVec<KW> acc;
#pragma unroll
        for (int k = 0; k < KW; k++) acc.v[k] = 0.0;
#pragma unroll
        for (int u = 0; u < ND; u++)
#pragma unroll
            for (int k = 0; k < KW; k++) acc.v[k] += v[u].v[k];
        if (valid) finish_n<KW, TS, PS>(c, lrow, acc, xo, od);
    }
}

// one sweep of this block's waves; `sweep` = ctl->sweep as the caller read it.  PS: inside k_pr_multi_n (see ntab)
template <int KW, bool TS, int PS>
__device__ __forceinline__ void sweep_n_body(const PrParams& p, const int sweep, const double (&S_in)[KW], const int (&act_in)[KW]) {
    PrCtl* ctl = p.ctl;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (two-vector form: the vectors alternate between x and x_alt, so that the previous ones are still there for the topics' L1 changes)
    NCtx<KW, TS> c{p, p.tab_rd[sweep & 1], p.tab_wr[sweep & 1], {}, {}, {}, {}, {}, {},
                   (p.x_alt && (sweep & 1)) ? p.x_alt : p.x, p.x_alt ? ((sweep & 1) ? p.x : p.x_alt) : p.x};
#pragma unroll
    for (int k = 0; k < KW; k++) {
        c.tele[k] = p.tele_col ? p.tele_col[k] : p.teleport;          // (per column only in the two-vector form)
        c.S[k] = S_in[k];
        c.act[k] = act_in[k] != 0;
        c.x0[k] = sweep == 0 ? p.x0[k] : 0.0;                     // Q4: iteration 1 accumulates onto 1/n
        c.dsum[k] = 0.0;
        c.csum[k] = 0.0;
    }
    const uint32_t* __restrict__ off = p.woff + (size_t)(blockIdx.x * WAVES + wave) * 8;
    const uint32_t* __restrict__ in_src = p.in_src;

    // The four phases in the order `p.n_order` names (2 bits per position: 0 = long rows, 1 = mid rows, 2 = rows of <= 8 in-edges, 3 = edge-less
    // rows; option "pr.n_class_order"): as in k_pr_sweep the order matters more than the deal (round 5).
    for (int s4 = 0; s4 < 4; s4++) {
    switch ((p.n_order >> (2 * s4)) & 3u) {
    case 0: {
        // ---- V_SEG / V_ROWW: the wave strides the row's (piece's) edges, four gathers per lane in flight
        for (uint32_t it = off[0]; it < off[1]; it++) {
            const WorkItem w = p.work[it];
            const uint32_t lrow = w.row;
            NVec<KW> xo = load_x<KW>(c.xr, lrow);
            const uint32_t od = lrow < p.sl_nd ? NT_LOAD(&p.outdeg[lrow]) : 1u;
            NVec<KW> acc;
    #pragma unroll
            for (int k = 0; k < KW; k++) acc.v[k] = 0.0;
            // (the index words of the next 256 edges are requested before the gathers of the current ones are consumed)
            uint32_t src_n[4];
            auto idx256 = [&](uint32_t e, uint32_t (&src)[4]) __attribute__((always_inline)) {
    #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t j = e + (uint32_t)(u * 64 + lane);
                    const uint32_t raw = NT_LOAD(&in_src[j < w.end ? j : w.beg]);
                    src[u] = j < w.end ? (raw & SRC_MASK) : p.zrow;
                }
            };
            idx256(w.beg, src_n);
            for (uint32_t e = w.beg; e < w.end; e += 256) {
                uint32_t src[4];
    #pragma unroll
                for (int u = 0; u < 4; u++) src[u] = src_n[u];
                idx256(e + 256, src_n);                                       // (past the end: four loads of the first edge, dropped)
                NVec<KW> v[4];
    #pragma unroll
                for (int u = 0; u < 4; u++) v[u] = ntab<KW, PS>(c.T, src[u]);
    #pragma unroll
                for (int u = 0; u < 4; u++)
    #pragma unroll
                    for (int k = 0; k < KW; k++) acc.v[k] += v[u].v[k];
            }
    #pragma unroll
            for (int k = 0; k < KW; k++)
    #pragma unroll
                for (int o = 1; o < 64; o <<= 1) acc.v[k] += __shfl_xor(acc.v[k], o, 64);
            if (w.kind == V_ROWW) {
                if (lane == 0) finish_n<KW, TS, PS>(c, lrow, acc, xo, od);
            } else {
                // several waves (of any blocks) share this row: publish the piece's sum write-through, drain, take the ticket; the
                // last to arrive adds the pieces in order with sc1 loads (no fences — see block_reduce_and_publish)
                const double mine = (KW == 2 && (lane & 1)) ? acc.v[KW - 1] : acc.v[0];
                if (lane < KW) __hip_atomic_store(&p.segpart[(size_t)(w.sbase + w.count) * KW + lane], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                unsigned prev = 0;
                if (lane == 0) prev = __hip_atomic_fetch_add(&p.rowticket[w.tix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                prev = (unsigned)__builtin_amdgcn_readfirstlane((int)prev);
                if (prev == w.nseg - 1) {
                    if (lane == 0) {
                        __hip_atomic_store(&p.rowticket[w.tix], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        NVec<KW> ys;
    #pragma unroll
                        for (int k = 0; k < KW; k++) {
                            ys.v[k] = 0.0;
                            for (uint32_t q = 0; q < w.nseg; q++)
                                ys.v[k] += __hip_atomic_load(&p.segpart[(size_t)(w.sbase + q) * KW + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        if constexpr (PS == 1) {
                            // (the rank this row got in the previous sweep may have been written by another CU: read it now, past its L1)
                            NVec<KW> xs;
    #pragma unroll
                            for (int k = 0; k < KW; k++) xs.v[k] = __hip_atomic_load(&c.xr[(size_t)lrow * KW + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            finish_n<KW, TS, PS, true>(c, lrow, ys, xs, od, p.hubsum + (size_t)w.tix * 2 * KW);
                        } else {
                            finish_n<KW, TS, PS>(c, lrow, ys, xo, od, p.hubsum + (size_t)w.tix * 2 * KW);
                        }
                    }
                }
            }
        }

    } break;
    case 1: {
        // ---- V_QUAD: one row per 8-lane group; the rows of an item are all nch 16-edge turns long
        {
            const int gl = lane & 7, grp = lane >> 3;
            for (uint32_t it = off[1]; it < off[2]; it++) {
                const WorkItem w = p.work[it];
                const uint32_t nq = (w.count + 7) / 8;
                for (uint32_t q = 0; q < nq; q++) {
                    const uint32_t rr = q * 8 + (uint32_t)grp;
                    const bool valid = rr < w.count;
                    const uint32_t lrow = w.row + (valid ? rr : 0u);
                    const uint32_t b = p.in_ptr[lrow], e_end = valid ? p.in_ptr[lrow + 1] : b;
                    NVec<KW> xo = load_x<KW>(c.xr, lrow);
                    const uint32_t od = lrow < p.sl_nd ? NT_LOAD(&p.outdeg[lrow]) : 1u;
                    NVec<KW> acc;
    #pragma unroll
                    for (int k = 0; k < KW; k++) acc.v[k] = 0.0;
                    uint32_t src_n[4];
                    auto idx32 = [&](uint32_t ch, uint32_t (&src)[4]) __attribute__((always_inline)) {
    #pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const uint32_t j = b + ch * 16u + (uint32_t)(u * 8 + gl);
                            const uint32_t raw = NT_LOAD(&in_src[j < e_end ? j : b]);
                            src[u] = j < e_end ? (raw & SRC_MASK) : p.zrow;
                        }
                    };
                    idx32(0, src_n);
                    for (uint32_t ch = 0; ch < w.nseg; ch += 2) {           // two turns (32 edge slots of the row) per trip: four gathers per lane
                        uint32_t src[4];
    #pragma unroll
                        for (int u = 0; u < 4; u++) src[u] = src_n[u];
                        idx32(ch + 2, src_n);                               // the next trip's index words travel with this trip's gathers
                        NVec<KW> v[4];
    #pragma unroll
                        for (int u = 0; u < 4; u++) v[u] = ntab<KW, PS>(c.T, src[u]);
    #pragma unroll
                        for (int u = 0; u < 4; u++)
    #pragma unroll
                            for (int k = 0; k < KW; k++) acc.v[k] += v[u].v[k];
                    }
    #pragma unroll
                    for (int k = 0; k < KW; k++)
    #pragma unroll
                        for (int o = 1; o < 8; o <<= 1) acc.v[k] += __shfl_xor(acc.v[k], o, 64);
                    if (valid && gl == 0) finish_n<KW, TS, PS>(c, lrow, acc, xo, od);
                }
            }
        }

    } break;
    case 2: {
        // ---- V_DEG (all three classes): rows of exactly D <= 8 in-edges, their edges contiguous from item.beg: one lane per row
        for (uint32_t it = off[2]; it < off[5]; it++) {
            const WorkItem w = p.work[it];
            if (w.nseg <= 2) deg_lane_rows<KW, TS, 2, PS>(c, w, lane);          // (wave-uniform: most rows of a power-law graph)
            else if (w.nseg <= 4) deg_lane_rows<KW, TS, 4, PS>(c, w, lane);
            else deg_lane_rows<KW, TS, 8, PS>(c, w, lane);
        }

    } break;
    default: {
        // ---- V_ZERO: non-dangling rows without in-edges: their rank is the shared value, only the next contribution is written
        for (uint32_t it = off[5]; it < off[6]; it++) {
            const WorkItem w = p.work[it];
            for (uint32_t r0 = 0; r0 < w.count; r0 += 64) {
                const uint32_t rr = r0 + (uint32_t)lane;
                if (rr >= w.count) continue;
                const uint32_t lrow = w.row + rr;
                const uint32_t od = NT_LOAD(&p.outdeg[lrow]);
    #pragma unroll
                for (int k = 0; k < KW; k++) {
                    const bool ts = TS && p.memb && ((p.ts_mask >> k) & 1u);
                    const double xz_out = c.act[k] ? (ts ? zero_row_rank_ts(p, sweep, c.S[k], p.x0[k], 0.0) : zero_row_rank_ts(p, sweep, c.S[k], p.x0[k], c.tele[k])) : ctl_ld<PS>(&ctl->xz[k]);
                    const double xz_inn = ts ? (c.act[k] ? zero_row_rank_ts(p, sweep, c.S[k], p.x0[k], p.tin[k]) : ctl_ld<PS>(&ctl->xz_in[k])) : xz_out;
                    const double xz = ts && ((p.memb[lrow] >> k) & 1u) ? xz_inn : xz_out;
                    const double cc = p.d * xz / (double)od;                      // pagerank.go:136
                    tab_store<PS>(cc, &c.Tw[(size_t)lrow * KW + k]);
                    c.csum[k] += cc;                                               // pagerank.go:137
                }
            }
        }

    } break;
    }
    }

    // block_reduce_and_publish<KW> expects lane l to hold a partial of topic l % KW
    double ds = c.dsum[0], cs = c.csum[0];
    if constexpr (KW == 2) {
        const double d0o = __shfl_xor(c.dsum[0], 1, 64), d1o = __shfl_xor(c.dsum[1], 1, 64);
        const double c0o = __shfl_xor(c.csum[0], 1, 64), c1o = __shfl_xor(c.csum[1], 1, 64);
        ds = (lane & 1) ? c.dsum[1] + d1o : c.dsum[0] + d0o;
        cs = (lane & 1) ? c.csum[1] + c1o : c.csum[0] + c0o;
    }
    block_reduce_and_publish<KW, PS>(p, ds, cs, c.Tw, false);
}

template <int KW, bool TS>
__global__ __launch_bounds__(TPB, SS_PRN_MINW) void k_pr_sweep_n(PrParams p) {
    const PrCtl* ctl = p.ctl;
    // (everything this wave needs of the control block is requested before the first of it is looked at: one scalar-load latency
    //  at the start of a sweep that is mostly fixed cost on a small graph, instead of two)
    const int n_active = ctl->n_active, sweep = ctl->sweep;
    double S_in[KW];
    int act_in[KW];
#pragma unroll
    for (int k = 0; k < KW; k++) { S_in[k] = ctl->S[k]; act_in[k] = ctl->active[k]; }
    if (n_active == 0) return;        // every topic converged: the launch is a no-op
    sweep_n_body<KW, TS, false>(p, sweep, S_in, act_in);
}

// ---- several sweeps in ONE launch (round 5: graphs whose sweep is all fixed cost) -------------------------------------------------
// BASELINE config 2 (2^20 nodes / 5M edges, one vector) sweeps in 54 us of which 33 us are an EMPTY grid's: launch, control-block
// reads, the two-level hand-in of the partial sums, kernel end.  pagerank.go:93-119 is a loop; here the loop runs inside the launch:
// every block walks its waves' items, hands its partial sums in exactly as k_pr_sweep_n does, and then WAITS until the last block to
// arrive has applied the stop rule and published the next sweep's number (finalize_ctl<true>: write-through stores, drained, the
// sweep counter last) — that wait is the grid-wide barrier between two sweeps.  Nothing is fenced: whatever one sweep writes for
// another CU to read in the next (the contribution table, the control block, the partial sums, the row pieces' tickets) is stored
// write-through (sc1) and read with L1-bypassing sc1 loads (MI355X_MICROARCH.md, hand-offs without fences; the ranks x are read and
// written by the same lane of the same wave in every sweep — the deal is static — and need nothing).  The arithmetic and its order
// are those of k_pr_sweep_n: ranks and iteration counts are bit-identical to one launch per sweep.
// Residency: the grid is sized by the host to HALF of what the occupancy query admits (ss_pr_create), so that it is resident whatever
// else runs; a wait that still ends without the counter moving (SPIN_MAX polls, seconds) sets ctl->stuck and every block leaves — the
// host reports SS_ERR_STATE instead of a hung device.
constexpr uint32_t MULTI_SPIN_MAX = 1u << 24;
// PSM 1: write-through / sc1 form (above).  PSM 2: plain stores and loads with an agent-scope release in front of every block's arrival
// and an acquire behind every block's wait (the table then stays in the XCD's L2 for the block's own gathers, as between launches).
template <int KW, int PSM>
__global__ __launch_bounds__(TPB, SS_PRN_MINW) void k_pr_multi_n(PrParams p, int n_steps) {
    __shared__ int s_go, s_na, s_sw, s_act[KW];
    __shared__ double s_S[KW];
    PrCtl* ctl = p.ctl;
    // ONE lane per block reads the control block (write-through data: sc1 loads that all land on one L2 channel — every lane of 4096 waves
    // reading it was 20k requests to that channel per sweep) and hands it to the block through LDS
    auto read_ctl = [&]() __attribute__((always_inline)) {
        s_na = ctl_ld<1>(&ctl->n_active) == 0 || ctl_ld<1>(&ctl->stuck) ? 0 : 1;
        s_sw = ctl_ld<1>(&ctl->sweep);
#pragma unroll
        for (int k = 0; k < KW; k++) { s_S[k] = ctl_ld<1>(&ctl->S[k]); s_act[k] = ctl_ld<1>(&ctl->active[k]); }
    };
    if (threadIdx.x == 0) read_ctl();
    __syncthreads();
    for (int s = 0; s < n_steps; s++) {
        // (every block reads the same control block: it only changes when ALL blocks have handed in the sweep)
        if (s_na == 0) return;                                    // every topic has stopped: the remaining sweeps are no-ops
        const int sweep = s_sw;
        double S_in[KW];
        int act_in[KW];
#pragma unroll
        for (int k = 0; k < KW; k++) { S_in[k] = s_S[k]; act_in[k] = s_act[k]; }
        __syncthreads();                                          // (everybody has its copy: lane 0 may rewrite the LDS words below)
        sweep_n_body<KW, false, PSM>(p, sweep, S_in, act_in);
        if (s + 1 == n_steps) return;                             // the kernel boundary is the last barrier
        if (threadIdx.x == 0) {
            uint32_t spins = 0;
            while (ctl_ld<1>(&ctl->sweep) == sweep && ++spins < MULTI_SPIN_MAX) __builtin_amdgcn_s_sleep(8);
            const bool ok = spins < MULTI_SPIN_MAX;
            if (!ok) ctl_st<1>(&ctl->stuck, 1u);
            s_go = ok ? 1 : 0;
            if (ok) read_ctl();
            if constexpr (PSM == 2) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // drops this CU's L1 lines: the other blocks' table rows and ranks
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (holds the barrier until the invalidate has completed)
            }
        }
        __syncthreads();
        if (!s_go) return;
    }
}

template __device__ void begin_caller_context<1, 2>(const PrParams&, double*);   // pr_device.hpp: keeps the helpers' code the parent file's

}  // namespace

namespace ss {
void pr_sweep_n_launch(ss_pr* pr, hipStream_t st) {
    const bool ts = pr->prm.memb != nullptr;
    if (pr->gw == 1) {
        if (ts) hipLaunchKernelGGL((k_pr_sweep_n<1, true>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else hipLaunchKernelGGL((k_pr_sweep_n<1, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
    } else {
        if (ts) hipLaunchKernelGGL((k_pr_sweep_n<2, true>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
        else hipLaunchKernelGGL((k_pr_sweep_n<2, false>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
    }
}
int pr_sweep_n_occupancy(int gw) {
    int per_cu = 8;
    if (gw == 1) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_sweep_n<1, false>, TPB, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_sweep_n<2, false>, TPB, 0);
    return per_cu;
}
// the sweeps wait for each other inside the launch (pr->persist_mode 1: write-through hand-offs, 2: fences)
void pr_multi_n_launch(ss_pr* pr, hipStream_t st, int n_steps) {
    if (pr->gw == 1) {
        if (pr->persist_mode == 2) hipLaunchKernelGGL((k_pr_multi_n<1, 2>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm, n_steps);
        else hipLaunchKernelGGL((k_pr_multi_n<1, 1>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm, n_steps);
    } else {
        if (pr->persist_mode == 2) hipLaunchKernelGGL((k_pr_multi_n<2, 2>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm, n_steps);
        else hipLaunchKernelGGL((k_pr_multi_n<2, 1>), dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm, n_steps);
    }
}
int pr_multi_n_occupancy(int gw) {
    int per_cu = 0;
    if (gw == 1) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_multi_n<1, 1>, TPB, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pr_multi_n<2, 1>, TPB, 0);
    return per_cu;
}
}  // namespace ss
