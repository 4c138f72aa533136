// pr_step.hip — k_pr_step<1|2>: the block-item sweep for K <= 2, reached only through "pr.force_narrow" and "pr.narrow_wave" = 0
// (ss_pr_create's kernel choice in pagerank.hip; DESIGN.md K1, k_pr_step).  Exports ss::pr_step_launch and ss::pr_step_occupancy.
#include "pr_device.hpp"

namespace {

// sum of T[src][t] over edges beg+first, beg+first+stride, ... < end; 4 gathers in flight
template <int GW>
__device__ __forceinline__ double gather_sum(const double* __restrict__ T, const uint32_t* __restrict__ in_src,
                                             size_t beg, size_t end, unsigned first, unsigned stride, int t) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    size_t e = beg + first;
    for (; e + 3 * (size_t)stride < end; e += 4 * (size_t)stride) {
        const uint32_t s0 = in_src[e] & SRC_MASK, s1 = in_src[e + stride] & SRC_MASK,
                       s2 = in_src[e + 2 * (size_t)stride] & SRC_MASK, s3 = in_src[e + 3 * (size_t)stride] & SRC_MASK;
        a0 += T[(size_t)s0 * GW + t];
        a1 += T[(size_t)s1 * GW + t];
        a2 += T[(size_t)s2 * GW + t];
        a3 += T[(size_t)s3 * GW + t];
    }
    for (; e < end; e += stride) a0 += T[(size_t)(in_src[e] & SRC_MASK) * GW + t];
    return (a0 + a1) + (a2 + a3);
}

// ---- the sweep, K <= 2 (GW = 1 / 2) on graphs whose padded table would not stay cache-resident ---------------
// Persistent grid: a fixed number of blocks walks the work table round-robin, so the
// per-launch costs (partials, ticket) are paid ~2k times, not per work item.  (K >= 3: k_pr_sweep in pr_sweep.hip.)
template <int GW>
__global__ __launch_bounds__(TPB) void k_pr_step(PrParams p) {
    constexpr int NSLOT = 64 / GW;
    __shared__ double rowred[WAVES][MAXK];
    __shared__ int s_rowlast;

    PrCtl* ctl = p.ctl;
    if (ctl->n_active == 0) return;   // every topic converged: the launch is a no-op
    const int sweep = ctl->sweep;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = lane % GW, slot = lane / GW;
    const double S = ctl->S[t];
    const bool act = ctl->active[t] != 0;
    const double x0 = sweep == 0 ? p.x0[t] : 0.0;      // Q4: iteration 1 accumulates onto 1/n
    const double* __restrict__ T = p.tab_rd[sweep & 1];
    double* __restrict__ Tw = p.tab_wr[sweep & 1];

    double dsum = 0.0, csum = 0.0;

    // hub: a row of several segments, finished by whichever block arrives last — its terms go to the row's own slot (PrParams::hubsum)
    auto finish = [&](uint32_t lrow, double y, double* hub) __attribute__((always_inline)) {
        const double xo = NT_LOAD(&p.x[(size_t)lrow * GW + t]);
        const uint32_t od = lrow < p.sl_nd ? NT_LOAD(&p.outdeg[lrow]) : 1u;
        y += x0;
        const size_t xi = (size_t)lrow * GW + t;
        double xn = (y + teleport_of(p, lrow, t)) / S;  // pagerank.go:117
        if (act) {
            NT_STORE(xn, &p.x[xi]);
            if (!hub) dsum += fabs(xn - xo);            // pagerank.go:118
        } else {
            xn = xo;                                    // converged topic: frozen
        }
        double c = 0.0;
        if (lrow < p.sl_nd) {                           // non-dangling row: next sweep's contribution
            c = p.d * xn / (double)od;                  // pagerank.go:136
            NT_STORE(c, &Tw[xi]);
            if (!hub) csum += c;                        // pagerank.go:137
        }
        if (hub) {
            __hip_atomic_store(&hub[t], fabs(xn - xo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&hub[GW + t], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };

    for (uint32_t item = blockIdx.x; item < p.n_items; item += gridDim.x) {
        const WorkItem w = p.work[item];
        if (w.kind == W_SEG) {
            // one block per segment of a long row
            const uint32_t lrow = w.row;
            const size_t rbeg = p.in_ptr[lrow], rend = p.in_ptr[lrow + 1];
            const size_t beg = rbeg + (size_t)w.count * p.seg_edges;
            const size_t end = min(rend, beg + (size_t)p.seg_edges);
            double acc = gather_sum<GW>(T, p.in_src, beg, end, wave * NSLOT + slot, WAVES * NSLOT, t);
            acc = wave_sum_topic<GW>(acc);
            __syncthreads();                            // rowred / s_rowlast reuse across items
            if (lane < GW) rowred[wave][t] = acc;
            __syncthreads();
            double y = 0.0;
            if (threadIdx.x < GW) {
                y = rowred[0][t];
#pragma unroll
                for (int q = 1; q < WAVES; q++) y += rowred[q][t];
            }
            if (w.nseg == 1) {
                if (threadIdx.x < GW) finish(lrow, y, nullptr);
            } else {
                // several blocks share this row: publish the segment partial; the last
                // arriver adds the partials in segment order and finishes the row
                // (the fence-free hand-off of block_reduce_and_publish / long_rows: the partial is stored write-through by
                // wave 0, which drains its stores and then takes the ticket itself; the last arriver reads with sc1 loads)
                if (threadIdx.x < GW) __hip_atomic_store(&p.segpart[(size_t)(w.sbase + w.count) * GW + t], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (threadIdx.x == 0) {
                    const unsigned prev = __hip_atomic_fetch_add(&p.rowticket[w.tix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int last = prev == w.nseg - 1;
                    if (last) __hip_atomic_store(&p.rowticket[w.tix], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_rowlast = last;
                }
                __syncthreads();
                if (s_rowlast && threadIdx.x < GW) {
                    double ys = 0.0;
                    for (uint32_t q = 0; q < w.nseg; q++)
                        ys += __hip_atomic_load(&p.segpart[(size_t)(w.sbase + q) * GW + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    finish(lrow, ys, p.hubsum + (size_t)w.tix * 2 * GW);
                }
            }
        } else if (w.kind == W_WAVE) {
            // one wave per row, the wave's lane groups stride the row's in-edges
            if ((uint32_t)wave < w.count) {
                const uint32_t lrow = w.row + wave;
                const size_t beg = p.in_ptr[lrow], end = p.in_ptr[lrow + 1];
                double acc = gather_sum<GW>(T, p.in_src, beg, end, slot, NSLOT, t);
                acc = wave_sum_topic<GW>(acc);
                if (slot == 0) finish(lrow, acc, nullptr);
            }
        } else if (w.kind == W_GROUP) {
            // one lane group (GW lanes) per row; rows are degree-sorted so trip counts match inside a wave
            for (uint32_t r = wave * NSLOT + slot; r < w.count; r += WAVES * NSLOT) {
                const uint32_t lrow = w.row + r;
                const size_t beg = p.in_ptr[lrow], end = p.in_ptr[lrow + 1];
                double acc = 0.0;
                for (size_t e = beg; e < end; e++) acc += T[(size_t)(p.in_src[e] & SRC_MASK) * GW + t];
                finish(lrow, acc, nullptr);
            }
        } else {
            // non-dangling rows without in-edges: their rank is the shared value xz, only the next
            // contribution d*xz/outdeg has to be written (dangling ones need nothing at all)
            const bool ts = p.memb && ((p.ts_mask >> t) & 1u);
            const double xz_out = act ? (ts ? zero_row_rank_ts(p, sweep, S, p.x0[t], 0.0) : zero_row_rank(p, sweep, S, p.x0[t])) : ctl->xz[t];
            const double xz_inn = ts ? (act ? zero_row_rank_ts(p, sweep, S, p.x0[t], p.tin[t]) : ctl->xz_in[t]) : xz_out;
            const uint32_t nel = w.count * GW;
            for (uint32_t i = threadIdx.x; i < nel; i += TPB) {
                const uint32_t lrow = w.row + i / GW;
                const double xz = ts && ((p.memb[lrow] >> t) & 1u) ? xz_inn : xz_out;
                const double c = p.d * xz / (double)NT_LOAD(&p.outdeg[lrow]);   // pagerank.go:136
                NT_STORE(c, &Tw[(size_t)lrow * GW + t]);
                csum += c;                                                        // pagerank.go:137
            }
        }
    }

    block_reduce_and_publish<GW>(p, dsum, csum, Tw, false);
}

template __device__ void begin_caller_context<1, 2>(const PrParams&, double*);   // pr_device.hpp: keeps the helpers' code the parent file's

}  // namespace

namespace ss {
void pr_step_launch(ss_pr* pr, hipStream_t st) {
    if (pr->gw == 1) hipLaunchKernelGGL(k_pr_step<1>, dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
    else hipLaunchKernelGGL(k_pr_step<2>, dim3(pr->nblocks), dim3(TPB), 0, st, pr->prm);
}
// (not asked of the runtime: the grid is 8 blocks per CU at most, whatever the kernel's registers admit — grid_for in pagerank.hip)
int pr_step_occupancy(int) { return 8; }
}  // namespace ss
