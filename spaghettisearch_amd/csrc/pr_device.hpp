// pr_device.hpp — the device helpers that more than one family of PageRank kernels uses: the per-topic wave sum, the shared rank of
// the rows without in-edges, the teleport of a (row, topic), the control block's accesses and its finalize, the hand-in of the block
// partial sums (block_reduce_and_publish), the cache policy of the streaming data.  Included by pagerank.hip (begin / finalize / read
// kernels), pr_sweep.hip, pr_sweep_n.hip and pr_step.hip; in an anonymous namespace, like score_common.hpp: every translation unit has
// its own copy of the device code.  A helper that only one family uses lives in that family's file.
#pragma once
#include "pr_state.hpp"

#include <cmath>

namespace {

// ---- reductions --------------------------------------------------------------

// sum over the lanes of a wave that hold the same topic (lane % GW), fixed butterfly order
template <int GW>
__device__ __forceinline__ double wave_sum_topic(double v) {
#pragma unroll
    for (int off = GW; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Rows without in-edges inherit nothing: cur = (1/n if first sweep) + 0, so after the normalise they ALL
// hold the same value per topic.  They are never stored or streamed; this is that shared value.
__device__ __forceinline__ double zero_row_rank(const PrParams& p, int sweep, double S, double x0) {
    return ((sweep == 0 ? x0 : 0.0) + p.teleport) / S;            // pagerank.go:104,117
}
// Teleport of (row, topic).  Reference: the absolute (1-d) for every node (pagerank.go:117).  With a teleport set
// (Haveliwala's topic-sensitive PageRank, README.md:9 — opt-in) the same total mass (1-d)*N is spread
// over the set's nodes only, so the normaliser S = sum w + (1-d)*N (pagerank.go:112) keeps its meaning.
__device__ __forceinline__ double teleport_of(const PrParams& p, uint32_t lrow, int t) {
    if (!p.memb || !((p.ts_mask >> t) & 1u)) return p.teleport;
    return ((p.memb[lrow] >> t) & 1u) ? p.tin[t] : 0.0;
}
__device__ __forceinline__ double zero_row_rank_ts(const PrParams& p, int sweep, double S, double x0, double tele) {
    return ((sweep == 0 ? x0 : 0.0) + tele) / S;
}

// The control block as the persistent multi-sweep kernel (k_pr_multi_n) needs it: written by the last block of sweep i, read by every
// block of sweep i + 1 INSIDE one launch, i.e. across CUs and XCDs with no kernel boundary in between — write-through stores and
// L1-bypassing loads (sc1; scalar loads would come from the never-refreshed scalar cache).  The one-sweep kernels use plain accesses.
template <int PS, typename T>
__device__ __forceinline__ T ctl_ld(const T* q) {
    if constexpr (PS) return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *q;
}
template <int PS, typename T>
__device__ __forceinline__ void ctl_st(T* q, T v) {
    if constexpr (PS) __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *q = v;
}

template <int PS = 0>
__device__ __forceinline__ void finalize_ctl(const PrParams& p, const double* dl, const double* cs, bool is_begin) {
    PrCtl* ctl = p.ctl;
    if (p.aff) {
        // columns 0 / 1 = p / q.  Both are divided by the common sigma = r' + s' (r' = W p + tau*N*r, s' = W q + tau*N*s), their
        // teleports are tau*r and tau*s.
        AffCtl* a = p.aff;
        if (is_begin) {
            // start: p = 1, q = 0, r = 0, s = 1
            const double r1 = cs[0], s1 = cs[1] + p.tele_n, sigma = r1 + s1;
            for (int k = 0; k < MAXK; k++) {
                const bool real = k < 2;
                ctl->xz[k] = real ? p.x0[k] : 0.0;
                ctl->xz_in[k] = ctl->xz[k];
                ctl->S[k] = real ? sigma : 1.0;
                ctl->csum[k] = real ? cs[k] : 0.0;
                ctl->delta[k] = 0.0;
                ctl->active[k] = real ? 1 : 0;
                ctl->iters[k] = 0;
                ctl->tele[k] = 0.0;
            }
            ctl->tele[1] = p.teleport;                                // tau * s with s = 1; tele[0] = tau * r with r = 0
            a->r_x = 0.0; a->s_x = 1.0;
            a->r_prev = 0.0; a->s_prev = 1.0;
            a->r_next = r1 / sigma; a->s_next = s1 / sigma;
            a->xz_prev[0] = ctl->xz[0];
            a->xz_prev[1] = ctl->xz[1];
            a->it = 0;
            ctl->sweep = 0;
            ctl->n_active = 2;
            return;
        }
        const int it = ctl->sweep + 1;
        a->r_prev = a->r_x; a->s_prev = a->s_x;
        a->r_x = a->r_next; a->s_x = a->s_next;                       // (r, s) of the vectors this sweep has written
        for (int k = 0; k < 2; k++) {
            a->xz_prev[k] = ctl->xz[k];
            ctl->xz[k] = zero_row_rank_ts(p, ctl->sweep, ctl->S[k], p.x0[k], ctl->tele[k]);
            ctl->xz_in[k] = ctl->xz[k];
            ctl->iters[k] = it;
            ctl->csum[k] = cs[k];
        }
        const double r1 = cs[0] + p.tele_n * a->r_x;                  // W p + tau*N*r
        const double s1 = cs[1] + p.tele_n * a->s_x;                  // W q + tau*N*s
        const double sigma = r1 + s1;
        a->r_next = r1 / sigma;
        a->s_next = s1 / sigma;
        ctl->tele[0] = p.teleport * a->r_x;
        ctl->tele[1] = p.teleport * a->s_x;
        ctl->S[0] = ctl->S[1] = sigma;
        ctl->sweep = it;
        return;
    }
    if (is_begin) {
        for (int k = 0; k < MAXK; k++) {
            const bool real = k < p.k_topics;
            ctl->xz[k] = real ? p.x0[k] : 0.0;
            ctl->xz_in[k] = real ? p.x0[k] : 0.0;
            ctl->S[k] = real ? cs[k] + p.tele_n : 1.0;
            ctl->csum[k] = real ? cs[k] : 0.0;
            ctl->delta[k] = 0.0;
            ctl->active[k] = real ? 1 : 0;
            ctl->iters[k] = 0;
        }
        ctl->sweep = 0;
        ctl->n_active = p.k_topics;
        return;
    }
    const int sw = ctl_ld<PS>(&ctl->sweep);
    const int it = sw + 1;
    int na = 0;
    for (int k = 0; k < p.k_topics; k++) {
        if (ctl_ld<PS>(&ctl->active[k])) {
            const double Sk = ctl_ld<PS>(&ctl->S[k]);
            ctl_st<PS>(&ctl->iters[k], it);
            ctl_st<PS>(&ctl->delta[k], dl[k]);              // includes the rows without in-edges (added by the caller)
            if (p.memb && ((p.ts_mask >> k) & 1u)) {
                ctl_st<PS>(&ctl->xz[k], zero_row_rank_ts(p, sw, Sk, p.x0[k], 0.0));
                ctl_st<PS>(&ctl->xz_in[k], zero_row_rank_ts(p, sw, Sk, p.x0[k], p.tin[k]));
            } else {
                const double xz = zero_row_rank(p, sw, Sk, p.x0[k]);
                ctl_st<PS>(&ctl->xz[k], xz);
                ctl_st<PS>(&ctl->xz_in[k], xz);
            }
            bool cont = dl[k] > p.eps;                      // pagerank.go:93
            if (p.max_iter > 0 && it >= p.max_iter) cont = false;
            ctl_st<PS>(&ctl->active[k], cont ? 1 : 0);
            na += cont ? 1 : 0;
            ctl_st<PS>(&ctl->S[k], cs[k] + p.tele_n);       // pagerank.go:111-112
            ctl_st<PS>(&ctl->csum[k], cs[k]);
        }
    }
    ctl_st<PS>(&ctl->n_active, na);
    if constexpr (PS) {
        // `sweep` is what the other blocks poll between two sweeps: it goes last, behind everything else this thread has stored
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    ctl_st<PS>(&ctl->sweep, it);
}

// Block partial -> global partials; the last block to arrive sums all partials in a
// fixed order and either finalises the control block (world==1) or leaves this
// rank's totals in the tail rows of the send buffer (world>1).
template <int GW, int PS = 0>
__device__ __forceinline__ void block_reduce_and_publish(const PrParams& p, double dsum, double csum, double* tail,
                                                         bool is_begin) {
    __shared__ double red[WAVES][2][MAXK];
    __shared__ double tot[2][MAXK];
    __shared__ double colsum[TPB];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = lane % GW;
    dsum = wave_sum_topic<GW>(dsum);
    csum = wave_sum_topic<GW>(csum);
    if (lane < GW) {
        red[wave][0][t] = dsum;
        red[wave][1][t] = csum;
    }
    __syncthreads();
    // Hand-off of the block's partial sums to the last block to arrive, without fences (a release would write back the
    // XCD's whole dirty L2 — this sweep's rank and table stores — once per block; MI355X_MICROARCH.md, hand-off forms):
    // every partial is stored write-through (sc1), the storing wave drains its stores, one lane takes a ticket with an
    // agent-scope atomic, and the last block reads the partials with sc1 loads.
    if (threadIdx.x < 2 * GW) {
        const int which = threadIdx.x / GW, tt = threadIdx.x % GW;
        double v = red[0][which][tt];
#pragma unroll
        for (int w = 1; w < WAVES; w++) v += red[w][which][tt];
        __hip_atomic_store(&p.partials[(size_t)blockIdx.x * 2 * GW + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // Two levels, so that nobody sums a thousand rows alone: the blocks form NG groups (block % NG); the last block of a
    // group to arrive sums the group's rows (one batch of loads per thread) into a group row, the last group to finish
    // sums the NG group rows.  Fixed grouping, fixed order: deterministic.
    constexpr unsigned NG = 8;
    constexpr int NCOL = 2 * GW;
    constexpr int NPART = TPB / NCOL;
    const unsigned ng = min(NG, gridDim.x);
    const unsigned grp = blockIdx.x % ng;
    const unsigned members = (gridDim.x - grp + ng - 1) / ng;         // blocks b = grp, grp + ng, ...
    double* const gpart = p.partials + (size_t)gridDim.x * NCOL;      // [NG][NCOL] behind the block rows
    if (threadIdx.x == 0) {
        if constexpr (PS == 2) {
            // fence form of k_pr_multi_n: this block's table and rank stores (plain: they stay in the XCD's L2 for its own gathers) are
            // written back before the block counts as arrived; the wait behind the fence is spelled out (ROCm 7.2 can drop the fence's own)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned prev = __hip_atomic_fetch_add(&p.ctl->gticket[grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == members - 1;
    }
    __syncthreads();
    if (!s_last) return;
    const int col = threadIdx.x % NCOL, part = threadIdx.x / NCOL;
    {
        double acc = 0.0;
        for (unsigned m0 = part; m0 < members; m0 += 16 * NPART) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const unsigned m = m0 + u * NPART;
                v[u] = __hip_atomic_load(&p.partials[(size_t)(grp + ng * (m < members ? m : m0)) * NCOL + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (m0 + u * NPART < members) acc += v[u];
        }
        colsum[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x < NCOL) {
        double v = 0.0;
        for (int q = 0; q < NPART; q++) v += colsum[q * NCOL + threadIdx.x];
        __hip_atomic_store(&gpart[(size_t)grp * NCOL + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) ctl_st<PS>(&p.ctl->gticket[grp], 0u);       // every member has arrived: ready for the next sweep (drained below, in front of this block's ticket)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(&p.ctl->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == ng - 1;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x < NCOL) {
        double v = 0.0;
        for (unsigned gq = 0; gq < ng; gq++)
            v += __hip_atomic_load(&gpart[(size_t)gq * NCOL + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot[threadIdx.x / GW][threadIdx.x % GW] = v;
    } else if (!is_begin && p.nmulti) {
        // the rows that were cut into pieces (PrParams::hubsum): the other threads add their terms meanwhile, in row order
        const unsigned hp = threadIdx.x / NCOL - 1;                   // 0 .. NPART - 2
        double acc = 0.0;
        for (unsigned h0 = hp; h0 < p.nmulti; h0 += 16 * (NPART - 1)) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const unsigned h = h0 + u * (NPART - 1);
                v[u] = __hip_atomic_load(&p.hubsum[(size_t)(h < p.nmulti ? h : h0) * NCOL + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (h0 + u * (NPART - 1) < p.nmulti) acc += v[u];
        }
        colsum[threadIdx.x] = acc;
    }
    __syncthreads();
    if (!is_begin && p.nmulti && threadIdx.x < NCOL) {
        double v = tot[threadIdx.x / GW][threadIdx.x % GW];
        for (int q = 1; q < NPART; q++) v += colsum[q * NCOL + threadIdx.x];
        tot[threadIdx.x / GW][threadIdx.x % GW] = v;
    }
    __syncthreads();
    // rows without in-edges: all equal, so their L1 change is count * |new - old| (not streamed, see zero_row_rank)
    if (!is_begin && threadIdx.x < GW && ctl_ld<PS>(&p.ctl->active[threadIdx.x])) {
        const double n_zero = (double)((p.cnt_nd - p.pos_nd) + (p.cnt_d - p.pos_d));
        if (p.memb && ((p.ts_mask >> threadIdx.x) & 1u)) {
            // two values per topic: inside and outside the teleport set
            const int k = threadIdx.x;
            const double out_new = zero_row_rank_ts(p, ctl_ld<PS>(&p.ctl->sweep), ctl_ld<PS>(&p.ctl->S[k]), p.x0[k], 0.0);
            const double in_new = zero_row_rank_ts(p, ctl_ld<PS>(&p.ctl->sweep), ctl_ld<PS>(&p.ctl->S[k]), p.x0[k], p.tin[k]);
            tot[0][k] += (n_zero - p.nz_in[k]) * fabs(out_new - ctl_ld<PS>(&p.ctl->xz[k])) + p.nz_in[k] * fabs(in_new - ctl_ld<PS>(&p.ctl->xz_in[k]));
        } else {
            const double xz_new = zero_row_rank(p, ctl_ld<PS>(&p.ctl->sweep), ctl_ld<PS>(&p.ctl->S[threadIdx.x]), p.x0[threadIdx.x]);
            tot[0][threadIdx.x] += n_zero * fabs(xz_new - ctl_ld<PS>(&p.ctl->xz[threadIdx.x]));
        }
    }
    __syncthreads();
    if (p.world == 1) {
        if (threadIdx.x == 0) {
            double dl[MAXK], cs[MAXK];
            for (int k = 0; k < MAXK; k++) {
                dl[k] = k < GW ? tot[0][k] : 0.0;
                cs[k] = k < GW ? tot[1][k] : 0.0;
            }
            ctl_st<PS>(&p.ctl->ticket, 0u);                          // (in front of finalize_ctl: its last store releases the next sweep)
            finalize_ctl<PS>(p, dl, cs, is_begin);
        }
    } else {
        // tail rows of this rank's all-gather piece: row sl_nd-2 = contribution sums, row sl_nd-1 = deltas
        if (threadIdx.x < GW) {
            tail[(size_t)(p.sl_nd - 2) * GW + threadIdx.x] = tot[1][threadIdx.x];
            tail[(size_t)(p.sl_nd - 1) * GW + threadIdx.x] = tot[0][threadIdx.x];
        }
        if (threadIdx.x == 0) p.ctl->ticket = 0;
    }
}

// The compile context of the two helpers above, for a file whose kernels all pass is_begin = false (the sweep-kernel families: only
// k_pr_begin in pagerank.hip passes true).  With nothing but `false` callers in a translation unit the compiler's interprocedural
// constant propagation, which runs in front of the inliner, folds the argument into the helpers first, and what is inlined into
// the sweep kernels afterwards comes out differently from the code measured and recorded for them (k_pr_sweep_n: 128 bytes more
// scratch, k_pr_sweep / k_pr_step / k_pr_sweep_n: 1 - 27 instructions fewer behind the hand-in; profiles/
// pagerank_kernels_split_resources.txt).  A family file instantiates this once for its two widths: a never-called function that
// shows that pass a caller with is_begin = true, as k_pr_begin did when all kernels shared one file.  `used` keeps it until that pass
// has run; its body sits behind a test that is false but decided only late in the pipeline, so nothing of it reaches the code object
// beyond a two-instruction stub, and no kernel's LDS or registers know of it.
template <int GA, int GB>
__device__ __attribute__((used, noinline)) void begin_caller_context(const PrParams& p, double* tail) {
    if (!__builtin_constant_p(p.world)) return;
    block_reduce_and_publish<GA>(p, 0.0, 0.0, tail, true);
    block_reduce_and_publish<GB>(p, 0.0, 0.0, tail, true);
}

// Streaming data (ranks, indices, next contributions) is touched once per sweep: mark it
// non-temporal so that it does not push the randomly gathered table out of L2.
#define NT_LOAD(p) __builtin_nontemporal_load(p)
#define NT_STORE(v, p) __builtin_nontemporal_store(v, p)

constexpr uint32_t SRC_MASK = 0x7FFFFFFFu;   // in_src bit 31 = "last in-edge of its row" (graph.hip)

}  // namespace
