// pagerank.hip — Topic-Sensitive PageRank power iteration for gfx950 (MI355X).
//
// Replaces ranking/pagerank.go:85-145 (updatePagerank + computeRankInherited),
// all categories of pagerank.go:54-63 at once: one K-wide sweep per iteration.
//
// Reference arithmetic per topic (Q3-Q6 of SURVEY.md §7):
//   w_p      = d * last[p] / outdeg(p)            for every p with outdeg>0   (:136)
//   total    = sum_p w_p + (1-d) * N                                          (:137,:112)
//   cur[v]   = (1/n if iteration==1 else 0) + sum_{p->v} w_p                  (:97-107,:140-142)
//   cur[v]   = (cur[v] + (1-d)) / total                                       (:117)
//   change   = sum_v |cur[v]-last[v]| ; loop while change > eps               (:93,:118)
//
// HBM layout (node-major, the K topic values of a node are contiguous so that ONE
// index read serves K gathers and a K=16 gather is one 128-byte line):
//   x     [n_local][GW]   rank of this rank's rows, updated in place
//   table [nd_int+1][GW]  contributions w_p of ALL non-dangling nodes, read by
//                         random gather; written for the next sweep; the last row is
//                         all zero (where the unused slots of a turn gather from)
//                         ("pr.share_zero_rows", k_pr_sweep without teleport sets: the rows without in-edges are not
//                          in the table — one shared row per distinct out-degree stands behind the zero row, and the
//                          state's own copy of in_src names it: SharedRows in pr_plan.hpp)
//                         (world==1: ping-pong pair; world>1: own slice -> `send`,
//                          ss_pr_exchange all-gathers it into `table`)
// One kernel per sweep (k_pr_sweep for K >= 3, k_pr_sweep_n for K <= 2; k_pr_step by option: pick_kernel below).
// The pull SpMV, the normalise, the L1 delta, the next sweep's contributions and
// their sum (next `total`) are fused; block partial sums are handed to the last
// block to arrive (write-through stores + ticket, no fences) and combined in a fixed
// order; that block also applies the stop rule — the loop needs no host round trip
// per iteration.
//
// Algorithmic bytes per sweep: 4E + 8N + 16*K*N.
//
// This file: the small kernels (begin, finalize, read-out, teleport sets, create-time passes, the probe), the choice of the sweep
// kernel and its one dispatch (pick_kernel, ss::pr_launch_step), ss_pr_create and the ss_pr_* stepping API.  The sweep kernels are
// one file per family, each behind a launcher and an occupancy query declared in pr_state.hpp: pr_sweep.hip (k_pr_sweep),
// pr_sweep_n.hip (k_pr_sweep_n, k_pr_multi_n), pr_step.hip (k_pr_step); the device helpers they share with this file's kernels are
// in pr_device.hpp.  The state and the kernel parameters are in pr_state.hpp, the work plan (items, deal, placement: host-only) in
// pr_plan.hpp, the one-call drivers (ss_pagerank_run*), the two-vector kernels and float32 on the wire in pagerank_run.hip.
#include "pr_device.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>

namespace {

// k_pr_sweep's items: their in-edge ranges from the device's in_ptr (the host deals the items by their turn counts, which it
// knows from the sorted in-degrees; copying in_ptr itself to the host cost 14 of the 17 ms of ss_pr_create at 10M nodes)
__global__ void k_pr_item_ranges(WorkItem* __restrict__ work, uint32_t n_items, const uint32_t* __restrict__ in_ptr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    WorkItem w = work[i];
    switch (w.kind) {
        case V_ROWW: w.beg = in_ptr[w.row]; w.end = in_ptr[w.row + 1]; break;
        case V_SEG:
            w.beg = in_ptr[w.row] + w.count * SEGW;
            w.end = min(in_ptr[w.row + 1], w.beg + SEGW);
            break;
        case V_QUAD:
        case V_DEG: w.beg = in_ptr[w.row]; w.end = in_ptr[w.row + w.count]; break;
        default: return;
    }
    work[i] = w;
}

// "pr.share_zero_rows": the state's copy of the in-edge stream.  A source without in-edges (>= pos_nd) becomes the shared row of its
// out-degree (sh_deg is rising: a bisection), flag bits kept; every other word is copied.  One streaming pass at create time.
__global__ __launch_bounds__(TPB) void k_pr_remap_src(const uint32_t* __restrict__ in_src, uint32_t* __restrict__ out, size_t n_edges, uint32_t pos_nd,
                                                      uint32_t cnt_nd, const uint32_t* __restrict__ outdeg, const uint32_t* __restrict__ sh_deg,
                                                      uint32_t n_shared, uint32_t zrow) {
    for (size_t e = (size_t)blockIdx.x * TPB + threadIdx.x; e < n_edges; e += (size_t)gridDim.x * TPB) {
        uint32_t w = NT_LOAD(&in_src[e]);
        const uint32_t s = w & SRC_MASK;
        if (s >= pos_nd) {
            uint32_t row = zrow;                              // (a source outside the map — there is none — would add an exact 0.0)
            if (s < cnt_nd && n_shared) {
                const uint32_t od = outdeg[s];
                uint32_t lo = 0, hi = n_shared;               // first j with sh_deg[j] >= od
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sh_deg[mid] < od) lo = mid + 1; else hi = mid;
                }
                if (lo < n_shared && sh_deg[lo] == od) row = zrow + 1 + lo;
            }
            w = (w & ~SRC_MASK) | row;
        }
        NT_STORE(w, &out[e]);
    }
}

// x0 = 1/n, first contributions and their sum (pagerank.go:103-106 + first :136-137)
template <int GW>
__global__ __launch_bounds__(TPB) void k_pr_begin(PrParams p) {
    const int lane = threadIdx.x & 63;
    const int t = lane % GW;
    const double x0 = p.x0[t];
    double* __restrict__ Tw = p.tab_wr[1];   // the table sweep 0 reads (tab_rd[0]) — see pr_make_params
    double csum = 0.0;
    // (p.share: the first table's shared rows, as k_pr_sweep writes them for the later ones)
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < p.n_shared * (uint32_t)GW; i += gridDim.x * TPB)
        Tw[(size_t)(p.zrow + 1) * GW + i] = p.d * x0 / (double)p.sh_deg[i / GW];
    const size_t n_el = ((size_t)p.sl_nd + p.sl_d) * GW;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_el; i += (size_t)gridDim.x * TPB) {
        const uint32_t lrow = (uint32_t)(i / GW);
        const bool real = lrow < p.sl_nd ? lrow < p.cnt_nd : (lrow - p.sl_nd) < p.cnt_d;
        p.x[i] = real ? x0 : 0.0;
        if (lrow < p.sl_nd) {
            double c = 0.0;
            if (real) c = p.d * x0 / (double)p.outdeg[lrow];
            if ((p.world == 1 || lrow + 2 < p.sl_nd) && lrow < p.tab_rows) Tw[i] = c;   // world>1: last two rows are the tail
            csum += c;
        }
    }
    block_reduce_and_publish<GW>(p, 0.0, csum, Tw, true);
}

// world>1: after the all-gather, combine the per-rank tails (rank order) and apply the stop rule
template <int GW>
__global__ void k_pr_finalize(PrParams p, const double* __restrict__ table, int is_begin) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!is_begin && p.ctl->n_active == 0) return;
    double dl[MAXK], cs[MAXK];
    for (int k = 0; k < MAXK; k++) { dl[k] = 0.0; cs[k] = 0.0; }
    for (int r = 0; r < p.world; r++) {
        const size_t base = ((size_t)r * p.sl_nd + (p.sl_nd - 2)) * GW;
        for (int k = 0; k < GW; k++) {
            cs[k] += table[base + k];
            dl[k] += table[base + GW + k];
        }
    }
    finalize_ctl(p, dl, cs, is_begin != 0);
}

template <int GW>
__global__ void k_pr_read(const double* __restrict__ x, const PrCtl* __restrict__ ctl, const uint32_t* __restrict__ old_id,
                          uint32_t sl_nd, uint32_t cnt_nd, uint32_t pos_nd, uint32_t sl_d, uint32_t cnt_d, uint32_t pos_d,
                          uint64_t id0_nd, uint64_t id0_d, int k_topics, uint64_t out_stride,
                          int by_original_id, uint32_t* __restrict__ ids_out, double* __restrict__ out,
                          const uint32_t* __restrict__ memb, uint32_t ts_mask) {
    const size_t n_rows = (size_t)cnt_nd + cnt_d;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t lrow = i < cnt_nd ? (uint32_t)i : sl_nd + (uint32_t)(i - cnt_nd);
    const uint64_t iid = lrow < sl_nd ? id0_nd + lrow : id0_d + (lrow - sl_nd);
    const uint32_t orig = old_id[iid];
    const size_t o = by_original_id ? (size_t)orig : i;
    if (ids_out) ids_out[i] = orig;
    // rows without in-edges are not stored: they all hold ctl->xz
    const bool zero = lrow < sl_nd ? lrow >= pos_nd : (lrow - sl_nd) >= pos_d;
    const uint32_t mb = memb ? memb[lrow] & ts_mask : 0u;     // inside a topic's teleport set: the zero rows' other shared value
    for (int k = 0; k < k_topics; k++)
        out[(size_t)k * out_stride + o] = zero ? (((mb >> k) & 1u) ? ctl->xz_in[k] : ctl->xz[k]) : x[(size_t)lrow * GW + k];
}

// ---- topic-sensitive teleport (opt-in): sets -> per-row membership bits of this rank's rows ------------------------
__global__ void k_pr_memb(const uint64_t* __restrict__ set_ptr, const uint32_t* __restrict__ set_nodes, int k_topics, uint64_t n_nodes,
                          const uint32_t* __restrict__ new_id, uint64_t nd_int, uint32_t sl_nd, uint32_t sl_d, int rank,
                          uint32_t* __restrict__ memb, uint32_t* __restrict__ seen, uint32_t* __restrict__ err) {
    const uint64_t total = set_ptr[k_topics];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        int k = 0;
        while (k + 1 < k_topics && set_ptr[k + 1] <= i) k++;
        const uint32_t v = set_nodes[i];
        if ((uint64_t)v >= n_nodes) { atomicOr(err, 1u); continue; }
        // |set_k| comes from set_ptr, membership is one bit per node: a node listed twice would get less than its share.
        // Checked over ALL nodes (not only this rank's rows) so that every rank of a sharded graph takes the same decision.
        if (atomicOr(&seen[v], 1u << k) & (1u << k)) { atomicOr(err, 2u); continue; }
        const uint64_t iid = new_id[v];
        uint32_t lrow;
        int owner;
        if (iid < nd_int) { owner = (int)(iid / sl_nd); lrow = (uint32_t)(iid % sl_nd); }
        else { owner = (int)((iid - nd_int) / sl_d); lrow = sl_nd + (uint32_t)((iid - nd_int) % sl_d); }
        if (owner == rank) atomicOr(&memb[lrow], 1u << k);
    }
}
// members among the rows without in-edges (their L1 change is counted, not streamed)
__global__ void k_pr_memb_zero_count(const uint32_t* __restrict__ memb, uint32_t sl_nd, uint32_t cnt_nd, uint32_t pos_nd, uint32_t cnt_d,
                                     uint32_t pos_d, int k_topics, unsigned long long* __restrict__ cnt) {
    const uint32_t z_nd = cnt_nd - pos_nd, n_zero = z_nd + (cnt_d - pos_d);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_zero; i += gridDim.x * blockDim.x) {
        const uint32_t lrow = i < z_nd ? pos_nd + i : sl_nd + pos_d + (i - z_nd);
        const uint32_t mb = memb[lrow];
        for (int k = 0; k < k_topics; k++)
            if ((mb >> k) & 1u) atomicAdd(&cnt[k], 1ull);
    }
}

// ---- diagnostic: the ceiling of the sweep's access pattern (ss_pr_probe) -----------------------------------------
// Gather-only pass over THIS graph's in-edge stream with the sweep's own load shape (one coalesced 64-byte index
// load per lane group, 16 independent whole-row gathers in flight) and nothing else: no row ends, no rank read or
// write, no contribution write, no reductions.  mode 0 = the real index stream, 1 = indices hashed to uniformly
// random rows (no hub reuse), 2 = consecutive rows (a streamed table).  Each lane group keeps one running sum and
// stores it once, so the loads cannot be dropped.
// POL (experiments with the cache policy of the gathers): 0 default, 1 all non-temporal, 2 all sc1 (agent-scope atomic
// load), 3 rows below `hot` default / others non-temporal, 4 rows below `hot` default / others sc1
template <int GW, int POL>
__global__ __launch_bounds__(TPB) void k_pr_probe(const double* __restrict__ T, const uint32_t* __restrict__ in_src, size_t n_edges,
                                                  uint32_t n_rows, int mode, double* __restrict__ sink, uint32_t hot) {
    if constexpr (GW >= 8) {
        constexpr int NSLOT = 64 / GW;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int t = lane % GW, slot = lane / GW, gbase = lane - t;
        const size_t groups = (size_t)gridDim.x * WAVES * NSLOT;
        const size_t gi = ((size_t)blockIdx.x * WAVES + wave) * NSLOT + slot;
        // contiguous span of 16-edge chunks per lane group
        const size_t n_chunks = n_edges / CH;
        const size_t per = (n_chunks + groups - 1) / groups;
        size_t c = min(gi * per, n_chunks);
        const size_t c_hi = min(c + per, n_chunks);
        double acc = 0.0;
        for (; c < c_hi; c++) {
            constexpr int R = CH / GW;
            uint32_t src[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const size_t e = c * CH + (size_t)(r * GW + t);
                uint32_t v = NT_LOAD(&in_src[e]) & SRC_MASK;
                if (mode == 1) v = (uint32_t)(((uint64_t)(v * 2654435761u + (uint32_t)e * 40503u) * n_rows) >> 32);
                if (mode == 2) v = (uint32_t)(e % n_rows);
                src[r] = v;
            }
            double v[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const uint32_t sj = (uint32_t)__shfl((int)src[j / GW], gbase + (j % GW), 64);
                const double* a = &T[(size_t)sj * GW + t];
                if constexpr (POL == 0) v[j] = *a;
                else if constexpr (POL == 1) v[j] = __builtin_nontemporal_load(a);
                else if constexpr (POL == 2) v[j] = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if constexpr (POL == 3) v[j] = sj < hot ? *a : __builtin_nontemporal_load(a);
                else v[j] = sj < hot ? *a : __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int j = 0; j < CH; j++) acc += v[j];
        }
        sink[((size_t)blockIdx.x * TPB + threadIdx.x)] = acc;
    }
}

}  // namespace

namespace {

// Which sweep kernel a state runs, its lane-group width, and whether ss_pr_step's sweeps share one launch: decided here, once.
void pick_kernel(const ss_ctx* ctx, ss_pr* pr, int k, uint64_t table_rows) {
    // K = 3, 4 run the wave-item sweep padded to 8 topics (measured on the 10M/50M R-MAT at K=4: 0.77 ms against 0.94 ms
    // for the 4-wide block-item kernel).  K <= 2: the wave-item kernel for one or two topics, k_pr_sweep_n, unpadded (round 4).
    // Before it (option "pr.narrow_wave" = 0): padded to 8 when the padded table stays cache-resident (<= 64 MB of 64-byte
    // rows: the padding costs no HBM traffic then; 2^20 nodes / 5M edges, K=1: 0.074 ms), else the block-item kernel k_pr_step
    // (10M/50M, K=1: 0.55 ms against 0.79 ms padded).  "pr.force_narrow": always k_pr_step (tests reach it on small graphs).
    const bool force_narrow = ctx->opt("pr.force_narrow", 0) != 0, narrow_wave = ctx->opt("pr.narrow_wave", 1) != 0;
    if (k > 2) {
        pr->kernel = PR_SWEEP;
        pr->gw = k <= 8 ? 8 : 16;
    } else if (force_narrow) {
        pr->kernel = PR_STEP;
        pr->gw = k;
    } else if (narrow_wave) {
        pr->kernel = PR_SWEEP_N;
        pr->gw = k;
    } else if (table_rows * 64 <= (64ull << 20)) {
        pr->kernel = PR_SWEEP;
        pr->gw = 8;
    } else {
        pr->kernel = PR_STEP;
        pr->gw = k;
    }
    pr->nwave = pr->kernel == PR_SWEEP_N;
    // Several sweeps per launch (k_pr_multi_n), OPT-IN ("pr.persistent" = 1: write-through hand-offs, 2: release / acquire fences): one
    // rank, the reference's uniform teleport, K <= 2 on the wave-item kernel.  The blocks wait for each other between two sweeps, so ALL
    // of them must be resident: half of what the occupancy query admits per CU, at most "pr.persistent_blocks" (default 4; grid_for).
    // Measured and therefore off by default (round 5, config 2: 2^20 nodes / 5M edges, K = 1): 0.054 ms per sweep with one launch per
    // sweep against 0.113 (write-through) / 0.152 (fences) inside one launch at 4 blocks per CU, 0.075 / 0.094 at 2, 0.078 / 0.082 at 1 —
    // the wait costs ~25 us per 256 resident blocks, far more than the 33 us an empty launch of this sweep costs in all; 10M / 50M:
    // 0.38 against 0.51 ms.  Results are bit-identical in every mode (test_sweeps_inside_one_launch_are_bit_identical).
    const int64_t want = ctx->opt("pr.persistent", 0);
    pr->persist_mode = want == 2 ? 2 : 1;
    pr->persist = pr->nwave && pr->g->world == 1 && !ctx->opt("pr.affine", 0) && want > 0;
}

template <int GW>
void launch_begin(ss_pr* pr, hipStream_t st, unsigned nb) {
    hipLaunchKernelGGL(k_pr_begin<GW>, dim3(nb), dim3(TPB), 0, st, pr->prm);
}
template <int GW>
void launch_finalize(ss_pr* pr, hipStream_t st, int is_begin) {
    hipLaunchKernelGGL(k_pr_finalize<GW>, dim3(1), dim3(64), 0, st, pr->prm, (const double*)pr->tab0.p, is_begin);
}
// The same by ORIGINAL id on an unsharded graph (ss_pr_read: rank_out[k][v]): one thread per original node v.  k_pr_read above
// walks the rows in internal order and scatters 8-byte values into K topic planes at random original ids (every store a partial
// line: 3.0 ms for the 1.28 GB of config 4, 3.05 GB fetched); here the WRITES are the coalesced side — for every topic the 64
// lanes of a wave store 64 consecutive doubles — and the reads gather whole rows (GW doubles, one 128-byte line at GW = 16).
template <int GW>
__global__ __launch_bounds__(TPB) void k_pr_read_orig(const double* __restrict__ x, const PrCtl* __restrict__ ctl, const uint32_t* __restrict__ new_id,
                                                      uint64_t n, uint32_t sl_nd, uint32_t pos_nd, uint32_t pos_d, int k_topics,
                                                      double* __restrict__ out, const uint32_t* __restrict__ memb, uint32_t ts_mask) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t lrow = new_id[v];                  // world == 1: internal id == local row
    const bool zero = lrow < sl_nd ? lrow >= pos_nd : (lrow - sl_nd) >= pos_d;
    double r[GW];
    if (!zero) {
        if constexpr (GW >= 2) {
            const double2* const row = reinterpret_cast<const double2*>(x + (size_t)lrow * GW);
#pragma unroll
            for (int j = 0; j < GW / 2; j++) { const double2 t = row[j]; r[2 * j] = t.x; r[2 * j + 1] = t.y; }
        } else {
            r[0] = x[lrow];
        }
    } else {
        const uint32_t mb = memb ? memb[lrow] & ts_mask : 0u;
#pragma unroll
        for (int k = 0; k < GW; k++) r[k] = ((mb >> k) & 1u) ? ctl->xz_in[k] : ctl->xz[k];
    }
#pragma unroll
    for (int k = 0; k < GW; k++)
        if (k < k_topics) out[(size_t)k * n + v] = r[k];
}

template <int GW>
void launch_read(ss_pr* pr, hipStream_t st, int by_orig, uint64_t stride, uint32_t* ids, double* out) {
    const ss_graph* g = pr->g;
    const size_t n_rows = (size_t)g->cnt_nd + g->cnt_d;
    if (!n_rows) return;
    if (by_orig && g->world == 1 && !ids && stride == g->n) {
        hipLaunchKernelGGL(k_pr_read_orig<GW>, dim3(ss::div_up(g->n, TPB)), dim3(TPB), 0, st, (const double*)pr->x.p, (const PrCtl*)pr->ctl.p,
                           (const uint32_t*)g->new_id.p, g->n, g->sl_nd, pr->prm.pos_nd, pr->prm.pos_d, pr->k, out, pr->prm.memb, pr->prm.ts_mask);
        return;
    }
    hipLaunchKernelGGL(k_pr_read<GW>, dim3(ss::div_up(n_rows, TPB)), dim3(TPB), 0, st, (const double*)pr->x.p,
                       (const PrCtl*)pr->ctl.p, (const uint32_t*)g->old_id.p, g->sl_nd, g->cnt_nd, pr->prm.pos_nd, g->sl_d, g->cnt_d,
                       pr->prm.pos_d,
                       (uint64_t)g->rank * g->sl_nd, g->nd_int + (uint64_t)g->rank * g->sl_d, pr->k, stride, by_orig, ids, out,
                       pr->prm.memb, pr->prm.ts_mask);
}

// the small kernels (begin, finalize, read) exist for every lane-group width
#define SS_GW_DISPATCH(gw, fn, ...)          \
    switch (gw) {                            \
        case 1: fn<1>(__VA_ARGS__); break;   \
        case 2: fn<2>(__VA_ARGS__); break;   \
        case 8: fn<8>(__VA_ARGS__); break;   \
        default: fn<16>(__VA_ARGS__); break; \
    }

}  // namespace

namespace ss {
unsigned begin_blocks(const ss_pr* pr) { return std::max(1u, std::min(2048u, ss::div_up((size_t)pr->g->n_local() * pr->gw, TPB))); }
void pr_launch_begin(ss_pr* pr, hipStream_t st, unsigned nb) { SS_GW_DISPATCH(pr->gw, launch_begin, pr, st, nb); }
void pr_launch_step(ss_pr* pr, hipStream_t st, bool lean) {
    switch (pr->kernel) {
        case PR_STEP: pr_step_launch(pr, st); break;
        case PR_SWEEP: pr_sweep_launch(pr, st, lean); break;
        case PR_SWEEP_N: pr_sweep_n_launch(pr, st); break;
    }
}
void pr_launch_finalize(ss_pr* pr, hipStream_t st, int is_begin) { SS_GW_DISPATCH(pr->gw, launch_finalize, pr, st, is_begin); }
}  // namespace ss

namespace {

// ---- ss_pr_create's steps ---------------------------------------------------------------------------------------------------
// What the context's "pr.*" options say about the plan: the one place they are read.  The defaults depend on the kernel and on
// the graph's size.
PlanOptions plan_options(const ss_ctx* ctx, const ss_pr* pr, size_t n_local) {
    const bool small = n_local <= ((size_t)4 << 20);
    PlanOptions o;
    o.t_quad = (uint32_t)ctx->opt("pr.t_quad", pr->nwave ? 256 : 128);
    // item granularity (measured, sweep ms at 2 / 4 / 8 / 16 / 32 turns per V_DEG item): 2^20 nodes, 5M edges, K=1: 0.078 / 0.077 / 0.096 /
    // 0.102 / 0.158; 10M nodes, 50M edges, K=16: 0.973 / 0.968 / 0.968 / 0.988 / 1.013 — a small graph gives every wave ~20 turns in all,
    // and the deal can only balance what the items let it; the large one pays for more items in the deal itself (host time)
    o.item_turns = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(64, ctx->opt("pr.item_turns", pr->nwave ? (small ? 1 : 4) : (small ? 4 : 8))));
    // How many waves: k_pr_sweep gives every wave at least one item; k_pr_sweep_n at least "pr.items_per_wave" (default 4: 0.0537 / 0.0531 / 0.0522 / 0.0483 / 0.0523 ms at 1 / 2 / 3 / 4 / 6) — on a small
    // graph what a sweep costs is mostly per WAVE (launch, control-block and offset reads, the hand-in of the partial sums), and a wave
    // with a single pass of 64 rows is all overhead.  Config 2 (2^20 nodes / 5M edges, K = 1), ms per sweep by resident blocks per CU:
    // 8: 0.0533, 6: 0.0513, 4: 0.0485, 3: 0.0461, 2: 0.0468.  [Built, measured, removed: the same waves in 1024-thread blocks (a quarter
    // of the arrivals at the hand-in): 0.067 against 0.054 — sixteen waves wait for their slowest at every workgroup barrier.]
    o.items_per_wave = pr->nwave ? (size_t)std::max<int64_t>(1, ctx->opt("pr.items_per_wave", 4)) : 1;
    o.deal_snake = ctx->opt("pr.deal_snake", PlanOptions::AUTO);
    o.deal_global = ctx->opt("pr.deal_global", pr->nwave && pr->gw == 1 ? 1 : 2);
    o.blocks_per_cu = ctx->opt("pr.blocks_per_cu", PlanOptions::AUTO);
    o.class_order = ctx->opt("pr.class_order", 235401);
    o.n_class_order = ctx->opt("pr.n_class_order", small ? 2310 : 123);
    o.stagger = ctx->opt("pr.stagger", 0);
    return o;
}

// blocks per CU the runtime admits of a sweep kernel: `row` = the state's PrKernel, or OCC_MULTI_N for k_pr_multi_n (gw = 1, 2)
// (the occupancy query is a runtime call of ~0.3 ms: asked once per kernel, width and process)
constexpr int OCC_MULTI_N = 3;
int blocks_per_cu(int row, int gw) {
    static std::mutex occ_mu;
    static int occ_cache[4][MAXK + 1] = {};
    std::lock_guard<std::mutex> lk_occ(occ_mu);
    int& occ = occ_cache[row][gw];
    if (!occ) {
        int per_cu = 0;
        switch (row) {
            case PR_STEP: per_cu = ss::pr_step_occupancy(gw); break;
            case PR_SWEEP: per_cu = ss::pr_sweep_occupancy(gw); break;
            case PR_SWEEP_N: per_cu = ss::pr_sweep_n_occupancy(gw); break;
            default: per_cu = ss::pr_multi_n_occupancy(gw); break;
        }
        occ = std::max(per_cu, 1);
    }
    return occ;
}
// The grid: persistent, each block (k_pr_step) or wave (the wave-item kernels) walks the work table round-robin: k_pr_step: 8 blocks
// per CU at most; wave items: exactly the waves the chip holds at once (per_cu: blocks_per_cu of the state's kernel).
unsigned grid_for(const ss_ctx* ctx, const ss_pr* pr, const PlanOptions& opt, int per_cu, size_t n_items) {
    per_cu = (int)std::max<int64_t>(1, opt.blocks_per_cu == PlanOptions::AUTO ? per_cu : opt.blocks_per_cu);
    if (pr->persist) {
        // what the runtime admits of k_pr_multi_n itself, less two: the query answers one block per CU too many for kernels with
        // 97-112 SGPRs (MI355X_MICROARCH.md, residency), and a block that is not resident would be waited for in vain
        const int admit = std::max(1, blocks_per_cu(OCC_MULTI_N, pr->gw) - 2);
        per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(admit, std::max(1, per_cu / 2)), ctx->opt("pr.persistent_blocks", 4)));
    }
    return pr->kernel != PR_STEP ? (unsigned)std::min<size_t>(std::max<size_t>(1, ss::div_up(n_items, (size_t)WAVES * opt.items_per_wave)), (size_t)ctx->cu_count * per_cu)
                                 : (unsigned)std::min<size_t>(n_items, (size_t)ctx->cu_count * 8);
}

void fill_params(ss_pr* pr, const Cut& cut, const PlanOptions& opt, double damping, double eps, int32_t max_iter, int32_t k_topics) {
    const ss_graph* g = pr->g;
    PrParams& p = pr->prm;
    p.in_ptr = g->in_ptr.p;
    p.in_src = g->in_src.p;
    p.outdeg = g->outdeg.p;
    p.x = pr->x.p;
    if (g->world == 1) {
        // sweep s reads tab[s&1], writes tab[(s&1)^1]; begin writes tab_wr[1] = tab0
        p.tab_rd[0] = pr->tab0.p; p.tab_wr[0] = pr->tab1.p;
        p.tab_rd[1] = pr->tab1.p; p.tab_wr[1] = pr->tab0.p;
    } else {
        p.tab_rd[0] = p.tab_rd[1] = pr->tab0.p;
        p.tab_wr[0] = p.tab_wr[1] = pr->send.p;
    }
    p.work = pr->work.p;
    p.partials = pr->partials.p;
    p.segpart = pr->segpart.p;
    p.rowticket = pr->rowticket.p;
    p.hubsum = pr->hubsum.p;
    p.nmulti = cut.nmulti;
    p.ctl = pr->ctl.p;
    p.x0 = pr->x0.p;
    p.d = damping;
    p.teleport = 1.0 - damping;                       // pagerank.go:90
    p.eps = eps;
    p.tele_n = p.teleport * (double)g->n;             // pagerank.go:112
    p.max_iter = max_iter;
    p.k_topics = k_topics;
    p.world = g->world;
    p.sl_nd = g->sl_nd;
    p.cnt_nd = g->cnt_nd;
    p.sl_d = g->sl_d;
    p.cnt_d = g->cnt_d;
    p.seg_edges = cut.seg_edges;
    p.n_items = (uint32_t)cut.items.size();
    p.pos_nd = cut.pos_nd;
    p.pos_d = cut.pos_d;
    p.zrow = (uint32_t)g->nd_int;
    p.tab_rows = g->sl_nd;
    p.woff = pr->woff.p;
    p.stagger_div = opt.stagger != 0 ? (uint32_t)std::max(g->ctx->cu_count, 1) : 0u;
    p.stagger_code = opt.stagger >= 10 ? (uint32_t)(opt.stagger - 10) : 0u;
    p.class_order = pack_class_order(opt.class_order);
    p.n_order = pack_n_order(opt.n_class_order);
    p.woff_lean = pr->lean ? pr->woff_lean.p : nullptr;
}

// pr.trace: 64-bit FNV-1a hashes of the plan (the host work table as uploaded, the per-wave offsets, the scalar fields of PrParams): two
// builds that plan alike print the same line
uint64_t fnv1a(const void* q, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char* b = static_cast<const unsigned char*>(q);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
void trace_plan(const ss_pr* pr, const std::vector<WorkItem>& work, const std::vector<uint32_t>& woff) {
    const PrParams& p = pr->prm;
    const double sd[] = {p.d, p.teleport, p.eps, p.tele_n};
    const uint32_t su[] = {(uint32_t)p.max_iter, (uint32_t)p.k_topics, (uint32_t)p.world, p.sl_nd, p.cnt_nd, p.sl_d, p.cnt_d, p.seg_edges, p.n_items,
                           p.pos_nd, p.pos_d, p.ts_mask, p.zrow, p.stagger_div, p.stagger_code, p.class_order, p.n_order};
    fprintf(stderr, "[pr trace] plan: work %016llx (%zu items)  woff %016llx  params %016llx  nblocks %u\n",
            (unsigned long long)fnv1a(work.data(), work.size() * sizeof(WorkItem)), work.size(),
            (unsigned long long)fnv1a(woff.data(), woff.size() * sizeof(uint32_t)),
            (unsigned long long)fnv1a(su, sizeof(su), fnv1a(sd, sizeof(sd))), pr->nblocks);
}

// The contribution table(s) of a state, zeroed: `rows` rows including the all-zero row k_pr_sweep's unused slots gather from (never
// written: the exchange and the sweeps stop in front of it).
int32_t alloc_tables(ss_pr* pr, hipStream_t st, size_t rows) {
    const ss_graph* g = pr->g;
    ss_ctx* ctx = g->ctx;
    const size_t GW = (size_t)pr->gw;
    SS_HIP(ctx, pr->tab0.alloc(rows * GW));
    SS_HIP(ctx, hipMemsetAsync(pr->tab0.p, 0, std::max<size_t>(pr->tab0.bytes(), 8), st));
    if (g->world == 1) {
        SS_HIP(ctx, pr->tab1.alloc(rows * GW));
        SS_HIP(ctx, hipMemsetAsync(pr->tab1.p, 0, std::max<size_t>(pr->tab1.bytes(), 8), st));
    } else {
        SS_HIP(ctx, pr->send.alloc((size_t)g->sl_nd * GW));
        SS_HIP(ctx, hipMemsetAsync(pr->send.p, 0, std::max<size_t>(pr->send.bytes(), 8), st));
    }
    return SS_OK;
}
// A state with shared rows back to the full table and the graph's own index stream (before ss_pr_begin: nothing is in the tables yet).
int32_t unshare_rows(ss_pr* pr, hipStream_t st) {
    if (!pr->prm.share) return SS_OK;
    const ss_graph* g = pr->g;
    SS_HIP(g->ctx, hipStreamSynchronize(st));
    SS_TRY(alloc_tables(pr, st, (size_t)g->nd_int + 1));
    pr->src_shared.release();
    pr->sh_deg.release();
    PrParams& p = pr->prm;
    p.tab_rd[0] = pr->tab0.p; p.tab_wr[0] = pr->tab1.p;
    p.tab_rd[1] = pr->tab1.p; p.tab_wr[1] = pr->tab0.p;
    p.in_src = g->in_src.p;
    p.sh_deg = nullptr;
    p.n_shared = 0;
    p.share = 0;
    p.zrow = (uint32_t)g->nd_int;
    p.tab_rows = g->sl_nd;
    return SS_OK;
}

#ifdef SS_PR_WAVETIME
// variant build: the modelled load of every wave, in all and per class (tools/pr_wavetime.py)
void dump_wave_loads(const Cut& cut, const std::vector<double>& cost, const std::vector<uint32_t>& owner, uint32_t nw) {
    FILE* f = open_dump("pr_load.csv");
    if (!f) return;
    std::vector<double> wl(nw, 0.0), wcls((size_t)nw * 6, 0.0);
    for (size_t i = 0; i < cut.items.size(); i++) {
        int kc = 0; while (kc < 5 && i >= cut.vbeg[kc + 1]) kc++;
        wl[owner[i]] += cost[i]; wcls[(size_t)owner[i] * 6 + kc] += cost[i];
    }
    fprintf(f, "wave,load,c0,c1,c2,c3,c4,c5\n");
    for (uint32_t w = 0; w < nw; w++) fprintf(f, "%u,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f\n", w, wl[w], wcls[(size_t)w * 6], wcls[(size_t)w * 6 + 1], wcls[(size_t)w * 6 + 2], wcls[(size_t)w * 6 + 3], wcls[(size_t)w * 6 + 4], wcls[(size_t)w * 6 + 5]);
    fclose(f);
}
#endif

}  // namespace

extern "C" {

int32_t ss_pr_create(ss_graph* g, double damping, double eps, int32_t max_iter, int32_t k_topics,
                     const int32_t* n_topic, ss_pr** out) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out) return ctx->fail(SS_ERR_INVALID, "ss_pr_create: out is NULL");
    *out = nullptr;
    if (k_topics < 1 || !n_topic) return ctx->fail(SS_ERR_INVALID, "ss_pr_create: k_topics < 1 or n_topic NULL");
    if (k_topics > MAXK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_pr_create: k_topics %d > %d per state (ss_pagerank_run splits larger K)", k_topics, MAXK);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    ss_pr* pr = new (std::nothrow) ss_pr();
    if (!pr) return ctx->fail(SS_ERR_OOM, "ss_pr_create: host OOM");
    std::unique_ptr<ss_pr> guard(pr);
    pr->g = g;
    pr->k = k_topics;
    pick_kernel(ctx, pr, k_topics, g->nd_int);
    const int GW = pr->gw;
    const bool vitems = pr->kernel != PR_STEP;         // wave-owned items (k_pr_sweep / k_pr_sweep_n); otherwise k_pr_step's block items
    const int GI = pr->nwave ? 8 : GW;                 // lane-group width the ITEMS are cut for
    const size_t n_local = g->n_local();
    if (((uint64_t)g->nd_int + 1) * GW * 8 >= (1ull << 32))
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_pr_create: contribution table of %llu rows x %d topics exceeds 4 GiB (shard the graph over more ranks)",
                         (unsigned long long)g->nd_int, GW);

    const bool trace = ctx->opt("pr.trace", 0) != 0;
    auto t_now = [] { return std::chrono::steady_clock::now(); };
    auto t_ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    // the large tables first: the device zeroes them (gigabytes at config 4) while the host builds and deals the work items below
    SS_HIP(ctx, pr->x.alloc(n_local * GW));
    // Shared rows for the edge-less sources (option "pr.share_zero_rows", default on): a state on k_pr_sweep<GW, false> — one rank, not
    // the two-vector form; teleport sets arrive later and take the state back to the full table (unshare_rows).  The table's size is
    // then known only behind the plan (the out-degrees of the rows without in-edges come back from the device under the deal).
    bool share = GW >= 8 && g->world == 1 && ctx->opt("pr.affine", 0) == 0 && ctx->opt("pr.share_zero_rows", 1) != 0;
    if (!share) SS_TRY(alloc_tables(pr, st, (size_t)g->nd_int + 1));

    // the plan (pr_plan.hpp): rows cut into items, the grid, and for the wave-item kernels the items dealt to the grid's waves — the
    // items' turn counts come from the sorted in-degrees the graph keeps on the host, their edge ranges are filled in on the device
    // (k_pr_item_ranges)
    const auto tc0 = t_now();
    const PlanOptions opt = plan_options(ctx, pr, n_local);
    Cut cut = cut_items(g->h_indeg_nd, g->h_indeg_d, g->sl_nd, GI, pr->nwave, opt);
    // (share: the tail's out-degrees travel to pinned host memory while the items are dealt; no tail, nothing to share)
    const uint32_t n_tail = g->cnt_nd - cut.pos_nd;
    struct PinGuard { ss_ctx* c; void* p = nullptr; size_t cap = 0; ~PinGuard() { c->pin_free(p, cap); } } tail_od{ctx};
    if (share && n_tail == 0) {
        share = false;
        SS_TRY(alloc_tables(pr, st, (size_t)g->nd_int + 1));
    }
    if (share) {
        tail_od.p = ctx->pin_alloc((size_t)n_tail * sizeof(uint32_t), &tail_od.cap);
        if (!tail_od.p) return ctx->fail(SS_ERR_OOM, "ss_pr_create: no pinned host memory for %u out-degrees", n_tail);
        SS_HIP(ctx, hipMemcpyAsync(tail_od.p, g->outdeg.p + cut.pos_nd, (size_t)n_tail * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    const auto tc1 = t_now();
    const int per_cu = blocks_per_cu(pr->kernel, GW);
    const auto tc1a = t_now();
    pr->nblocks = grid_for(ctx, pr, opt, per_cu, cut.items.size());
    static const std::vector<uint32_t> no_woff;
    const std::vector<uint32_t>* woff = &no_woff;
    if (vitems) {
        const uint32_t nw = pr->nblocks * WAVES;
        const auto td0 = t_now();
        const std::vector<double>& cost = item_costs(cut, g->h_indeg_nd, g->h_indeg_d, g->sl_nd, GI, pr->nwave);
        const auto td0a = t_now();
        std::vector<uint32_t>& owner = deal_items(cut, cost, nw, pr->nwave, opt);
#ifdef SS_PR_WAVETIME
        dump_wave_loads(cut, cost, owner, nw);
#endif
        const auto td1 = t_now();
        if (trace) fprintf(stderr, "[pr trace]   deal: occupancy query %.2f ms, costs %.3f ms, owners %.3f ms\n", t_ms(tc1, tc1a), t_ms(td0, td0a), t_ms(td0a, td1));
        woff = &place_items(cut, owner, nw);
        if (trace) fprintf(stderr, "[pr trace]   deal: placement %.3f ms\n", t_ms(td1, t_now()));
    }
    const std::vector<WorkItem>& items = cut.items;
    // The lean walk (option "pr.lean_sweeps", default on): a state on k_pr_sweep, one rank, not the two-vector form.  Whether a sweep
    // runs lean is decided per launch (ss::pr_step); its items stand behind the others in the work table.
    pr->lean = pr->kernel == PR_SWEEP && g->world == 1 && ctx->opt("pr.affine", 0) == 0 && ctx->opt("pr.lean_sweeps", 1) != 0;
    static const std::vector<WorkItem> no_items;
    const std::vector<WorkItem>* lean_items = &no_items;
    const std::vector<uint32_t>* lean_woff = &no_woff;
    if (pr->lean) {
        const auto tl0 = t_now();
        const LeanPlan lp = plan_lean_items(items, *woff, pr->nblocks * WAVES, g->sl_nd, (uint32_t)items.size());   // (behind the full table)
        lean_items = &lp.items;
        lean_woff = &lp.woff;
        if (trace) fprintf(stderr, "[pr trace]   lean walk: %zu of %zu items, %.3f ms\n", lp.items.size() - 2, items.size() - 2, t_ms(tl0, t_now()));
    }

    // the graph's build temporaries (ss_graph::late_free): its last kernels ran under the host work above
    g->settle();
    const auto tc2 = t_now();
    SharedRows sh;
    if (share) {
        SS_HIP(ctx, hipStreamSynchronize(st));
        const auto ts0 = t_now();
        sh = plan_shared_rows(static_cast<const uint32_t*>(tail_od.p), n_tail, cut.pos_nd);
        const auto ts1 = t_now();
        SS_TRY(alloc_tables(pr, st, (size_t)sh.table_rows));
        SS_HIP(ctx, pr->sh_deg.alloc(sh.deg.size()));
        SS_HIP(ctx, hipMemcpyAsync(pr->sh_deg.p, sh.deg.data(), sh.deg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        SS_HIP(ctx, pr->src_shared.alloc(g->e_local));
        if (g->e_local)
            hipLaunchKernelGGL(k_pr_remap_src, dim3((unsigned)std::min<uint64_t>(ss::div_up(g->e_local, TPB), (uint64_t)ctx->cu_count * 16)), dim3(TPB), 0, st,
                               (const uint32_t*)g->in_src.p, pr->src_shared.p, (size_t)g->e_local, cut.pos_nd, g->cnt_nd, (const uint32_t*)g->outdeg.p,
                               (const uint32_t*)pr->sh_deg.p, (uint32_t)sh.deg.size(), sh.zrow);
        if (trace) fprintf(stderr, "[pr trace]   shared rows: %u rows without in-edges -> %zu shared rows (host %.3f ms), table %llu rows\n", n_tail, sh.deg.size(),
                           t_ms(ts0, ts1), (unsigned long long)sh.table_rows);
    }
    SS_HIP(ctx, pr->partials.alloc(((size_t)std::max(pr->nblocks, ss::begin_blocks(pr)) + 8) * 2 * GW));   // block rows + 8 group rows
    SS_HIP(ctx, pr->segpart.alloc((size_t)std::max(cut.nsegs, 1u) * GW));
    SS_HIP(ctx, pr->rowticket.alloc(std::max(cut.nmulti, 1u)));
    SS_HIP(ctx, pr->hubsum.alloc((size_t)std::max(cut.nmulti, 1u) * 2 * GW));
    SS_HIP(ctx, hipMemsetAsync(pr->hubsum.p, 0, pr->hubsum.bytes(), st));
    SS_HIP(ctx, hipMemsetAsync(pr->rowticket.p, 0, pr->rowticket.bytes(), st));
    SS_HIP(ctx, pr->woff.alloc(std::max<size_t>(woff->size(), 8)));
    if (!woff->empty()) SS_HIP(ctx, hipMemcpyAsync(pr->woff.p, woff->data(), woff->size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const size_t n_work = items.size() + lean_items->size();
    SS_HIP(ctx, pr->work.alloc(n_work));
    SS_HIP(ctx, hipMemcpyAsync(pr->work.p, items.data(), items.size() * sizeof(WorkItem), hipMemcpyHostToDevice, st));
    if (pr->lean) {
        SS_HIP(ctx, hipMemcpyAsync(pr->work.p + items.size(), lean_items->data(), lean_items->size() * sizeof(WorkItem), hipMemcpyHostToDevice, st));
        SS_HIP(ctx, pr->woff_lean.alloc(std::max<size_t>(lean_woff->size(), 8)));
        SS_HIP(ctx, hipMemcpyAsync(pr->woff_lean.p, lean_woff->data(), lean_woff->size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (vitems)
        hipLaunchKernelGGL(k_pr_item_ranges, dim3(ss::div_up(n_work, TPB)), dim3(TPB), 0, st, pr->work.p, (uint32_t)n_work, (const uint32_t*)g->in_ptr.p);
    SS_HIP(ctx, pr->ctl.alloc(1));
    SS_HIP(ctx, hipMemsetAsync(pr->ctl.p, 0, sizeof(PrCtl), st));
    double h_x0[MAXK];
    for (int k = 0; k < MAXK; k++) h_x0[k] = k < k_topics ? 1.0 / (double)n_topic[k] : 0.0;   // pagerank.go:104
    SS_HIP(ctx, pr->x0.alloc(MAXK));
    SS_HIP(ctx, hipMemcpyAsync(pr->x0.p, h_x0, sizeof(h_x0), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipStreamSynchronize(st));   // items / h_x0 are stack/host temporaries
    if (trace) fprintf(stderr, "[pr trace] ss_pr_create: build_work %.2f ms (%zu items), edge ranges + deal %.2f ms, alloc + upload %.2f ms\n", t_ms(tc0, tc1), items.size(), t_ms(tc1, tc2), t_ms(tc2, t_now()));
    if (trace) fprintf(stderr, "[pr trace] where the state lives: x %p  tab0 %p  tab1 %p  in_src %p  in_ptr %p  outdeg %p  work %p  woff %p\n", (void*)pr->x.p, (void*)pr->tab0.p,
                       (void*)pr->tab1.p, (void*)g->in_src.p, (void*)g->in_ptr.p, (void*)g->outdeg.p, (void*)pr->work.p, (void*)pr->woff.p);

    fill_params(pr, cut, opt, damping, eps, max_iter, k_topics);
    if (share) {
        PrParams& p = pr->prm;
        p.in_src = pr->src_shared.p;
        p.sh_deg = pr->sh_deg.p;
        p.n_shared = (uint32_t)sh.deg.size();
        p.share = 1;
        p.zrow = sh.zrow;
        p.tab_rows = cut.pos_nd;
    }
    if (trace) trace_plan(pr, items, *woff);
    g->users++;
    *out = guard.release();
    return SS_OK;
}

int32_t ss_pr_set_teleport(ss_pr* pr, const uint64_t* set_ptr, const uint32_t* set_nodes) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (pr->begun) return ctx->fail(SS_ERR_STATE, "ss_pr_set_teleport: call before ss_pr_begin");
    hipStream_t st = ctx->stream;
    PrParams& p = pr->prm;
    if (!set_ptr) {                                  // back to the reference's uniform teleport
        p.memb = nullptr; p.tin = nullptr; p.nz_in = nullptr; p.ts_mask = 0;
        return SS_OK;
    }
    const ss_graph* g = pr->g;
    const int K = pr->k;
    SS_TRY(unshare_rows(pr, st));                    // the teleport-set kernels keep a table row per row
    std::vector<uint64_t> h_ptr(K + 1);
    SS_HIP(ctx, ss::copy_in(ctx->stream, h_ptr.data(), set_ptr, (K + 1) * sizeof(uint64_t)));
    if (h_ptr[0] != 0) return ctx->fail(SS_ERR_INVALID, "ss_pr_set_teleport: set_ptr[0] != 0");
    for (int k = 0; k < K; k++)
        if (h_ptr[k + 1] < h_ptr[k]) return ctx->fail(SS_ERR_INVALID, "ss_pr_set_teleport: set_ptr not non-decreasing");
    const uint64_t total = h_ptr[K];
    if (total && !set_nodes) return ctx->fail(SS_ERR_INVALID, "ss_pr_set_teleport: set_nodes is NULL");
    double h_tin[MAXK];
    uint32_t mask = 0;
    for (int k = 0; k < MAXK; k++) {
        h_tin[k] = 0.0;
        if (k < K && h_ptr[k + 1] > h_ptr[k]) {
            mask |= 1u << k;
            h_tin[k] = p.teleport * (double)g->n / (double)(h_ptr[k + 1] - h_ptr[k]);     // the set shares the mass (1-d)*N
        }
    }
    const size_t n_local = g->n_local();
    ss::DevBuf<uint64_t> d_ptr;
    ss::DevBuf<uint32_t> d_nodes, d_err, d_seen;
    ss::DevBuf<unsigned long long> d_cnt;
    SS_HIP(ctx, d_ptr.alloc(K + 1));
    SS_HIP(ctx, d_seen.alloc(g->n));
    SS_HIP(ctx, hipMemsetAsync(d_seen.p, 0, std::max<size_t>(d_seen.bytes(), 4), st));
    SS_HIP(ctx, d_nodes.alloc(total));
    SS_HIP(ctx, d_err.alloc(1));
    SS_HIP(ctx, d_cnt.alloc(MAXK));
    SS_HIP(ctx, pr->memb.alloc(n_local));
    SS_HIP(ctx, pr->tin.alloc(MAXK));
    SS_HIP(ctx, pr->nz_in.alloc(MAXK));
    SS_HIP(ctx, hipMemcpyAsync(d_ptr.p, h_ptr.data(), (K + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (total) SS_HIP(ctx, hipMemcpyAsync(d_nodes.p, set_nodes, total * sizeof(uint32_t), hipMemcpyDefault, st));
    SS_HIP(ctx, hipMemsetAsync(pr->memb.p, 0, std::max<size_t>(pr->memb.bytes(), 4), st));
    SS_HIP(ctx, hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), st));
    SS_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, MAXK * sizeof(unsigned long long), st));
    if (total)
        hipLaunchKernelGGL(k_pr_memb, dim3(std::min<unsigned>(ss::div_up(total, TPB), 4096u)), dim3(TPB), 0, st, (const uint64_t*)d_ptr.p,
                           (const uint32_t*)d_nodes.p, K, g->n, (const uint32_t*)g->new_id.p, g->nd_int, std::max(g->sl_nd, 1u), std::max(g->sl_d, 1u),
                           g->rank, pr->memb.p, d_seen.p, d_err.p);
    const uint32_t n_zero = (g->cnt_nd - p.pos_nd) + (g->cnt_d - p.pos_d);
    if (n_zero)
        hipLaunchKernelGGL(k_pr_memb_zero_count, dim3(std::min<unsigned>(ss::div_up(n_zero, TPB), 4096u)), dim3(TPB), 0, st,
                           (const uint32_t*)pr->memb.p, g->sl_nd, g->cnt_nd, p.pos_nd, g->cnt_d, p.pos_d, K, d_cnt.p);
    SS_HIP(ctx, hipGetLastError());
    uint32_t h_err = 0;
    unsigned long long h_cnt[MAXK];
    SS_HIP(ctx, ss::fetch(ctx, st, &h_err, d_err.p, sizeof(h_err), h_cnt, d_cnt.p, sizeof(h_cnt)));
    if (h_err & 1u) return ctx->fail(SS_ERR_INVALID, "ss_pr_set_teleport: a teleport set holds a node id >= n_nodes");
    if (h_err & 2u) return ctx->fail(SS_ERR_INVALID, "ss_pr_set_teleport: a teleport set lists a node twice (the ids of a set must be distinct)");
    double h_nz[MAXK];
    for (int k = 0; k < MAXK; k++) h_nz[k] = (double)h_cnt[k];
    SS_HIP(ctx, hipMemcpyAsync(pr->tin.p, h_tin, sizeof(h_tin), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipMemcpyAsync(pr->nz_in.p, h_nz, sizeof(h_nz), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    p.memb = pr->memb.p;
    p.tin = pr->tin.p;
    p.nz_in = pr->nz_in.p;
    p.ts_mask = mask;
    return SS_OK;
}

int32_t ss_pr_destroy(ss_pr* pr) {
#ifdef SS_PR_WAVETIME
    if (pr) ss::pr_dump_wave_times(pr);
#endif

    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (!ss::device_wedged(ctx->device)) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->comm_stream);
    }
    pr->g->users--;
    delete pr;
    return SS_OK;
}

int32_t ss_pr_begin(ss_pr* pr) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (pr->need_finalize) return ctx->fail(SS_ERR_STATE, "ss_pr_begin: pending exchange/finalize");
    SS_HIP(ctx, hipMemsetAsync(&pr->ctl.p->ticket, 0, sizeof(uint32_t), ctx->stream));
    ss::pr_launch_begin(pr, ctx->stream, ss::begin_blocks(pr));
    SS_HIP(ctx, hipGetLastError());
    pr->begun = true;
    pr->sweeps_enq = 0;
    if (pr->g->world > 1) {
        pr->need_finalize = true;
        pr->finalize_is_begin = true;
    }
    return SS_OK;
}

int32_t ss_pr_step(ss_pr* pr, int32_t n_steps) {
    if (!pr) return SS_ERR_INVALID;
    return ss::pr_step(pr, n_steps, 2);           // a caller may read the ranks and the last L1 change behind every call
}

int32_t ss_pr_lean_sweeps(ss_pr* pr, int64_t* n_out) {
    if (!pr || !n_out) return SS_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(pr->g->ctx->mu);
    *n_out = pr->n_lean;
    return SS_OK;
}

}  // extern "C"

// Which sweeps of a call run lean (k_pr_sweep<GW, false, true>): only those whose rank array and L1 change nobody can see.  The state
// is in fixed-iteration mode (eps < 0: no stop rule reads the change, no topic freezes), has a lean walk (ss_pr_create: k_pr_sweep,
// one rank, "pr.lean_sweeps"), no teleport sets and not the two-vector form; the sweep is none of the call's last `full_tail` and
// none of the last two before max_iter, where the run ends.  The last sweep's L1 change needs the ranks of the sweep before it, so
// that one runs full as well (for its rank store alone; its old-rank read is the price of having two kernels, not three).
int32_t ss::pr_step(ss_pr* pr, int32_t n_steps, int32_t full_tail) {
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (!pr->begun) return ctx->fail(SS_ERR_STATE, "ss_pr_step: ss_pr_begin not called");
    if (pr->need_finalize) return ctx->fail(SS_ERR_STATE, "ss_pr_step: pending exchange/finalize");
    if (n_steps < 1) return ctx->fail(SS_ERR_INVALID, "ss_pr_step: n_steps < 1");
    if (pr->g->world > 1 && n_steps != 1) return ctx->fail(SS_ERR_INVALID, "ss_pr_step: world>1 needs an exchange after every step");
    SS_HIP(ctx, hipEventRecord(ctx->ev[0][0], ctx->stream));
    if (pr->persist && !pr->prm.memb && !pr->prm.aff) {
        ss::pr_multi_n_launch(pr, ctx->stream, (int)n_steps);   // the sweeps wait for each other inside the launch
    } else {
        const PrParams& p = pr->prm;
        const bool lean_ok = pr->lean && p.eps < 0.0 && !p.memb && !p.aff;
        for (int i = 0; i < n_steps; i++) {
            const int64_t s = pr->sweeps_enq + 1 + i;                  // this sweep's number since ss_pr_begin
            const bool lean = lean_ok && i + full_tail < n_steps && (p.max_iter <= 0 || s + 2 <= p.max_iter);
            ss::pr_launch_step(pr, ctx->stream, lean);
        }
    }
    pr->sweeps_enq += n_steps;
    SS_HIP(ctx, hipEventRecord(ctx->ev[0][1], ctx->stream));
    ctx->ev_valid[0] = true;
    SS_HIP(ctx, hipGetLastError());
    if (pr->g->world > 1) {
        pr->need_finalize = true;
        pr->finalize_is_begin = false;
    }
    return SS_OK;
}

extern "C" {

int32_t ss_pr_finalize(ss_pr* pr) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (pr->g->world == 1) return ctx->fail(SS_ERR_STATE, "ss_pr_finalize: world==1 folds the finalize into the sweep");
    if (!pr->need_finalize) return ctx->fail(SS_ERR_STATE, "ss_pr_finalize: nothing to finalize");
    ss::pr_launch_finalize(pr, ctx->stream, pr->finalize_is_begin ? 1 : 0);
    SS_HIP(ctx, hipGetLastError());
    pr->need_finalize = false;
    return SS_OK;
}

int32_t ss_pr_exchange_buffers(ss_pr* pr, void** send_dev, uint64_t* send_bytes, void** recv_dev, uint64_t* recv_bytes) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    if (pr->g->world == 1) return ctx->fail(SS_ERR_STATE, "ss_pr_exchange_buffers: world==1 has no exchange");
    if (send_dev) *send_dev = pr->send.p;
    if (send_bytes) *send_bytes = pr->send.bytes();
    if (recv_dev) *recv_dev = pr->tab0.p;
    if (recv_bytes) *recv_bytes = (uint64_t)pr->g->nd_int * pr->gw * sizeof(double);   // without the table's zero row
    return SS_OK;
}

int32_t ss_pr_exchange(ss_pr* pr, int32_t allreduce) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const ss_graph* g = pr->g;
    if (g->world == 1) return ctx->fail(SS_ERR_STATE, "ss_pr_exchange: world==1 has no exchange");
    if (!pr->need_finalize) return ctx->fail(SS_ERR_STATE, "ss_pr_exchange: nothing to exchange (call after ss_pr_begin / ss_pr_step)");
    if (!ctx->comm || ctx->comm_world != g->world || ctx->comm_rank != g->rank)
        return ctx->fail(SS_ERR_STATE, "ss_pr_exchange: the context's communicator (rank %d of %d) does not match the graph's shard (rank %d of %d)",
                         ctx->comm ? ctx->comm_rank : -1, ctx->comm ? ctx->comm_world : 0, g->rank, g->world);
    const size_t slice = (size_t)g->sl_nd * pr->gw;            // doubles per rank
    if (!allreduce && ctx->opt("pr.wire_f32", 0) != 0) {       // opt-in: float32 on the wire (pagerank_run.hip: k_wire_pack)
        SS_HIP(ctx, ss::pr_wire_alloc(pr));
        ss::pr_wire_pack(pr, ctx->stream);
        SS_TRY(ss::comm_allgather(ctx, pr->wire_send.p, pr->wire_recv.p, ss::pr_wire_floats(pr) * sizeof(float)));
        ss::pr_wire_unpack(pr, ctx->stream);
        return SS_OK;
    }
    if (!allreduce) return ss::comm_allgather(ctx, pr->send.p, pr->tab0.p, slice * sizeof(double));
    // north-star form: own slice inside a zeroed full-size table, tables summed
    SS_HIP(ctx, hipMemsetAsync(pr->tab0.p, 0, pr->tab0.bytes(), ctx->stream));
    SS_HIP(ctx, hipMemcpyAsync(pr->tab0.p + (size_t)g->rank * slice, pr->send.p, slice * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return ss::comm_allreduce_f64(ctx, pr->tab0.p, pr->tab0.p, slice * (size_t)g->world);
}

int32_t ss_pr_status(ss_pr* pr, int32_t* iters_out, int32_t* n_active, int32_t* sweeps, double* last_delta_out,
                     double* last_total_out) {
    if (!pr) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const PrCtl* hp = nullptr;
    SS_TRY(read_ctl(ctx, pr, ctx->stream, "ss_pr_status", &hp));
    const PrCtl h = *hp;
    if (h.stuck) return ctx->fail(SS_ERR_STATE, "ss_pr_status: the multi-sweep kernel gave up waiting between two sweeps (its grid of %u blocks was not resident: "
                                  "other kernels held the CUs for seconds); the state is void — set option pr.persistent = 0 and run again", pr->nblocks);
    for (int k = 0; k < pr->k; k++) {
        if (iters_out) iters_out[k] = h.iters[k];
        if (last_delta_out) last_delta_out[k] = h.delta[k];
        if (last_total_out) last_total_out[k] = h.S[k];
    }
    if (n_active) *n_active = h.n_active;
    if (sweeps) *sweeps = h.sweep;
    return SS_OK;
}

int32_t ss_pr_read_local(ss_pr* pr, uint32_t* ids_out, double* rank_out) {
    if (!pr || !rank_out) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const ss_graph* g = pr->g;
    const size_t n_rows = (size_t)g->cnt_nd + g->cnt_d;
    ss::DevBuf<uint32_t> d_ids;
    ss::DevBuf<double> d_out;
    SS_HIP(ctx, d_ids.alloc(n_rows));
    SS_HIP(ctx, d_out.alloc(n_rows * pr->k));
    SS_GW_DISPATCH(pr->gw, launch_read, pr, ctx->stream, 0, (uint64_t)n_rows, d_ids.p, d_out.p);
    SS_HIP(ctx, hipGetLastError());
    if (ids_out && n_rows) SS_HIP(ctx, hipMemcpyAsync(ids_out, d_ids.p, n_rows * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
    if (n_rows) SS_HIP(ctx, hipMemcpyAsync(rank_out, d_out.p, n_rows * pr->k * sizeof(double), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SS_OK;
}

int32_t ss_pr_read(ss_pr* pr, double* rank_out) {
    if (!pr || !rank_out) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const ss_graph* g = pr->g;
    if (g->world != 1) return ctx->fail(SS_ERR_STATE, "ss_pr_read: world>1, use ss_pr_read_local");
    // ranks wanted in device memory: written there directly (no K*N*8-byte staging buffer and copy)
    hipPointerAttribute_t pa{};
    const bool dev_out = hipPointerGetAttributes(&pa, rank_out) == hipSuccess && pa.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    ss::DevBuf<double> d_out;
    if (!dev_out) SS_HIP(ctx, d_out.alloc((size_t)g->n * pr->k));
    SS_GW_DISPATCH(pr->gw, launch_read, pr, ctx->stream, 1, (uint64_t)g->n, (uint32_t*)nullptr, dev_out ? rank_out : d_out.p);
    SS_HIP(ctx, hipGetLastError());
    if (!dev_out) SS_HIP(ctx, hipMemcpyAsync(rank_out, d_out.p, (size_t)g->n * pr->k * sizeof(double), hipMemcpyDefault, ctx->stream));
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SS_OK;
}

int32_t ss_pr_probe(ss_pr* pr, int32_t mode, int32_t n_reps, float* ms_out) {
    if (!pr || !ms_out) return SS_ERR_INVALID;
    ss_ctx* ctx = pr->g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    if (pr->gw < 8) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_pr_probe: the probe mirrors the chunked gather of the K >= 5 kernels");
    if (mode < 0 || (mode & 7) > 2 || (mode >> 3) > 4 || n_reps < 1) return ctx->fail(SS_ERR_INVALID, "ss_pr_probe: mode 0..2 (+ 8 * gather cache policy 0..4), n_reps >= 1");
    const int pol = mode >> 3;
    mode &= 7;
    const uint32_t hot = (uint32_t)ctx->opt("pr.probe_hot", 24576);
    const ss_graph* g = pr->g;
    const unsigned nb = (unsigned)ctx->cu_count * 8;
    ss::DevBuf<double> sink;
    SS_HIP(ctx, sink.alloc((size_t)nb * TPB));
    hipEvent_t e0, e1;
    SS_HIP(ctx, hipEventCreate(&e0));
    SS_HIP(ctx, hipEventCreate(&e1));
    hipStream_t st = ctx->stream;
    // (the probe walks the GRAPH's index stream over a table of nd_int rows; a state with shared rows has a shorter one: a scratch table)
    ss::DevBuf<double> full;
    if (pr->prm.share) {
        SS_HIP(ctx, full.alloc(((size_t)g->nd_int + 1) * pr->gw));
        SS_HIP(ctx, hipMemsetAsync(full.p, 0, full.bytes(), ctx->stream));
    }
    const double* T = pr->prm.share ? full.p : pr->tab0.p;
    for (int r = 0; r < n_reps + 1; r++) {
        if (r == 1) SS_HIP(ctx, hipEventRecord(e0, st));          // first launch = warm-up
#define SS_PROBE_LAUNCH(GWV, POLV) hipLaunchKernelGGL((k_pr_probe<GWV, POLV>), dim3(nb), dim3(TPB), 0, st, T, (const uint32_t*)g->in_src.p, (size_t)g->e_local, (uint32_t)g->nd_int, mode, sink.p, hot)
        if (pr->gw == 8) SS_PROBE_LAUNCH(8, 0);
        else switch (pol) {
            case 0: SS_PROBE_LAUNCH(16, 0); break;
            case 1: SS_PROBE_LAUNCH(16, 1); break;
            case 2: SS_PROBE_LAUNCH(16, 2); break;
            case 3: SS_PROBE_LAUNCH(16, 3); break;
            default: SS_PROBE_LAUNCH(16, 4); break;
        }
    }
    SS_HIP(ctx, hipEventRecord(e1, st));
    SS_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    SS_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    SS_HIP(ctx, hipGetLastError());
    *ms_out = ms / (float)n_reps;
    return SS_OK;
}

}  // extern "C"
