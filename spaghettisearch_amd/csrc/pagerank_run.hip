// pagerank_run.hip — PageRank in one call: ss_pagerank_run, ss_pagerank_run_sharded, ss_pagerank_run_group and the drivers behind them
// (the pipelined sharded power iteration, the two-vector form "pr.affine" on one rank and on shards), with the kernels only these
// drivers launch: the two-vector form's streaming kernels (k_aff_*) and float32 on the wire (k_wire_*).  The sweep itself, its
// state and the ss_pr_* stepping API the drivers are built on: pagerank.hip, pr_state.hpp.
#include "pr_state.hpp"

#include <algorithm>

namespace {

// ---- two-vector form: per-topic L1 change, stop rule, write-out ("pr.affine"; see AffCtl) ---------------------------------------
// x holds (p, q) of the rows WITH in-edges; the edge-less rows share one (p, q) per class position (ctl->xz).  A topic's rank
// of a row is (p*u + q) / (r*u + s).
constexpr int AFF_KC = 16;        // topics a thread accumulates per pass over the rows
__global__ __launch_bounds__(TPB) void k_aff_delta(const double2* __restrict__ xp, const double2* __restrict__ xn, const AffCtl* __restrict__ a,
                                                   uint32_t sl_nd, uint32_t pos_nd, uint32_t pos_d, double* __restrict__ partials) {
    __shared__ double red[WAVES][AFF_KC];
    if (a->n_active == 0) return;                                     // every topic has stopped: the enqueued iterations are no-ops
    const int k_real = a->k_real;
    const double r_old = a->r_prev, r_new = a->r_x, s_old = a->s_prev, s_new = a->s_x;
    const uint32_t n_rows = pos_nd + pos_d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k0 = 0; k0 < k_real; k0 += AFF_KC) {
        double u[AFF_KC], d_old[AFF_KC], d_new[AFF_KC], acc[AFF_KC];
        bool any = false;
#pragma unroll
        for (int j = 0; j < AFF_KC; j++) {
            const bool on = k0 + j < k_real && a->active[k0 + j] != 0;
            any = any || on;
            u[j] = on ? a->u[k0 + j] : 0.0;
            d_old[j] = on ? r_old * u[j] + s_old : 1.0;
            d_new[j] = on ? r_new * u[j] + s_new : 1.0;
            acc[j] = 0.0;
        }
        if (any) {
            for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n_rows; i += gridDim.x * TPB) {
                const uint32_t lrow = i < pos_nd ? i : sl_nd + (i - pos_nd);
                const double2 o = xp[lrow], n = xn[lrow];
#pragma unroll
                for (int j = 0; j < AFF_KC; j++) acc[j] += fabs((n.x * u[j] + n.y) / d_new[j] - (o.x * u[j] + o.y) / d_old[j]);   // pagerank.go:118
            }
        }
#pragma unroll
        for (int j = 0; j < AFF_KC; j++) {
            double v = acc[j];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) red[wave][j] = v;
        }
        __syncthreads();
        if (threadIdx.x < AFF_KC && k0 + (int)threadIdx.x < k_real) {
            double v = 0.0;
            for (int w = 0; w < WAVES; w++) v += red[w][threadIdx.x];
            partials[(size_t)blockIdx.x * AFF_MAXK + k0 + threadIdx.x] = v;
        }
        __syncthreads();
    }
}
// one block: the topics' L1 changes (block partials in block order + the edge-less rows, which all hold one value), pagerank.go:93
// and the max_iter cut, per topic
// `stride`: doubles between two blocks' (ranks') rows of sums — AFF_MAXK for a partials / gather buffer, sl_nd * 2 when the ranks' sums are
// read where they arrived: in the spare tail rows of the all-gathered contribution table
__global__ __launch_bounds__(AFF_MAXK) void k_aff_ctl(AffCtl* __restrict__ a, PrCtl* __restrict__ ctl, const double* __restrict__ partials, unsigned nb,
                                                      double n_zero, double eps, int max_iter, size_t stride) {
    __shared__ int s_na, s_nj;
    __shared__ double s_part[16][AFF_KC];
    __shared__ double s_dl[AFF_MAXK];
    const int k = threadIdx.x;
    if (a->n_active == 0) {
        if (k == 0) a->n_just = 0;
        return;
    }
    if (k == 0) { s_na = 0; s_nj = 0; }
    const int k_real = a->k_real;
    // the blocks' partial sums, 16 topics at a time: thread (part, j) adds blocks part, part + 16, ... of topic j in block order, thread
    // j then adds the 16 parts in order — fixed order, and nobody adds 256 numbers alone
    for (int k0 = 0; k0 < k_real; k0 += AFF_KC) {
        const int j = k & (AFF_KC - 1), part = k >> 4;
        double v = 0.0;
        if (k0 + j < k_real)
            for (unsigned b = (unsigned)part; b < nb; b += 16) v += partials[(size_t)b * stride + k0 + j];
        s_part[part][j] = v;
        __syncthreads();
        if (k < AFF_KC) {
            double t = 0.0;
            for (int q = 0; q < 16; q++) t += s_part[q][k];
            s_dl[k0 + k] = t;
        }
        __syncthreads();
    }
    const int it = a->it + 1;
    if (k < k_real) {
        a->just[k] = 0;
        if (a->active[k]) {
            double dl = s_dl[k];
            const double u = a->u[k];
            const double z_new = (ctl->xz[0] * u + ctl->xz[1]) / (a->r_x * u + a->s_x);
            const double z_old = (a->xz_prev[0] * u + a->xz_prev[1]) / (a->r_prev * u + a->s_prev);
            dl += n_zero * fabs(z_new - z_old);
            a->delta[k] = dl;
            a->iters[k] = it;
            bool cont = dl > eps;                                       // pagerank.go:93
            if (max_iter > 0 && it >= max_iter) cont = false;
            if (cont) atomicAdd(&s_na, 1);
            else { a->active[k] = 0; a->just[k] = 1; atomicAdd(&s_nj, 1); }
        }
    }
    __syncthreads();
    if (k == 0) {
        a->it = it;
        a->n_active = s_na;
        a->n_just = s_nj;
        if (s_na == 0) ctl->n_active = 0;                             // the sweeps that are already enqueued return at once
    }
}
// ranks of the topics that have just stopped, by ORIGINAL id (rank_out[k][v]): one thread per node, its row's (p, q) once
__global__ __launch_bounds__(TPB) void k_aff_emit(const double2* __restrict__ x, const PrCtl* __restrict__ ctl, const AffCtl* __restrict__ a,
                                                  const uint32_t* __restrict__ new_id, uint64_t n, uint32_t sl_nd, uint32_t pos_nd, uint32_t pos_d,
                                                  double* __restrict__ out) {
    if (a->n_just == 0) return;
    const double r = a->r_x, sx = a->s_x;
    const int k_real = a->k_real;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t lrow = new_id[v];
        const bool zero = lrow < sl_nd ? lrow >= pos_nd : (lrow - sl_nd) >= pos_d;
        double2 pq;
        if (zero) pq = make_double2(ctl->xz[0], ctl->xz[1]);
        else pq = x[lrow];
        for (int k = 0; k < k_real; k++)
            if (a->just[k]) {
                const double u = a->u[k];
                out[(size_t)k * n + v] = (pq.x * u + pq.y) / (r * u + sx);
            }
    }
}

// sharded two-vector form: this rank's per-topic sums (its blocks' partials in a fixed order + its own edge-less rows); the ranks'
// sums are all-gathered and k_aff_ctl adds them in rank order (nb = world, n_zero = 0), so every rank decides alike
__global__ __launch_bounds__(AFF_MAXK) void k_aff_local(const AffCtl* __restrict__ a, const PrCtl* __restrict__ ctl, const double* __restrict__ partials, unsigned nb,
                                                        double n_zero, double* __restrict__ loc) {
    __shared__ double s_part[16][AFF_KC];
    const int k = threadIdx.x;
    const int k_real = a->k_real;
    if (a->n_active == 0) return;
    for (int k0 = 0; k0 < k_real; k0 += AFF_KC) {
        const int j = k & (AFF_KC - 1), part = k >> 4;
        double v = 0.0;
        if (k0 + j < k_real)
            for (unsigned b = (unsigned)part; b < nb; b += 16) v += partials[(size_t)b * AFF_MAXK + k0 + j];
        s_part[part][j] = v;
        __syncthreads();
        if (k < AFF_KC && k0 + k < k_real) {
            double t = 0.0;
            for (int q = 0; q < 16; q++) t += s_part[q][k];
            const int kk = k0 + k;
            if (a->active[kk]) {
                const double u = a->u[kk];
                const double z_new = (ctl->xz[0] * u + ctl->xz[1]) / (a->r_x * u + a->s_x);
                const double z_old = (a->xz_prev[0] * u + a->xz_prev[1]) / (a->r_prev * u + a->s_prev);
                t += n_zero * fabs(z_new - z_old);
            }
            loc[kk] = t;
        }
        __syncthreads();
    }
}
// ... and the ranks of the topics that have just stopped, for this rank's rows in local order (out[k][row], as ss_pr_read_local)
__global__ __launch_bounds__(TPB) void k_aff_emit_local(const double2* __restrict__ x, const PrCtl* __restrict__ ctl, const AffCtl* __restrict__ a,
                                                        uint32_t sl_nd, uint32_t cnt_nd, uint32_t cnt_d, uint32_t pos_nd, uint32_t pos_d,
                                                        double* __restrict__ out, int lag) {
    if (a->n_just == 0) return;
    // lag: the decision arrives one exchange late (its sums rode on the next iteration's all-gather): `x` are the vectors BEFORE the last
    // sweep, and their r, s and edge-less rows are the control block's "previous" ones
    const double r = lag ? a->r_prev : a->r_x, sx = lag ? a->s_prev : a->s_x;
    const double xz0 = lag ? a->xz_prev[0] : ctl->xz[0], xz1 = lag ? a->xz_prev[1] : ctl->xz[1];
    const int k_real = a->k_real;
    const uint32_t n_rows = cnt_nd + cnt_d;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += gridDim.x * blockDim.x) {
        const uint32_t lrow = i < cnt_nd ? i : sl_nd + (i - cnt_nd);
        const bool zero = lrow < sl_nd ? lrow >= pos_nd : (lrow - sl_nd) >= pos_d;
        double2 pq;
        if (zero) pq = make_double2(xz0, xz1);
        else pq = x[lrow];
        for (int k = 0; k < k_real; k++)
            if (a->just[k]) {
                const double u = a->u[k];
                out[(size_t)k * n_rows + i] = (pq.x * u + pq.y) / (r * u + sx);
            }
    }
}

// ---- float32 on the wire (option "pr.wire_f32", opt-in; bench.py reports it under `decompositions` only) --------------------
// The doc-range-sharded sweep is bound by the bytes a rank receives per sweep over its point-to-point xGMI links (VERDICT r3:
// 52 MB per link at K = 16 whatever the world size).  With this option a rank's contribution slice travels as float32 — half the
// bytes — and is widened again on arrival; the two tail rows of the slice (the rank's partial sums: normaliser and L1 change,
// which every rank must combine identically and which decide the stop rule) travel as (hi, lo) float pairs, i.e. to ~2^-48.
// Every rank decodes the SAME gathered floats, its own slice included, so the ranks stay in lockstep.  The ranks differ from the
// float64 exchange by the rounding of the contributions (2^-24 relative each, averaging out in the sums): inside the 1e-6 parity
// gate, not the reference's float64 arithmetic — which is why it is not the default.  Arithmetic on the device stays float64.
__global__ void k_wire_pack(const double* __restrict__ send, uint32_t n_body, uint32_t n_tail, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_body) out[i] = (float)send[i];
    else if (i < n_body + n_tail) {
        const double d = send[i];
        const float hi = (float)d;
        out[n_body + 2 * (i - n_body)] = hi;
        out[n_body + 2 * (i - n_body) + 1] = (float)(d - (double)hi);
    }
}
// in: [world][n_body + 2 n_tail] floats -> table [world][n_body + n_tail] doubles
__global__ void k_wire_unpack(const float* __restrict__ in, uint32_t world, uint32_t n_body, uint32_t n_tail, double* __restrict__ table) {
    const uint64_t per_out = (uint64_t)n_body + n_tail, per_in = (uint64_t)n_body + 2ull * n_tail;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_out * world) return;
    const uint64_t r = i / per_out, j = i % per_out;
    const float* src = in + r * per_in;
    table[i] = j < n_body ? (double)src[j] : (double)src[n_body + 2 * (j - n_body)] + (double)src[n_body + 2 * (j - n_body) + 1];
}
// floats a rank sends: the slice's body rows + its tail rows (the two sums rows and the TAIL_SUM_ROWS in front of them) as pairs
constexpr uint32_t WIRE_TAIL_ROWS = 2u + TAIL_SUM_ROWS;

}  // namespace

namespace ss {
size_t pr_wire_floats(const ss_pr* pr) { return (size_t)pr->g->sl_nd * pr->gw + (size_t)WIRE_TAIL_ROWS * (size_t)pr->gw; }
hipError_t pr_wire_alloc(ss_pr* pr) {
    if (pr->wire_send.p) return hipSuccess;
    hipError_t e = pr->wire_send.alloc(pr_wire_floats(pr));
    if (e == hipSuccess) e = pr->wire_recv.alloc(pr_wire_floats(pr) * (size_t)pr->g->world);
    return e;
}
void pr_wire_pack(ss_pr* pr, hipStream_t st) {
    const uint32_t n_tail = WIRE_TAIL_ROWS * (uint32_t)pr->gw, n_body = pr->g->sl_nd * (uint32_t)pr->gw - n_tail;
    hipLaunchKernelGGL(k_wire_pack, dim3(ss::div_up((size_t)n_body + n_tail, TPB)), dim3(TPB), 0, st, (const double*)pr->send.p, n_body, n_tail, pr->wire_send.p);
}
void pr_wire_unpack(ss_pr* pr, hipStream_t st) {
    const uint32_t n_tail = WIRE_TAIL_ROWS * (uint32_t)pr->gw, n_body = pr->g->sl_nd * (uint32_t)pr->gw - n_tail;
    hipLaunchKernelGGL(k_wire_unpack, dim3(ss::div_up(((size_t)n_body + n_tail) * pr->g->world, TPB)), dim3(TPB), 0, st, (const float*)pr->wire_recv.p,
                       (uint32_t)pr->g->world, n_body, n_tail, pr->tab0.p);
}
}  // namespace ss

namespace {

// ---- the sharded power iteration as ONE pipeline inside the library ---------------------------------
// The K topic vectors are split into B topic blocks (separate states over the same shard); block b's exchange runs on the
// context's second stream while block b+1 is finalised and swept on the first:
//     compute:  [fin 0][sweep 0]      [fin 1][sweep 1]      [fin 0][sweep 0] ...
//     comm:                 [exchange 0 ..........][exchange 1 ..........]
// HIP events order the two streams; the host enqueues and looks at the device-side stop rule every BATCH sweeps.  Topics are
// independent power iterations (pagerank.go:54-63), so a block's results are bit for bit those of running its topics alone.
// The exchange is a functor: RCCL for one shard per process (ss_pagerank_run_sharded), device-to-device copies for the
// shards of a single-process group (ss_pagerank_run_group: tests, and one process driving several shards on one device).
struct ShardBlocks { std::vector<ss_pr*> blk; };

template <typename Exchange>
int32_t run_pipelined(ss_ctx* ctx, std::vector<ShardBlocks>& sh, int32_t max_iter, Exchange&& exchange, int32_t* iters_out,
                      const std::vector<int>& blk_k0) {
    const int B = (int)sh[0].blk.size(), S = (int)sh.size();
    hipStream_t cs = ctx->stream, xs = ctx->comm_stream;
    std::vector<hipEvent_t> ev_step(B), ev_xchg(B);
    for (int b = 0; b < B; b++) {
        SS_HIP(ctx, hipEventCreateWithFlags(&ev_step[b], hipEventDisableTiming));
        SS_HIP(ctx, hipEventCreateWithFlags(&ev_xchg[b], hipEventDisableTiming));
    }
    auto cleanup = [&] {
        if (!ss::device_wedged(ctx->device)) {                       // (after a timed-out collective neither stream will ever drain)
            (void)hipStreamSynchronize(xs);
            (void)hipStreamSynchronize(cs);
        }
        for (int b = 0; b < B; b++) { (void)hipEventDestroy(ev_step[b]); (void)hipEventDestroy(ev_xchg[b]); }
    };
    int32_t rc = SS_OK;
    auto start_exchange = [&](int b) -> int32_t {
        SS_HIP(ctx, hipEventRecord(ev_step[b], cs));
        SS_HIP(ctx, hipStreamWaitEvent(xs, ev_step[b], 0));
        SS_TRY(exchange(b, xs));
        SS_HIP(ctx, hipEventRecord(ev_xchg[b], xs));
        return SS_OK;
    };
    // prime: every block begun, its first exchange in flight
    for (int b = 0; b < B && rc == SS_OK; b++) {
        for (int s = 0; s < S; s++) {
            ss_pr* pr = sh[s].blk[b];
            SS_HIP(ctx, hipMemsetAsync(&pr->ctl.p->ticket, 0, sizeof(uint32_t), cs));
            ss::pr_launch_begin(pr, cs, ss::begin_blocks(pr));
            pr->begun = true;
        }
        rc = start_exchange(b);
    }
    bool first = true;
    const int BATCH = 8;
    int32_t sweeps_done = 0;
    for (;;) {
        if (rc != SS_OK) break;
        int todo = BATCH;
        if (max_iter > 0) todo = std::min(BATCH, std::max(1, max_iter - sweeps_done));
        for (int i = 0; i < todo && rc == SS_OK; i++) {
            for (int b = 0; b < B && rc == SS_OK; b++) {
                if (hipStreamWaitEvent(cs, ev_xchg[b], 0) != hipSuccess) { rc = ctx->fail(SS_ERR_HIP, "hipStreamWaitEvent"); break; }
                for (int s = 0; s < S; s++) ss::pr_launch_finalize(sh[s].blk[b], cs, first ? 1 : 0);
                for (int s = 0; s < S; s++) ss::pr_launch_step(sh[s].blk[b], cs);
                rc = start_exchange(b);
            }
            first = false;
            sweeps_done++;
        }
        if (rc != SS_OK) break;
        if (hipGetLastError() != hipSuccess) { rc = ctx->fail(SS_ERR_HIP, "sharded sweep: launch failed"); break; }
        // the stop rule lives on the device and is evaluated identically on every rank (same gathered sums, same order);
        // what the host reads lags the in-flight sweep by one, and launches after convergence are no-ops on all ranks alike
        int32_t n_active = 0;
        for (int b = 0; b < B && rc == SS_OK; b++) {
            const PrCtl* hp = nullptr;
            if ((rc = read_ctl(ctx, sh[0].blk[b], cs, "sharded sweep (waiting for the exchange)", &hp)) != SS_OK) break;
            n_active += hp->n_active;
        }
        if (n_active == 0) break;
    }
    // drain: apply the exchanges still in flight (no-ops after convergence)
    for (int b = 0; b < B && rc == SS_OK; b++) {
        if (hipStreamWaitEvent(cs, ev_xchg[b], 0) != hipSuccess) { rc = ctx->fail(SS_ERR_HIP, "hipStreamWaitEvent"); break; }
        for (int s = 0; s < S; s++) {
            ss::pr_launch_finalize(sh[s].blk[b], cs, first ? 1 : 0);
            sh[s].blk[b]->need_finalize = false;
        }
    }
    if (rc == SS_OK && iters_out) {
        for (int b = 0; b < B && rc == SS_OK; b++) {
            const PrCtl* hp = nullptr;
            if ((rc = read_ctl(ctx, sh[0].blk[b], cs, "sharded sweep (last exchange)", &hp)) != SS_OK) break;
            for (int k = 0; k < sh[0].blk[b]->k; k++) iters_out[blk_k0[b] + k] = hp->iters[k];
        }
    }
    cleanup();
    return rc;
}

// topic blocks of a K-topic run: option "pr.topic_blocks" (default 2 above 8 topics: one block's exchange then hides behind
// the other block's sweep — and both blocks still fill an 8-wide table; splitting 8 topics or fewer would pad every block to
// the 8-wide kernel and double the bytes on the wire), never more blocks than topics
int topic_blocks_for(ss_ctx* ctx, int k_topics) {
    int B = (int)ctx->opt("pr.topic_blocks", k_topics > 8 ? 2 : 1);
    return std::max(1, std::min(B, k_topics));
}

// ---- the two-vector form (option "pr.affine") -----------------------------------------------------------------------------------
// A K = 2 state becomes the (p, q) pair of the two-vector form: the control block with the topics' start values u_k = 1 / n_topic[k],
// the start vector x0 = (1, 0) (p = 1, q = 0: the start vector is u * 1), and the sweep's three attachments.  `aff`, `x_alt`: the
// caller's device buffers (one AffCtl, n_local * 2 doubles).  Waits for the stream (the host copies are temporaries).
int32_t aff_init(ss_pr* pr, int32_t k_topics, const int32_t* n_topic, AffCtl* aff, double* x_alt) {
    ss_ctx* ctx = pr->g->ctx;
    hipStream_t st = ctx->stream;
    std::vector<AffCtl> h(1);
    std::memset(h.data(), 0, sizeof(AffCtl));
    for (int k = 0; k < k_topics; k++) { h[0].u[k] = 1.0 / (double)n_topic[k]; h[0].active[k] = 1; }   // pagerank.go:104
    h[0].k_real = k_topics;
    h[0].n_active = k_topics;
    SS_HIP(ctx, hipMemcpyAsync(aff, h.data(), sizeof(AffCtl), hipMemcpyHostToDevice, st));
    const double x0[MAXK] = {1.0, 0.0};
    SS_HIP(ctx, hipMemcpyAsync(pr->x0.p, x0, sizeof(x0), hipMemcpyHostToDevice, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    pr->prm.aff = aff;
    pr->prm.tele_col = pr->ctl.p->tele;
    pr->prm.x_alt = x_alt;
    return SS_OK;
}

// ---- the two-vector form on a sharded graph: a TWO-column exchange per iteration, whatever K is ----------------------------------
// One K = 2 state per shard; per iteration: sweep (local rows) -> all-gather of the 2-wide contribution slices -> k_pr_finalize
// (affine branch: r, s, the column teleports; identical on every rank) -> the topics' L1 changes over the local rows -> all-gather
// of the ranks' K sums -> stop rule (k_aff_ctl adds them in rank order) -> write-out of the topics that have just stopped.
struct AffShard {
    ss::DevBuf<AffCtl> aff;
    ss::DevBuf<double> x_alt, partials, loc, gath, out;
    double n_zero = 0.0;
};
int32_t aff_attach(ss_pr* pr, AffShard& A, int32_t k_topics, const int32_t* n_topic, int world) {
    ss_ctx* ctx = pr->g->ctx;
    if (!pr->nwave || pr->gw != 2) return ctx->fail(SS_ERR_UNSUPPORTED, "pr.affine: needs the wave-item K = 2 sweep (pr.narrow_wave / pr.force_narrow at their defaults)");
    const ss_graph* g = pr->g;
    const size_t n_rows = (size_t)g->cnt_nd + g->cnt_d;
    SS_HIP(ctx, A.aff.alloc(1));
    SS_HIP(ctx, A.x_alt.alloc((size_t)g->n_local() * 2));
    SS_HIP(ctx, A.partials.alloc((size_t)AFF_NB * AFF_MAXK));
    SS_HIP(ctx, A.loc.alloc(AFF_MAXK));
    SS_HIP(ctx, A.gath.alloc((size_t)world * AFF_MAXK));
    SS_HIP(ctx, A.out.alloc(std::max<size_t>(1, (size_t)k_topics * n_rows)));
    SS_HIP(ctx, hipMemsetAsync(A.loc.p, 0, A.loc.bytes(), ctx->stream));
    SS_TRY(aff_init(pr, k_topics, n_topic, A.aff.p, A.x_alt.p));
    A.n_zero = (double)((g->cnt_nd - pr->prm.pos_nd) + (g->cnt_d - pr->prm.pos_d));
    return SS_OK;
}
template <typename Exchange, typename ExchangeSums>
int32_t run_affine_sharded(ss_ctx* ctx, std::vector<ShardBlocks>& sh, std::vector<AffShard>& A, int world, double eps, int32_t max_iter, int32_t k_topics,
                           Exchange&& exchange, ExchangeSums&& exchange_sums, int32_t* iters_out) {
    const int S = (int)sh.size();
    hipStream_t st = ctx->stream;
    for (int s = 0; s < S; s++) {
        ss_pr* pr = sh[s].blk[0];
        SS_HIP(ctx, hipMemsetAsync(&pr->ctl.p->ticket, 0, sizeof(uint32_t), st));
        ss::pr_launch_begin(pr, st, ss::begin_blocks(pr));
        pr->begun = true;
    }
    SS_TRY(exchange(0, st));
    for (int s = 0; s < S; s++) ss::pr_launch_finalize(sh[s].blk[0], st, 1);
    int32_t n_active = k_topics, it = 0;
    const int BATCH = 4;
    // ONE collective per iteration (option "pr.affine_lag", default 1): the ranks' per-topic L1 sums of iteration i are written into the
    // spare tail rows of the rank's contribution slice (graph.hpp: TAIL_SUM_ROWS) and travel with iteration i + 1's all-gather, so the
    // stop decisions of iteration i are taken one exchange later — from the same numbers, added in the same rank order — and the ranks
    // of a topic that stops are written from the vectors of the iteration it stopped in, which the alternating pair still holds.
    // A second, 2 KB all-gather per iteration was pure latency on a ~0.25 ms iteration; it survives only as the flush
    // after the last sweep of a max_iter run.  0: the round-4 protocol (sums in a collective of their own, decisions at once).
    // (the spare rows hold 2 * TAIL_SUM_ROWS = 64 sums = SS_MAX_TOPICS; these two entry points take up to AFF_MAXK topics in this form, and
    //  beyond 64 the sums keep their own collective)
    const bool lag = ctx->opt("pr.affine_lag", 1) != 0 && k_topics <= (int32_t)(2 * TAIL_SUM_ROWS);
    auto sums_row = [&](ss_pr* pr, double* base) { return base + ((size_t)pr->g->sl_nd - 2 - TAIL_SUM_ROWS) * 2; };
    auto delta_and_local = [&](int s, double* loc) {
        ss_pr* pr = sh[s].blk[0];
        const ss_graph* g = pr->g;
        const double2* const x_old = reinterpret_cast<const double2*>((it & 1) ? A[s].x_alt.p : pr->x.p);
        const double2* const x_new = reinterpret_cast<const double2*>((it & 1) ? pr->x.p : A[s].x_alt.p);
        hipLaunchKernelGGL(k_aff_delta, dim3(AFF_NB), dim3(TPB), 0, st, x_old, x_new, (const AffCtl*)A[s].aff.p, g->sl_nd, pr->prm.pos_nd, pr->prm.pos_d,
                           A[s].partials.p);
        hipLaunchKernelGGL(k_aff_local, dim3(1), dim3(AFF_MAXK), 0, st, (const AffCtl*)A[s].aff.p, (const PrCtl*)pr->ctl.p, (const double*)A[s].partials.p,
                           AFF_NB, A[s].n_zero, loc);
    };
    auto ctl_and_emit = [&](int s, const double* sums, size_t stride, int emit_lag) {
        ss_pr* pr = sh[s].blk[0];
        const ss_graph* g = pr->g;
        // (emit_lag: the vectors before the last sweep — iteration it - 1 — else the ones it has just written)
        const bool odd = (it & 1) != 0;
        const double2* const x_src = reinterpret_cast<const double2*>(emit_lag ? (odd ? A[s].x_alt.p : pr->x.p) : (odd ? pr->x.p : A[s].x_alt.p));
        hipLaunchKernelGGL(k_aff_ctl, dim3(1), dim3(AFF_MAXK), 0, st, A[s].aff.p, pr->ctl.p, sums, (unsigned)world, 0.0, eps, max_iter, stride);
        const unsigned nbe = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(4096, ss::div_up((uint64_t)g->cnt_nd + g->cnt_d, TPB)));
        hipLaunchKernelGGL(k_aff_emit_local, dim3(nbe), dim3(TPB), 0, st, x_src, (const PrCtl*)pr->ctl.p, (const AffCtl*)A[s].aff.p, g->sl_nd, g->cnt_nd,
                           g->cnt_d, pr->prm.pos_nd, pr->prm.pos_d, A[s].out.p, emit_lag);
    };
    while (n_active > 0) {
        for (int b = 0; b < BATCH; b++) {
            for (int s = 0; s < S; s++) ss::pr_launch_step(sh[s].blk[0], st);
            SS_TRY(exchange(0, st));
            for (int s = 0; s < S; s++) ss::pr_launch_finalize(sh[s].blk[0], st, 0);
            if (lag) {
                for (int s = 0; s < S; s++) {
                    ss_pr* pr = sh[s].blk[0];
                    // iteration it - 1: its sums have just arrived with this iteration's table (every rank's slice, rank order)
                    if (it > 0) ctl_and_emit(s, sums_row(pr, pr->tab0.p), (size_t)pr->g->sl_nd * 2, 1);
                    delta_and_local(s, sums_row(pr, pr->send.p));              // iteration it: into the slice the NEXT all-gather sends
                }
            } else {
                for (int s = 0; s < S; s++) delta_and_local(s, A[s].loc.p);
                SS_TRY(exchange_sums(st));
                for (int s = 0; s < S; s++) ctl_and_emit(s, A[s].gath.p, (size_t)AFF_MAXK, 0);
            }
            it++;
            if (max_iter > 0 && it >= max_iter) break;
        }
        SS_HIP(ctx, hipGetLastError());
        ctx->pin_used = 0;
        int32_t* const hn = ctx->pin<int32_t>();
        SS_HIP(ctx, hipMemcpyAsync(hn, &A[0].aff.p->n_active, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SS_TRY(ss::sync_bounded(ctx, st, "sharded two-vector sweep (waiting for the exchange)"));
        n_active = *hn;
        if (max_iter > 0 && it >= max_iter) break;
    }
    if (lag && max_iter > 0 && it >= max_iter && n_active > 0) {
        // the last sweep's sums have no further all-gather to ride on: one small collective of their own, then the decisions (every
        // topic still running stops here: it >= max_iter) and the ranks from the vectors that sweep has written
        it--;                                                          // (the lambdas take the parity of the sweep they describe)
        for (int s = 0; s < S; s++) {
            ss_pr* pr = sh[s].blk[0];
            hipLaunchKernelGGL(k_aff_local, dim3(1), dim3(AFF_MAXK), 0, st, (const AffCtl*)A[s].aff.p, (const PrCtl*)pr->ctl.p, (const double*)A[s].partials.p,
                               AFF_NB, A[s].n_zero, A[s].loc.p);
        }
        SS_TRY(exchange_sums(st));
        for (int s = 0; s < S; s++) ctl_and_emit(s, A[s].gath.p, (size_t)AFF_MAXK, 0);
        it++;
        SS_HIP(ctx, hipGetLastError());
    }
    for (int s = 0; s < S; s++) sh[s].blk[0]->need_finalize = false;
    if (iters_out) {
        std::vector<AffCtl> h(1);
        SS_HIP(ctx, hipMemcpyAsync(h.data(), A[0].aff.p, sizeof(AffCtl), hipMemcpyDeviceToHost, st));
        SS_TRY(ss::sync_bounded(ctx, st, "sharded two-vector sweep (status)"));
        for (int k = 0; k < k_topics; k++) iters_out[k] = h[0].iters[k];
    }
    return SS_OK;
}
// the ids of a shard's rows in local order (what ss_pr_read_local returns beside the ranks)
int32_t local_ids(ss_pr* pr, uint32_t* ids_out) {
    const size_t n_rows = (size_t)pr->g->cnt_nd + pr->g->cnt_d;
    std::vector<double> scratch(std::max<size_t>(1, n_rows * (size_t)pr->k));
    return ss_pr_read_local(pr, ids_out, scratch.data());
}

// eps < 0 never converges: such a run needs max_iter (a NaN eps stops after one sweep).  `who`: the entry point, for the error.
int32_t check_eps(ss_ctx* ctx, const char* who, double eps, int32_t max_iter) {
    if (!(eps >= 0.0) && max_iter <= 0 && !(eps != eps)) return ctx->fail(SS_ERR_INVALID, "%s: eps < 0 (never converges) needs max_iter > 0", who);
    return SS_OK;
}

// The states of a sharded run: sh[s].blk[b] = topic block b (topics k0[b] .. k0[b + 1]) on shard s — or, in the two-vector form, the
// one K = 2 state per shard with its AffShard attached.  The two-vector form needs every n_topic[k] >= 1; check_first: that is
// checked before anything is created (ss_pagerank_run_group), otherwise behind the first shard's states (ss_pagerank_run_sharded).
// On an error the states created so far stay in `sh` for the caller to destroy.
int32_t make_topic_blocks(ss_ctx* ctx, const char* who, ss_graph* const* shards, int n_shards, bool affine, bool check_first, double damping, double eps,
                          int32_t max_iter, int32_t k_topics, const int32_t* n_topic, std::vector<ShardBlocks>& sh, std::vector<AffShard>& aff, std::vector<int>& k0) {
    const int B = affine ? 1 : topic_blocks_for(ctx, k_topics);
    sh.resize(n_shards);
    aff.resize(affine ? n_shards : 0);
    k0.resize(B + 1);
    for (int b = 0; b <= B; b++) k0[b] = (int)((int64_t)k_topics * b / B);
    auto check_sizes = [&]() -> int32_t {
        for (int k = 0; k < k_topics; k++)
            if (n_topic[k] < 1) return ctx->fail(SS_ERR_INVALID, "%s: n_topic[%d] < 1", who, k);
        return SS_OK;
    };
    if (affine && check_first) SS_TRY(check_sizes());
    const int32_t two[2] = {1, 1};
    for (int s = 0; s < n_shards; s++) {
        for (int b = 0; b < B; b++) {
            ss_pr* pr = nullptr;
            SS_TRY(affine ? ss_pr_create(shards[s], damping, -1.0, 0, 2, two, &pr)
                          : ss_pr_create(shards[s], damping, eps, max_iter, k0[b + 1] - k0[b], n_topic + k0[b], &pr));
            sh[s].blk.push_back(pr);
        }
        if (affine && !check_first && s == 0) SS_TRY(check_sizes());
        if (affine) SS_TRY(aff_attach(sh[s].blk[0], aff[s], k_topics, n_topic, shards[s]->world));
    }
    return SS_OK;
}

// ss_pagerank_run in the two-vector form (option "pr.affine" = 1; world 1, the reference's uniform teleport): every topic of the
// reference's recurrence from TWO vectors (AffCtl).  One iteration = a copy of the stored vectors, one K = 2 sweep (k_pr_sweep_n<2>),
// one streaming pass for the topics' L1 changes, the stop rule, and the write-out of the topics that have just stopped.
int32_t run_affine(ss_graph* g, double damping, double eps, int32_t max_iter, int32_t k_topics, const int32_t* n_topic,
                   double* rank_out, int32_t* iters_out) {
    ss_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    if (k_topics > AFF_MAXK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_pagerank_run (pr.affine): at most %d topics", AFF_MAXK);
    for (int k = 0; k < k_topics; k++)
        if (n_topic[k] < 1) return ctx->fail(SS_ERR_INVALID, "ss_pagerank_run: n_topic[%d] < 1", k);
    const int32_t two[2] = {1, 1};
    ss_pr* pr = nullptr;
    SS_TRY(ss_pr_create(g, damping, -1.0, 0, 2, two, &pr));
    struct Guard { ss_pr* p; ~Guard() { ss_pr_destroy(p); } } guard{pr};
    if (!pr->nwave || pr->gw != 2) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_pagerank_run (pr.affine): needs the wave-item K = 2 sweep (pr.narrow_wave / pr.force_narrow at their defaults)");
    const uint32_t n_local = g->n_local();
    ss::DevBuf<AffCtl> aff;
    ss::DevBuf<double> x_prev, partials, d_out;
    SS_HIP(ctx, aff.alloc(1));
    SS_HIP(ctx, x_prev.alloc((size_t)n_local * 2));
    SS_HIP(ctx, partials.alloc((size_t)AFF_NB * AFF_MAXK));
    SS_TRY(aff_init(pr, k_topics, n_topic, aff.p, x_prev.p));
    // results: straight into the caller's array when it lives on the device
    hipPointerAttribute_t at{};
    const bool dev_out = hipPointerGetAttributes(&at, rank_out) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    double* out = rank_out;
    if (!dev_out) {
        SS_HIP(ctx, d_out.alloc((size_t)k_topics * g->n));
        out = d_out.p;
    }
    SS_TRY(ss_pr_begin(pr));
    const double n_zero = (double)((g->cnt_nd - pr->prm.pos_nd) + (g->cnt_d - pr->prm.pos_d));
    int32_t n_active = k_topics, it = 0;
    const int BATCH = 4;
    while (n_active > 0) {
        for (int b = 0; b < BATCH; b++) {
            // sweep number `it` (from 0) reads x / x_alt (even / odd) and writes the other one
            const double2* const x_old = reinterpret_cast<const double2*>((it & 1) ? x_prev.p : pr->x.p);
            const double2* const x_new = reinterpret_cast<const double2*>((it & 1) ? pr->x.p : x_prev.p);
            ss::pr_launch_step(pr, st);
            hipLaunchKernelGGL(k_aff_delta, dim3(AFF_NB), dim3(TPB), 0, st, x_old, x_new, (const AffCtl*)aff.p, g->sl_nd, pr->prm.pos_nd, pr->prm.pos_d, partials.p);
            hipLaunchKernelGGL(k_aff_ctl, dim3(1), dim3(AFF_MAXK), 0, st, aff.p, pr->ctl.p, (const double*)partials.p, AFF_NB, n_zero, eps, max_iter, (size_t)AFF_MAXK);
            hipLaunchKernelGGL(k_aff_emit, dim3((unsigned)std::min<uint64_t>(4096, ss::div_up(g->n, TPB))), dim3(TPB), 0, st, x_new, (const PrCtl*)pr->ctl.p,
                               (const AffCtl*)aff.p, (const uint32_t*)g->new_id.p, g->n, g->sl_nd, pr->prm.pos_nd, pr->prm.pos_d, out);
            it++;
            if (max_iter > 0 && it >= max_iter) break;
        }
        SS_HIP(ctx, hipGetLastError());
        SS_HIP(ctx, ss::fetch(ctx, st, &n_active, &aff.p->n_active, sizeof(int32_t)));
        if (max_iter > 0 && it >= max_iter) break;                 // (the stop rule has closed every topic at max_iter)
    }
    std::vector<AffCtl> h(1);
    SS_HIP(ctx, hipMemcpyAsync(h.data(), aff.p, sizeof(AffCtl), hipMemcpyDeviceToHost, st));
    if (!dev_out) SS_HIP(ctx, hipMemcpyAsync(rank_out, d_out.p, (size_t)k_topics * g->n * sizeof(double), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (iters_out)
        for (int k = 0; k < k_topics; k++) iters_out[k] = h[0].iters[k];
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_pagerank_run_sharded(ss_graph* g, double damping, double eps, int32_t max_iter, int32_t k_topics,
                                const int32_t* n_topic, int32_t allreduce, uint32_t* ids_out, double* rank_out, int32_t* iters_out) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (g->world < 2) return ctx->fail(SS_ERR_STATE, "ss_pagerank_run_sharded: needs a sharded graph (world > 1); use ss_pagerank_run");
    const bool affine = ctx->opt("pr.affine", 0) != 0 && !allreduce;      // the two-vector form: a 2-column exchange whatever K is
    const int k_max = affine ? AFF_MAXK : MAXK;
    if (k_topics < 1 || k_topics > k_max || !n_topic || !rank_out)
        return ctx->fail(SS_ERR_INVALID, "ss_pagerank_run_sharded: k_topics must be 1..%d, n_topic/rank_out not NULL", k_max);
    SS_TRY(check_eps(ctx, "ss_pagerank_run_sharded", eps, max_iter));
    if (!ctx->comm || ctx->comm_world != g->world || ctx->comm_rank != g->rank)
        return ctx->fail(SS_ERR_STATE, "ss_pagerank_run_sharded: the context's communicator (rank %d of %d) does not match the graph's shard (rank %d of %d)",
                         ctx->comm ? ctx->comm_rank : -1, ctx->comm ? ctx->comm_world : 0, g->rank, g->world);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<ShardBlocks> sh;
    std::vector<AffShard> aff;
    std::vector<int> k0;
    int32_t rc = make_topic_blocks(ctx, "ss_pagerank_run_sharded", &g, 1, affine, false, damping, eps, max_iter, k_topics, n_topic, sh, aff, k0);
    const bool wire_f32 = ctx->opt("pr.wire_f32", 0) != 0;
    if (rc == SS_OK) {
        auto exchange = [&](int b, hipStream_t xs) -> int32_t {
            ss_pr* pr = sh[0].blk[b];
            const size_t slice = (size_t)g->sl_nd * pr->gw;            // doubles per rank
            if (!allreduce && wire_f32) {
                SS_HIP(ctx, ss::pr_wire_alloc(pr));
                ss::pr_wire_pack(pr, xs);
                SS_TRY(ss::comm_allgather_on(ctx, pr->wire_send.p, pr->wire_recv.p, ss::pr_wire_floats(pr) * sizeof(float), xs));
                ss::pr_wire_unpack(pr, xs);
                return SS_OK;
            }
            if (!allreduce) return ss::comm_allgather_on(ctx, pr->send.p, pr->tab0.p, slice * sizeof(double), xs);
            // north-star form: own slice inside a zeroed full-size table, tables summed
            SS_HIP(ctx, hipMemsetAsync(pr->tab0.p, 0, pr->tab0.bytes(), xs));
            SS_HIP(ctx, hipMemcpyAsync(pr->tab0.p + (size_t)g->rank * slice, pr->send.p, slice * sizeof(double), hipMemcpyDeviceToDevice, xs));
            return ss::comm_allreduce_f64_on(ctx, pr->tab0.p, pr->tab0.p, slice * (size_t)g->world, xs);
        };
        if (affine) {
            auto exchange_sums = [&](hipStream_t xs) -> int32_t {
                return ss::comm_allgather_on(ctx, aff[0].loc.p, aff[0].gath.p, (size_t)AFF_MAXK * sizeof(double), xs);
            };
            rc = run_affine_sharded(ctx, sh, aff, g->world, eps, max_iter, k_topics, exchange, exchange_sums, iters_out);
        } else {
            rc = run_pipelined(ctx, sh, max_iter, exchange, iters_out, k0);
        }
    }
    // this rank's rows: ids once, ranks block by block (topic-major: rank_out[k][rows])
    const size_t n_rows = (size_t)g->cnt_nd + g->cnt_d;
    if (affine) {
        if (rc == SS_OK && ids_out) rc = local_ids(sh[0].blk[0], ids_out);
        if (rc == SS_OK && n_rows) {
            if (hipMemcpyAsync(rank_out, aff[0].out.p, (size_t)k_topics * n_rows * sizeof(double), hipMemcpyDefault, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess)
                rc = ctx->fail(SS_ERR_HIP, "ss_pagerank_run_sharded: copy of the ranks failed");
        }
    } else
    for (int b = 0; b < (int)sh[0].blk.size() && rc == SS_OK; b++)
        rc = ss_pr_read_local(sh[0].blk[b], b == 0 ? ids_out : nullptr, rank_out + (size_t)k0[b] * n_rows);
    for (ss_pr* pr : sh[0].blk) ss_pr_destroy(pr);
    return rc;
}

int32_t ss_pagerank_run_group(ss_graph* const* shards, int32_t world, double damping, double eps, int32_t max_iter, int32_t k_topics,
                              const int32_t* n_topic, double* rank_out, int32_t* iters_out) {
    if (!shards || world < 2 || !shards[0]) return SS_ERR_INVALID;
    ss_ctx* ctx = shards[0]->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool affine = ctx->opt("pr.affine", 0) != 0;
    const int k_max = affine ? AFF_MAXK : MAXK;
    if (k_topics < 1 || k_topics > k_max || !n_topic || !rank_out)
        return ctx->fail(SS_ERR_INVALID, "ss_pagerank_run_group: k_topics must be 1..%d, n_topic/rank_out not NULL", k_max);
    SS_TRY(check_eps(ctx, "ss_pagerank_run_group", eps, max_iter));
    for (int s = 0; s < world; s++)
        if (!shards[s] || shards[s]->ctx != ctx || shards[s]->world != world || shards[s]->rank != s || shards[s]->n != shards[0]->n)
            return ctx->fail(SS_ERR_INVALID, "ss_pagerank_run_group: shards[%d] is not shard %d of %d of the same graph on this context", s, s, world);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<ShardBlocks> sh;
    std::vector<AffShard> aff;
    std::vector<int> k0;
    int32_t rc = make_topic_blocks(ctx, "ss_pagerank_run_group", shards, world, affine, true, damping, eps, max_iter, k_topics, n_topic, sh, aff, k0);
    const int B = (int)k0.size() - 1;
    if (rc == SS_OK) {
        // the all-gather, by hand: every shard's slice into every shard's table, rank order
        const bool wire_f32 = ctx->opt("pr.wire_f32", 0) != 0;
        auto exchange = [&](int b, hipStream_t xs) -> int32_t {
            if (wire_f32) {                                         // the float32 wire format, played by device-to-device copies
                for (int src = 0; src < world; src++) {
                    SS_HIP(ctx, ss::pr_wire_alloc(sh[src].blk[b]));
                    ss::pr_wire_pack(sh[src].blk[b], xs);
                }
                for (int dst = 0; dst < world; dst++) {
                    ss_pr* to = sh[dst].blk[b];
                    for (int src = 0; src < world; src++) {
                        ss_pr* from = sh[src].blk[b];
                        SS_HIP(ctx, hipMemcpyAsync(to->wire_recv.p + (size_t)src * ss::pr_wire_floats(from), from->wire_send.p, ss::pr_wire_floats(from) * sizeof(float),
                                                   hipMemcpyDeviceToDevice, xs));
                    }
                    ss::pr_wire_unpack(to, xs);
                }
                return SS_OK;
            }
            for (int dst = 0; dst < world; dst++)
                for (int src = 0; src < world; src++) {
                    ss_pr* from = sh[src].blk[b];
                    ss_pr* to = sh[dst].blk[b];
                    const size_t slice = (size_t)shards[src]->sl_nd * from->gw;
                    SS_HIP(ctx, hipMemcpyAsync(to->tab0.p + (size_t)src * slice, from->send.p, slice * sizeof(double), hipMemcpyDeviceToDevice, xs));
                }
            return SS_OK;
        };
        if (affine) {
            auto exchange_sums = [&](hipStream_t xs) -> int32_t {     // the K sums of every shard into every shard's table, rank order
                for (int dst = 0; dst < world; dst++)
                    for (int src = 0; src < world; src++)
                        SS_HIP(ctx, hipMemcpyAsync(aff[dst].gath.p + (size_t)src * AFF_MAXK, aff[src].loc.p, (size_t)AFF_MAXK * sizeof(double),
                                                   hipMemcpyDeviceToDevice, xs));
                return SS_OK;
            };
            rc = run_affine_sharded(ctx, sh, aff, world, eps, max_iter, k_topics, exchange, exchange_sums, iters_out);
        } else {
            rc = run_pipelined(ctx, sh, max_iter, exchange, iters_out, k0);
        }
    }
    // assemble [K][N] by original id
    const uint64_t n = shards[0]->n;
    for (int s = 0; s < world && rc == SS_OK && affine; s++) {
        const size_t n_rows = (size_t)shards[s]->cnt_nd + shards[s]->cnt_d;
        std::vector<uint32_t> ids(n_rows);
        std::vector<double> part((size_t)k_topics * n_rows);
        rc = local_ids(sh[s].blk[0], ids.data());
        if (rc == SS_OK && n_rows) {
            if (hipMemcpyAsync(part.data(), aff[s].out.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess)
                rc = ctx->fail(SS_ERR_HIP, "ss_pagerank_run_group: copy of the ranks failed");
        }
        for (int k = 0; k < k_topics && rc == SS_OK; k++)
            for (size_t i = 0; i < n_rows; i++) rank_out[(size_t)k * n + ids[i]] = part[(size_t)k * n_rows + i];
    }
    for (int s = 0; s < world && rc == SS_OK && !affine; s++) {
        const size_t n_rows = (size_t)shards[s]->cnt_nd + shards[s]->cnt_d;
        std::vector<uint32_t> ids(n_rows);
        for (int b = 0; b < B && rc == SS_OK; b++) {
            const int kb = k0[b + 1] - k0[b];
            std::vector<double> part((size_t)kb * n_rows);
            rc = ss_pr_read_local(sh[s].blk[b], ids.data(), part.data());
            if (rc != SS_OK) break;
            for (int k = 0; k < kb; k++)
                for (size_t i = 0; i < n_rows; i++) rank_out[(size_t)(k0[b] + k) * n + ids[i]] = part[(size_t)k * n_rows + i];
        }
    }
    for (auto& s : sh)
        for (ss_pr* pr : s.blk) ss_pr_destroy(pr);
    return rc;
}

int32_t ss_pagerank_run(ss_graph* g, double damping, double eps, int32_t max_iter, int32_t k_topics,
                        const int32_t* n_topic, double* rank_out, int32_t* iters_out) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (g->world != 1) return ctx->fail(SS_ERR_STATE, "ss_pagerank_run: needs a (rank 0, world 1) graph");
    if (k_topics < 1 || k_topics > SS_MAX_TOPICS || !n_topic || !rank_out)
        return ctx->fail(SS_ERR_INVALID, "ss_pagerank_run: bad k_topics / NULL argument");
    SS_TRY(check_eps(ctx, "ss_pagerank_run", eps, max_iter));
    if (ctx->opt("pr.affine", 0) != 0) return run_affine(g, damping, eps, max_iter, k_topics, n_topic, rank_out, iters_out);
    // topics are independent power iterations (pagerank.go:54-63): run them MAXK at a time
    for (int k0 = 0; k0 < k_topics; k0 += MAXK) {
        const int kk = std::min(MAXK, k_topics - k0);
        ss_pr* pr = nullptr;
        SS_TRY(ss_pr_create(g, damping, eps, max_iter, kk, n_topic + k0, &pr));
        int32_t rc = ss_pr_begin(pr);
        int32_t n_active = kk, sweeps = 0;
        // the stop rule lives on the device; the host only looks every BATCH sweeps
        // (launches after convergence are no-ops)
        const int BATCH = 8;
        while (rc == SS_OK && n_active > 0) {
            int todo = BATCH;
            if (max_iter > 0) todo = std::min(BATCH, std::max(1, max_iter - sweeps));
            // (a fixed-iteration run: nothing reads ranks or the L1 change between the batches, and max_iter keeps its last two sweeps full)
            rc = ss::pr_step(pr, todo, eps < 0.0 ? 0 : 2);
            if (rc == SS_OK) rc = ss_pr_status(pr, iters_out ? iters_out + k0 : nullptr, &n_active, &sweeps, nullptr, nullptr);
        }
        if (rc == SS_OK) rc = ss_pr_read(pr, rank_out + (size_t)k0 * g->n);
        ss_pr_destroy(pr);
        if (rc != SS_OK) return rc;
    }
    return SS_OK;
}

}  // extern "C"
