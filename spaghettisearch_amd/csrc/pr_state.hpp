// pr_state.hpp — the PageRank state and everything of the PageRank path that crosses a translation unit: pagerank.hip (the small
// kernels, the choice of the sweep kernel, ss_pr_create and the ss_pr_* stepping API), the sweep-kernel families pr_sweep.hip,
// pr_sweep_n.hip and pr_step.hip (each behind one launcher and one occupancy query, below) and pagerank_run.hip (the one-call drivers
// ss_pagerank_run*, the two-vector kernels, float32 on the wire).  The device helpers the kernels share are in pr_device.hpp.  The
// work items and their constants (WorkItem, W_* / V_*, TPB, WAVES, CH, SEGW) come from pr_plan.hpp, which has to stay free of
// device headers.  The kernel-side types live in an anonymous namespace, like
// score_common.hpp's: every translation unit has its own copy of the device code.
#pragma once
#include "graph.hpp"
#include "pr_plan.hpp"

#ifdef SS_PR_WAVETIME
#include <cstdio>
#include <cstdlib>
#include <string>
#endif

namespace {

constexpr int MAXK = 16;

struct PrCtl {
    double S[MAXK];       // normaliser (`totalValue`) for the next sweep
    double delta[MAXK];   // last L1 change
    double csum[MAXK];    // last contribution sum (diagnostics)
    double xz[MAXK];      // rank of EVERY row without in-edges (they all share one value per topic)
    double xz_in[MAXK];   // topic-sensitive teleport only: that rank for the rows INSIDE the topic's teleport set (xz: outside)
    double tele[MAXK];    // two-vector form only ("pr.affine"): the teleport of each COLUMN for the next sweep
    int32_t active[MAXK];
    int32_t iters[MAXK];
    int32_t sweep;        // sweeps completed
    int32_t n_active;
    uint32_t ticket;      // last-group arrival counter
    uint32_t stuck;       // k_pr_multi_n: a wait between two sweeps ran out of patience (the grid was not resident): the state is void
    uint32_t gticket[8];  // last-block-of-a-group arrival counters
};

// The two-vector form of the reference's recurrence (option "pr.affine", opt-in; DESIGN K1b).  Every topic of pagerank.go:85-124 runs
// the SAME linear map on the same graph and differs only in its start value u_k = 1/n_k (:104); with x = (p*u + q) / (r*u + s)
// elementwise (p, q vectors over the nodes, r, s scalars) one iteration maps (p, q, r, s) to
//     p' = M p + tau*r*1,  q' = M q + tau*s*1,  r' = W p + tau*N*r,  s' = W q + tau*N*s        (M: the inherited part, W: the sum of
// the contributions, tau = 1 - d; iteration 1 adds the start vector: p += 1) — so TWO vectors carry every topic, whatever K is.
// The state is kept scaled to r + s = 1.  Per-topic ranks, L1 changes and stop decisions are evaluated from (p, q, r) by streaming
// kernels; a topic's ranks are written out in the iteration it stops.  Not the reference's float64 operation order: ranks agree
// with the oracle to ~1e-13, iteration counts where the stop rule is not at a rounding tie.
constexpr int AFF_MAXK = 256;
constexpr unsigned AFF_NB = 512;  // blocks of k_aff_delta (their partial sums are added in a fixed order)
struct AffCtl {
    double u[AFF_MAXK];       // 1 / n_topic
    double delta[AFF_MAXK];   // last L1 change of the topic
    int32_t active[AFF_MAXK], iters[AFF_MAXK], just[AFF_MAXK];   // just: stopped in the iteration that has just been evaluated
    double r_x, r_prev, r_next;      // r of the stored vectors, of the previous ones, of the next sweep's result
    double s_x, s_prev, s_next;      // ... and s (the state is kept scaled to r + s = 1: s alone vanishes when d = 1)
    double xz_prev[2];               // the edge-less rows' (p, q) before the last sweep
    int32_t n_active, n_just, k_real, it;
};

struct PrParams {
    const uint32_t* in_ptr;
    const uint32_t* in_src;
    const uint32_t* outdeg;
    double* x;
    const double* tab_rd[2];
    double* tab_wr[2];
    const WorkItem* work;
    double* partials;     // [nblocks][2][GW]
    double* segpart;      // [nsegs][GW]
    uint32_t* rowticket;  // [n multi-segment rows]
    double* hubsum;       // [n multi-segment rows][2][GW]: the L1 change and the next contribution of each such row, added in row order behind the blocks' sums
    uint32_t nmulti;      // multi-segment rows
    PrCtl* ctl;
    const double* x0;     // [GW] 1/n_topic
    double d, teleport, eps, tele_n;
    int32_t max_iter, k_topics, world;
    uint32_t sl_nd, cnt_nd, sl_d, cnt_d, seg_edges, n_items;
    uint32_t pos_nd, pos_d;   // rows WITH in-edges per class (they come first: rows are in-degree sorted)
    // opt-in true topic-sensitive teleport (ss_pr_set_teleport; null = the reference's uniform teleport):
    const uint32_t* memb;     // [n_local] bit k: the row's node is in topic k's teleport set
    const double* tin;        // [MAXK] teleport of a member: (1-d) * N / |set_k|
    const double* nz_in;      // [MAXK] rows without in-edges (this rank) inside topic k's set
    uint32_t ts_mask;         // bit k: topic k has a teleport set (others keep the uniform teleport)
    uint32_t zrow;            // index of the table's all-zero row (= nd_int): where the unused slots of a chunk gather from
    const uint32_t* woff;     // k_pr_sweep: [waves][8]: wave w's items of class c are work[woff[8w+c] .. woff[8w+c+1])
    uint32_t stagger_div;     // k_pr_sweep: blocks per arrival round (= CUs); 0 = every block walks the classes in the same order
    uint32_t stagger_code;    // start classes of the rounds as base-6 digits (0 = round r starts at position r of the class order)
    uint32_t class_order;     // k_pr_sweep: the order in which a wave walks its six work classes, 3 bits per position
    uint32_t n_order;         // k_pr_sweep_n: the order of its four phases, 2 bits per position
    double* x_alt;            // two-vector form: sweep s reads x (s even) / x_alt (s odd) and writes the other one; null otherwise
    AffCtl* aff;              // two-vector form ("pr.affine"): its control block; null otherwise
    const double* tele_col;   // ... and the per-column teleport (ctl->tele); null = the uniform p.teleport
    // shared rows of the edge-less sources (option "pr.share_zero_rows", k_pr_sweep<GW, false> only; pr_plan.hpp: SharedRows)
    const uint32_t* sh_deg;   // [n_shared] the distinct out-degrees of the non-dangling rows without in-edges, rising
    uint32_t n_shared;        // shared rows: table rows zrow + 1 .. zrow + n_shared
    uint32_t share;           // 1: the table ends at pos_nd (+ zero row + shared rows) and in_src is the state's remapped copy
    uint32_t tab_rows;        // rows of the table that belong to a local row of their own (share: pos_nd, otherwise sl_nd)
    // the lean sweep (option "pr.lean_sweeps", k_pr_sweep<GW, false, true> only; pr_plan.hpp: LeanPlan)
    const uint32_t* woff_lean; // [waves][8] as woff, into the work table's second part: the same walk without the dangling rows' items
};

}  // namespace

// the sweep-kernel families: which one a state runs is decided once, in ss_pr_create (pagerank.hip: pick_kernel)
enum PrKernel : int {
    PR_STEP = 0,           // k_pr_step: block items, K <= 2 by option only
    PR_SWEEP = 1,          // k_pr_sweep: wave items, lane groups of 8 / 16 topics
    PR_SWEEP_N = 2,        // k_pr_sweep_n (and its persistent form k_pr_multi_n): wave items, K <= 2 unpadded
};

struct ss_pr {
    ss_graph* g = nullptr;
    PrKernel kernel = PR_SWEEP;
    int gw = 1;            // lane-group width = padded topic count
    ss::DevBuf<float> wire_send, wire_recv;   // option "pr.wire_f32": the contribution slice as float32 on the wire
    bool nwave = false;    // K <= 2 on the wave-item kernel k_pr_sweep_n (gw = K; the work items are those of the 8-wide sweep)
    int persist_mode = 1;  // 1: write-through hand-offs, 2: release / acquire fences around the wait
    bool persist = false;  // ... with ss_pr_step's sweeps inside ONE launch (k_pr_multi_n): small graphs, whose sweep is mostly fixed cost
    int k = 1;
    PrParams prm{};
    unsigned nblocks = 0;
    ss::DevBuf<double> x, tab0, tab1, send, partials, segpart, hubsum, x0;
    ss::DevBuf<uint32_t> rowticket;
    ss::DevBuf<uint32_t> memb;          // topic-sensitive teleport (optional)
    ss::DevBuf<double> tin, nz_in;
    ss::DevBuf<WorkItem> work;
    ss::DevBuf<uint32_t> woff;          // k_pr_sweep: per-wave class offsets into work
    ss::DevBuf<uint32_t> src_shared;    // "pr.share_zero_rows": the state's copy of in_src, sources without in-edges -> their shared row
    ss::DevBuf<uint32_t> sh_deg;        // ... and the shared rows' out-degrees
    ss::DevBuf<uint32_t> woff_lean;     // "pr.lean_sweeps": the lean walk's per-wave class offsets (its items stand behind the others in `work`)
    bool lean = false;                  // ... the state has a lean walk: k_pr_sweep on one rank, option on (ss::pr_step decides per sweep)
    int64_t sweeps_enq = 0;             // sweeps enqueued since ss_pr_begin (the host's count: what a lean launch is decided from)
    int64_t n_lean = 0;                 // ... of them launched lean (ss_pr_lean_sweeps)
    ss::DevBuf<PrCtl> ctl;
    bool begun = false;
    bool need_finalize = false;   // world>1: a begin/step is waiting for its exchange + finalize
    bool finalize_is_begin = false;
};

// (hidden: these cross translation units, not the library's boundary — the exported symbols stay those of include/spaghetti_rank.h)
#pragma GCC visibility push(hidden)
namespace ss {
// pagerank.hip: launchers of its kernels; the kernel for the state's lane-group width (and teleport sets) is picked inside
unsigned begin_blocks(const ss_pr* pr);                            // grid of k_pr_begin
void pr_launch_begin(ss_pr* pr, hipStream_t st, unsigned nb);
void pr_launch_step(ss_pr* pr, hipStream_t st, bool lean = false); // one sweep: the one place that switches on pr->kernel
// n_steps sweeps on the context's stream, as ss_pr_step (which is this with full_tail = 2).  A state in fixed-iteration mode runs
// the sweeps whose ranks and L1 change no caller can see lean: all but the last `full_tail` of the call and the last two before
// max_iter.  ss_pagerank_run passes 0: between its batches it reads neither, and max_iter ends its run.
int32_t pr_step(ss_pr* pr, int32_t n_steps, int32_t full_tail);
void pr_launch_finalize(ss_pr* pr, hipStream_t st, int is_begin);  // world > 1: behind the exchange
// The sweep-kernel families, one file each: a launcher of one sweep over pr->nblocks blocks, which picks the instantiation for the
// state's width, teleport sets and mode itself, and the blocks per CU the runtime admits of the family's kernel of width gw
// (unclamped; pagerank.hip asks once per kernel and process and keeps the answer)
void pr_sweep_launch(ss_pr* pr, hipStream_t st, bool lean);        // pr_sweep.hip: k_pr_sweep<8|16, TS, LEAN>
int pr_sweep_occupancy(int gw);
void pr_sweep_n_launch(ss_pr* pr, hipStream_t st);                 // pr_sweep_n.hip: k_pr_sweep_n<1|2, TS>
int pr_sweep_n_occupancy(int gw);
void pr_multi_n_launch(ss_pr* pr, hipStream_t st, int n_steps);    // ... and k_pr_multi_n<1|2, 1|2>: n_steps sweeps in one launch
int pr_multi_n_occupancy(int gw);
void pr_step_launch(ss_pr* pr, hipStream_t st);                    // pr_step.hip: k_pr_step<1|2>
int pr_step_occupancy(int gw);
#ifdef SS_PR_WAVETIME
void pr_dump_wave_times(const ss_pr* pr);                          // pr_sweep.hip (variant build): called by ss_pr_destroy
#endif
// pagerank_run.hip: float32 on the wire (option "pr.wire_f32")
size_t pr_wire_floats(const ss_pr* pr);
hipError_t pr_wire_alloc(ss_pr* pr);
void pr_wire_pack(ss_pr* pr, hipStream_t st);
void pr_wire_unpack(ss_pr* pr, hipStream_t st);
}  // namespace ss
#pragma GCC visibility pop

namespace {
#ifdef SS_PR_WAVETIME
// the variant build's two dumps go to the directory the environment names in SS_PR_WAVETIME_DIR (default: the working directory)
inline FILE* open_dump(const char* name) {
    const char* dir = getenv("SS_PR_WAVETIME_DIR");
    return fopen((std::string(dir && *dir ? dir : ".") + "/" + name).c_str(), "w");
}
#endif
// The state's control block, read back into the context's pinned scratch (a read-back into pageable memory pins the page per call:
// ss_ctx::h_pin); waits for `st`, bounded where a collective may be in flight.  `what` names the wait in the error.
inline int32_t read_ctl(ss_ctx* ctx, const ss_pr* pr, hipStream_t st, const char* what, const PrCtl** out) {
    ctx->pin_used = 0;
    PrCtl* const hp = ctx->pin<PrCtl>();
    if (hipMemcpyAsync(hp, pr->ctl.p, sizeof(PrCtl), hipMemcpyDeviceToHost, st) != hipSuccess) return ctx->fail(SS_ERR_HIP, "%s: status read failed", what);
    SS_TRY(ss::sync_bounded(ctx, st, what));
    *out = hp;
    return SS_OK;
}
}  // namespace
