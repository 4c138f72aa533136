// field_stats.hip — ss_field_stats and ss_field_histogram: the smallest and largest value, the exact sum and the number of missing values
// of a doc field, and the matches per bin of a field, over ALL docs a query matches.  DESIGN.md K4z; no reference counterpart.
//
// M(q) is ss_facet_counts' match set, formed by the code that call uses (match_set.hpp).  Both walks give a workgroup a RUN of
// consecutive 32768-doc blocks of one query and form the match words per block (match_set.hpp, steps 1 to 3, warm bounds along the run).
//
// k_field_stats<NF> gathers value[field][d] of every set bit for NF asked fields.  A thread keeps min, max, the 128-bit sum (a low word
// with carry, a high word) and the missing count per field in registers; the waves reduce them by shuffles, the workgroup through LDS,
// and one partial ss_field_stat per field goes to the scratch row [query of the group][run][field].  k_field_stats_merge, one thread
// per (query, field), folds the R partials and writes the output; launched without a query table it writes the identity entry and
// n_match 0 of every query first, which the queries without a list keep.  No atomics, and min, max and the two's complement sum are
// associative and exact: no order can show.
//
// k_field_hist<LDS, MODE> has k_group_count's shape with the bin computed from the gathered value (field_stats_plan.hpp: a shift, the
// host's reciprocal, `/`, or a search over the edges).  A thread walks its 128 docs in ascending order and merges consecutive equal bins
// into one add.  The adds go to a histogram in LDS that joins the query's counter row at the end of the run (n_bins at most
// "fstats.lds_bins"), or straight to the row by non-returning global atomics; below, above and missing stay in registers.  The row's
// four extra slots take them and the run's matches.  k_field_hist_out copies the rows and tails of a group's queries out.  Integer
// atomics only.
#include "field_stats_plan.hpp"
#include "match_set.hpp"

namespace fp = ss::fstats;
namespace hw = ss::hitwin;
namespace ms = ss::mset;

static_assert(fp::NO_VALUE == SS_NO_FIELD_VALUE && fp::MAX_STAT_FIELDS == SS_MAX_DOC_FIELDS && fp::MAX_HIST_BINS == SS_MAX_HIST_BINS,
              "field_stats_plan.hpp restates the ABI's limits");
static_assert(sizeof(ss_field_stat) == fp::STAT_BYTES && sizeof(ss_hist_tail) == 16, "ss_field_stat / ss_hist_tail layout");

namespace {

constexpr int FS_TPB = (int)ms::THREADS;
constexpr int FS_WPT = (int)ms::WORDS_PER_THREAD;
constexpr int FS_WAVES = FS_TPB / 64;
enum { MODE_SHIFT = 0, MODE_RECIPROCAL = 1, MODE_DIVIDE = 2, MODE_EDGES = 3 };

struct StatsParams {
    ss::MatchSetArgs match;
    const int64_t* col[fp::MAX_STAT_FIELDS];   // the asked fields' columns [n_docs]
    uint32_t n_blocks, R;
    uint32_t a0, n_group, run0;       // this launch: active queries [a0, a0 + n_group), runs from run0
    ss_field_stat* part;              // [n_group][R][NF]
};

struct StatsMergeParams {
    const uint32_t* aq;               // [n_active] the queries that have a list; NULL: the identity entries of queries [0, n_group)
    const ss_field_stat* part;
    uint32_t R, nf, a0, n_group;
    ss_field_stat* stats_out;         // [n_q][nf]
    uint32_t* n_match_out;            // [n_q], nullable
};

struct HistParams {
    ss::MatchSetArgs match;
    const int64_t* col;               // [n_docs]
    const int64_t* edges;             // [n_bins + 1], MODE_EDGES
    fp::Binner bin;
    uint32_t n_blocks, R, n_bins;
    uint32_t a0, n_group, run0;
    uint32_t edges_lds;               // MODE_EDGES: the edges are copied to LDS behind the histogram
    uint64_t stride;                  // words of a counter row
    uint32_t* rows;                   // [n_group][stride], zeroed
};

struct HistOutParams {
    const uint32_t* aq;
    const uint32_t* rows;
    uint64_t stride;
    uint32_t n_bins, a0;
    uint32_t* counts_out;             // [n_q][n_bins], zeroed
    ss_hist_tail* tails_out;          // [n_q], zeroed; nullable
};

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o, 64); }
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) { return (uint64_t)__shfl_xor((unsigned long long)v, o, 64); }

// Grid: blockIdx.x = (run - run0) * n_group + query, as k_group_count.
template <int NF>
__global__ __launch_bounds__(FS_TPB) void k_field_stats(StatsParams p) {
    __shared__ uint64_t cur[ms::MAX_LISTS][2];                               // each list's run in this block: [first, end)
    __shared__ __attribute__((aligned(16))) uint32_t img[ms::BLOCK_WORDS];   // the block's docs with a posting of the query
    __shared__ ss_field_stat wpart[FS_WAVES][NF];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.match.lptr[a], nl = p.match.lptr[a + 1] - l0;      // 1 .. MAX_LISTS (the host leaves out a query without lists)
    const uint32_t b0 = ms::run_begin(r, p.R, p.n_blocks), b1 = ms::run_begin(r + 1, p.R, p.n_blocks);
    int64_t mn[NF], mx[NF], hi[NF];
    uint64_t lo[NF];
    uint32_t miss[NF], matches = 0;                                          // of this thread's words, over the run
#pragma unroll
    for (int f = 0; f < NF; f++) {
        mn[f] = INT64_MAX;
        mx[f] = INT64_MIN;
        hi[f] = 0;
        lo[f] = 0;
        miss[f] = 0;
    }
    for (uint32_t blk = b0; blk < b1; blk++) {
        // ---- 1 to 3. the block's match words (match_set.hpp)
        if (blk == b0) ms::runs_cold(p.match, l0, nl, blk, cur);
        else ms::runs_warm(p.match, l0, nl, blk, cur);
        if (!ms::or_image(p.match, l0, nl, blk, cur, img)) continue;         // no list reaches the block
        const uint64_t w0 = ms::word_begin(blk);                             // this thread's first word
        uint32_t m[FS_WPT];
        matches += ms::and_allowed(m, p.match, a, blk, img);
        // ---- 4. the values of the set bits
#pragma unroll
        for (int i = 0; i < FS_WPT; i++) {
            uint32_t bits = m[i];
            while (bits) {
                const uint32_t d = (uint32_t)((w0 + i) * 32) + (uint32_t)(__ffs(bits) - 1);      // < n_docs < 2^32
                bits &= bits - 1;
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    const int64_t v = p.col[f][d];
                    if (v == fp::NO_VALUE) {
                        miss[f]++;
                        continue;
                    }
                    mn[f] = v < mn[f] ? v : mn[f];
                    mx[f] = v > mx[f] ? v : mx[f];
                    lo[f] += (uint64_t)v;                                    // v sign-extended to 128 bits joins hi : lo
                    hi[f] += (v >> 63) + (lo[f] < (uint64_t)v ? 1 : 0);
                }
            }
        }
    }
    // ---- the run's partial entries: the waves by shuffles, the workgroup through LDS
    matches = ms::wave_sum(matches);
#pragma unroll
    for (int f = 0; f < NF; f++) {
        miss[f] = ms::wave_sum(miss[f]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t omn = shfl_xor_i64(mn[f], o), omx = shfl_xor_i64(mx[f], o), ohi = shfl_xor_i64(hi[f], o);
            const uint64_t olo = shfl_xor_u64(lo[f], o);
            mn[f] = omn < mn[f] ? omn : mn[f];
            mx[f] = omx > mx[f] ? omx : mx[f];
            lo[f] += olo;
            hi[f] += ohi + (lo[f] < olo ? 1 : 0);
        }
        if ((tid & 63) == 0) wpart[tid >> 6][f] = ss_field_stat{mn[f], mx[f], lo[f], hi[f], matches - miss[f], miss[f]};
    }
    __syncthreads();
    if (tid < NF) {
        ss_field_stat t = wpart[0][tid];
#pragma unroll
        for (int w = 1; w < FS_WAVES; w++) {
            const ss_field_stat o = wpart[w][tid];
            t.min = o.min < t.min ? o.min : t.min;
            t.max = o.max > t.max ? o.max : t.max;
            t.sum_lo += o.sum_lo;
            t.sum_hi += o.sum_hi + (t.sum_lo < o.sum_lo ? 1 : 0);
            t.count += o.count;
            t.missing += o.missing;
        }
        p.part[((uint64_t)al * p.R + r) * NF + tid] = t;
    }
}

// Grid: one thread per (query of the group, field).  aq NULL: the identity entry of every query [0, n_group).
__global__ __launch_bounds__(FS_TPB) void k_field_stats_merge(StatsMergeParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * FS_TPB + threadIdx.x;
    if (i >= (uint64_t)p.n_group * p.nf) return;
    const uint32_t al = (uint32_t)(i / p.nf), f = (uint32_t)(i % p.nf);
    ss_field_stat t{INT64_MAX, INT64_MIN, 0, 0, 0, 0};
    uint32_t q = al;
    if (p.aq) {
        q = p.aq[p.a0 + al];
        for (uint32_t r = 0; r < p.R; r++) {
            const ss_field_stat o = p.part[((uint64_t)al * p.R + r) * p.nf + f];
            t.min = o.min < t.min ? o.min : t.min;
            t.max = o.max > t.max ? o.max : t.max;
            t.sum_lo += o.sum_lo;
            t.sum_hi += o.sum_hi + (t.sum_lo < o.sum_lo ? 1 : 0);
            t.count += o.count;
            t.missing += o.missing;
        }
    }
    p.stats_out[(uint64_t)q * p.nf + f] = t;
    if (f == 0 && p.n_match_out) p.n_match_out[q] = t.count + t.missing;
}

struct LdsEdges {                     // the edges where the search reads them
    const int64_t* e;
    __device__ __forceinline__ int64_t operator[](uint32_t i) const { return e[i]; }
};

// Grid: blockIdx.x = (run - run0) * n_group + query.  Dynamic LDS: the histogram, n_bins counters rounded up to four (LDS), then the
// edges (edges_lds).
template <bool LDS, int MODE>
__global__ __launch_bounds__(FS_TPB) void k_field_hist(HistParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fs_dyn[];
    __shared__ uint64_t cur[ms::MAX_LISTS][2];
    __shared__ __attribute__((aligned(16))) uint32_t img[ms::BLOCK_WORDS];
    __shared__ uint32_t wsum[FS_WAVES][fp::TAIL_SLOTS];
    const int tid = threadIdx.x;
    const uint32_t al = blockIdx.x % p.n_group, r = p.run0 + blockIdx.x / p.n_group, a = p.a0 + al;
    const uint32_t l0 = p.match.lptr[a], nl = p.match.lptr[a + 1] - l0;
    const uint32_t b0 = ms::run_begin(r, p.R, p.n_blocks), b1 = ms::run_begin(r + 1, p.R, p.n_blocks);
    const uint32_t nb = p.n_bins;
    uint32_t* const row = p.rows + (uint64_t)al * p.stride;
    uint32_t* const hist = fs_dyn;
    int64_t* const lds_edges = reinterpret_cast<int64_t*>(fs_dyn + (LDS ? fp::hist_lds_bytes(nb) / sizeof(uint32_t) : 0));   // 16-byte aligned
    if (LDS) {
        for (uint32_t i = tid; i < nb; i += FS_TPB) hist[i] = 0u;            // (the barrier of step 2 stands before the first add)
    }
    if (MODE == MODE_EDGES && p.edges_lds) {
        for (uint32_t i = tid; i <= nb; i += FS_TPB) lds_edges[i] = p.edges[i];                  // (likewise before the first search)
    }
    uint32_t matches = 0, below = 0, above = 0, missing = 0;                 // of this thread's words, over the run
    const auto add = [&](uint32_t slot, uint32_t len) {
        if (slot < nb) {
            if (LDS) atomicAdd(&hist[slot], len);
            else atomicAdd(&row[slot], len);
        } else {
            below += slot == fp::slot_below(nb) ? len : 0u;
            above += slot == fp::slot_above(nb) ? len : 0u;
            missing += slot == fp::slot_missing(nb) ? len : 0u;
        }
    };
    for (uint32_t blk = b0; blk < b1; blk++) {
        // ---- 1 to 3. the block's match words (match_set.hpp)
        if (blk == b0) ms::runs_cold(p.match, l0, nl, blk, cur);
        else ms::runs_warm(p.match, l0, nl, blk, cur);
        if (!ms::or_image(p.match, l0, nl, blk, cur, img)) continue;
        const uint64_t w0 = ms::word_begin(blk);
        uint32_t m[FS_WPT];
        matches += ms::and_allowed(m, p.match, a, blk, img);
        // ---- 4. the bins of the set bits, ascending by doc: consecutive equal bins become one add
        uint32_t run_slot = fp::slot_missing(nb), run_len = 0;
#pragma unroll
        for (int i = 0; i < FS_WPT; i++) {
            uint32_t bits = m[i];
            while (bits) {
                const uint32_t d = (uint32_t)((w0 + i) * 32) + (uint32_t)(__ffs(bits) - 1);      // < n_docs < 2^32
                bits &= bits - 1;
                const int64_t v = p.col[d];
                uint32_t slot;
                if (MODE == MODE_EDGES) slot = p.edges_lds ? fp::bin_edges(LdsEdges{lds_edges}, nb, v) : fp::bin_edges(p.edges, nb, v);
                else if (MODE == MODE_DIVIDE) slot = fp::bin_fixed<fp::DIV_PLAIN>(p.bin, v);
                else if (MODE == MODE_SHIFT) slot = fp::bin_fixed<fp::DIV_SHIFT>(p.bin, v);
                else slot = fp::bin_fixed<fp::DIV_RECIPROCAL>(p.bin, v);
                if (slot == run_slot) {
                    run_len++;
                    continue;
                }
                add(run_slot, run_len);
                run_slot = slot;
                run_len = 1;
            }
        }
        add(run_slot, run_len);
    }
    // ---- the run's histogram and its four totals join the row
    below = ms::wave_sum(below);
    above = ms::wave_sum(above);
    missing = ms::wave_sum(missing);
    matches = ms::wave_sum(matches);
    if ((tid & 63) == 0) {
        wsum[tid >> 6][0] = below;
        wsum[tid >> 6][1] = above;
        wsum[tid >> 6][2] = missing;
        wsum[tid >> 6][3] = matches;
    }
    __syncthreads();
    if (LDS) {
        for (uint32_t i = tid; i < nb; i += FS_TPB) {
            const uint32_t c = hist[i];
            if (c) atomicAdd(&row[i], c);
        }
    }
    if (tid < (int)fp::TAIL_SLOTS) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < FS_WAVES; w++) v += wsum[w][tid];
        if (v) atomicAdd(&row[nb + tid], v);                                 // slot_below, slot_above, slot_missing, slot_match
    }
}

// Grid: one workgroup per active query of the group.
__global__ __launch_bounds__(FS_TPB) void k_field_hist_out(HistOutParams p) {
    const uint32_t al = blockIdx.x, q = p.aq[p.a0 + al];
    const uint32_t* const row = p.rows + (uint64_t)al * p.stride;
    uint32_t* const out = p.counts_out + (uint64_t)q * p.n_bins;
    for (uint32_t i = threadIdx.x; i < p.n_bins; i += FS_TPB) out[i] = row[i];
    if (threadIdx.x == 0 && p.tails_out)
        p.tails_out[q] = ss_hist_tail{row[fp::slot_below(p.n_bins)], row[fp::slot_above(p.n_bins)], row[fp::slot_missing(p.n_bins)],
                                      row[fp::slot_match(p.n_bins)]};
}

template <int NF>
void launch_stats(const StatsParams& sp, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_field_stats<NF>, dim3(grid), dim3(FS_TPB), 0, st, sp);
}

template <bool LDS>
void launch_hist(int mode, const HistParams& hp, uint32_t grid, uint32_t lds, hipStream_t st) {
    if (mode == MODE_SHIFT) hipLaunchKernelGGL((k_field_hist<LDS, MODE_SHIFT>), dim3(grid), dim3(FS_TPB), lds, st, hp);
    else if (mode == MODE_RECIPROCAL) hipLaunchKernelGGL((k_field_hist<LDS, MODE_RECIPROCAL>), dim3(grid), dim3(FS_TPB), lds, st, hp);
    else if (mode == MODE_DIVIDE) hipLaunchKernelGGL((k_field_hist<LDS, MODE_DIVIDE>), dim3(grid), dim3(FS_TPB), lds, st, hp);
    else hipLaunchKernelGGL((k_field_hist<LDS, MODE_EDGES>), dim3(grid), dim3(FS_TPB), lds, st, hp);
}

int32_t field_stats_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id, const QueryConstraints& cons,
                         const QueryRanges& ranges, int32_t n_stat_fields, const int32_t* fields, ss_field_stat* stats_out, uint32_t* n_match_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_field_stats";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = fp::check_stats_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, stats_out != nullptr, n_stat_fields, fields != nullptr, nullptr,
                                            s->n_fields))
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    int32_t h_fields[fp::MAX_STAT_FIELDS] = {0, 0, 0, 0};
    SS_HIP(ctx, ss::copy_in(ctx->stream, h_fields, fields, (size_t)n_stat_fields * sizeof(int32_t)));
    if (const int rc = fp::check_stats_args(msg, sizeof(msg), entry, n_q, true, true, n_stat_fields, true, h_fields, s->n_fields))
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    const size_t nq = (size_t)n_q;
    const uint32_t nf = (uint32_t)n_stat_fields;
    ss::MatchCall mc;
    SS_TRY(ss::open_match_call(s, entry, n_q, q_ptr, q_terms, mask_id, cons, ranges, &mc));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[mc.as.turn];
    const bool dev_out = ss::on_device(stats_out) && (!n_match_out || ss::on_device(n_match_out));
    ss_field_stat* d_stats = stats_out;
    uint32_t* d_match = n_match_out;
    const size_t o_match = nq * nf * sizeof(ss_field_stat), out_bytes = o_match + nq * sizeof(uint32_t);
    if (!dev_out) {                                 // the scorer's block: stats | n_match
        SS_HIP(ctx, ensure(s->d_fstats_out, out_bytes));
        d_stats = reinterpret_cast<ss_field_stat*>(s->d_fstats_out.p);
        d_match = reinterpret_cast<uint32_t*>(s->d_fstats_out.p + o_match);
    }
    // every block the call needs is there before the first write to an output: a failure leaves the outputs as they were
    const uint32_t n_active = (uint32_t)mc.ml.aq.size(), n_blocks = ms::blocks(s->n_docs);
    const bool walk = n_active && n_blocks;
    const uint32_t R = ms::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("fstats.runs", 0));
    const uint32_t group = fp::group_queries(n_active, fp::stats_query_bytes(R, nf), fp::scratch_bytes_of(ctx->opt("fstats.scratch_bytes", 0)));
    ss::MatchTables mt;
    if (walk) {
        SS_HIP(ctx, ensure(s->d_fstats_part, (size_t)group * fp::stats_query_bytes(R, nf)));
        SS_TRY(ss::stage_match_tables(s, mc, nullptr, 0, &mt));
    }
    StatsMergeParams mp{};
    mp.nf = nf;
    mp.n_group = (uint32_t)n_q;
    mp.stats_out = d_stats;
    mp.n_match_out = d_match;
    // a query without a list keeps these identity entries; every other query's entries are written by its merge
    hipLaunchKernelGGL(k_field_stats_merge, dim3((uint32_t)ss::div_up(nq * nf, FS_TPB)), dim3(FS_TPB), 0, st, mp);
    if (walk) {
        StatsParams sp{};
        sp.match = mt.args;
        for (uint32_t f = 0; f < nf; f++) sp.col[f] = s->fields.p + (size_t)h_fields[f] * s->n_docs;
        sp.n_blocks = n_blocks;
        sp.R = R;
        sp.part = reinterpret_cast<ss_field_stat*>(s->d_fstats_part.p);
        mp.aq = mt.aq;
        mp.part = sp.part;
        mp.R = R;
        for (const ms::Group& g : ms::groups(n_active, group)) {                // one group after another: they share the partial entries
            sp.a0 = mp.a0 = g.first;
            sp.n_group = mp.n_group = g.count;
            for (const ms::Launch& l : ms::launches(R, g.count)) {
                sp.run0 = l.first;
                const uint32_t grid = l.count * g.count;
                if (nf == 1) launch_stats<1>(sp, grid, st);
                else if (nf == 2) launch_stats<2>(sp, grid, st);
                else if (nf == 3) launch_stats<3>(sp, grid, st);
                else launch_stats<4>(sp, grid, st);
            }
            hipLaunchKernelGGL(k_field_stats_merge, dim3((uint32_t)ss::div_up((size_t)g.count * nf, FS_TPB)), dim3(FS_TPB), 0, st, mp);
        }
    }
    SS_HIP(ctx, hipGetLastError());
    SS_HIP(ctx, turn.batch_ev.record(st));          // until here the call reads the turn's sets and tables
    if (dev_out) return SS_OK;                      // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    std::vector<unsigned char> h_out(out_bytes);
    SS_HIP(ctx, hipMemcpyAsync(h_out.data(), s->d_fstats_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    SS_HIP(ctx, hw::give_rows(stats_out, h_out.data(), nq, nf, sizeof(ss_field_stat), nullptr));
    if (n_match_out) SS_HIP(ctx, hw::give_rows(n_match_out, h_out.data() + o_match, nq, 1, sizeof(uint32_t), nullptr));
    return SS_OK;
}

int32_t field_histogram_impl(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                             const QueryConstraints& cons, const QueryRanges& ranges, int32_t field, int64_t origin, uint64_t width, const int64_t* edges,
                             int32_t n_bins, uint32_t* counts_out, ss_hist_tail* tails_out) {
    ss_ctx* ctx = s->ctx;
    const char* const entry = "ss_field_histogram";
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    char msg[256];
    if (const int rc = fp::check_hist_args(msg, sizeof(msg), entry, n_q, q_ptr != nullptr, counts_out != nullptr, field, width, edges != nullptr, nullptr,
                                           n_bins, s->n_fields))
        return ctx->fail(ss::plan_code(rc), "%s", msg);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t nb = (uint32_t)n_bins;
    std::vector<int64_t> h_edges;
    if (edges) {
        h_edges.resize((size_t)nb + 1);
        SS_HIP(ctx, ss::copy_in(ctx->stream, h_edges.data(), edges, h_edges.size() * sizeof(int64_t)));
        if (!fp::edges_ascending(h_edges.data(), nb)) return ctx->fail(SS_ERR_INVALID, "%s: edges are not strictly ascending", entry);
    }
    const size_t nq = (size_t)n_q;
    ss::MatchCall mc;
    SS_TRY(ss::open_match_call(s, entry, n_q, q_ptr, q_terms, mask_id, cons, ranges, &mc));
    // ---- nothing below refuses an argument
    hipStream_t st = ctx->stream;
    Turn& turn = s->turn[mc.as.turn];
    const bool dev_out = ss::on_device(counts_out) && (!tails_out || ss::on_device(tails_out));
    uint32_t* d_counts = counts_out;
    ss_hist_tail* d_tails = tails_out;
    const size_t o_tails = align16(nq * nb * sizeof(uint32_t)), out_bytes = o_tails + nq * sizeof(ss_hist_tail);
    if (!dev_out) {                                 // the scorer's block: counts | tails
        SS_HIP(ctx, ensure(s->d_fstats_out, out_bytes));
        d_counts = reinterpret_cast<uint32_t*>(s->d_fstats_out.p);
        d_tails = reinterpret_cast<ss_hist_tail*>(s->d_fstats_out.p + o_tails);
    }
    // every block the call needs is there before the first write to an output: a failure leaves the outputs as they were
    const uint32_t n_active = (uint32_t)mc.ml.aq.size(), n_blocks = ms::blocks(s->n_docs);
    const bool walk = n_active && n_blocks;
    const uint32_t R = ms::runs_per_query(n_blocks, n_active, (uint32_t)ctx->cu_count, ctx->opt("fstats.runs", 0));
    const bool use_lds = fp::use_lds(nb, ctx->opt("fstats.lds_bins", fp::DEFAULT_LDS_BINS));
    const uint64_t stride = fp::row_stride(nb);
    const uint32_t group = fp::group_queries(n_active, fp::hist_query_bytes(nb), fp::scratch_bytes_of(ctx->opt("fstats.scratch_bytes", 0)));
    ss::MatchTables mt;
    if (walk) {
        SS_HIP(ctx, ensure(s->d_fstats_part, (size_t)group * fp::hist_query_bytes(nb)));
        SS_TRY(ss::stage_match_tables(s, mc, edges ? h_edges.data() : nullptr, h_edges.size() * sizeof(int64_t), &mt));
    }
    // a query without a list keeps these zeros; every other query's rows are copied out behind its runs
    SS_HIP(ctx, hipMemsetAsync(d_counts, 0, nq * nb * sizeof(uint32_t), st));
    if (d_tails) SS_HIP(ctx, hipMemsetAsync(d_tails, 0, nq * sizeof(ss_hist_tail), st));
    if (walk) {
        HistParams hp{};
        hp.match = mt.args;
        hp.col = s->fields.p + (size_t)field * s->n_docs;
        hp.edges = reinterpret_cast<const int64_t*>(mt.extra);
        hp.bin = fp::make_binner(origin, edges ? 1 : width, nb);
        hp.n_blocks = n_blocks;
        hp.R = R;
        hp.n_bins = nb;
        hp.edges_lds = edges && fp::edges_in_lds(nb) ? 1u : 0u;
        hp.stride = stride;
        hp.rows = reinterpret_cast<uint32_t*>(s->d_fstats_part.p);
        HistOutParams op{};
        op.aq = mt.aq;
        op.rows = hp.rows;
        op.stride = stride;
        op.n_bins = nb;
        op.counts_out = d_counts;
        op.tails_out = d_tails;
        const int mode = edges ? MODE_EDGES : hp.bin.div.magic == 0 ? MODE_SHIFT : ctx->opt("fstats.plain_divide", 0) > 0 ? MODE_DIVIDE : MODE_RECIPROCAL;
        const uint32_t lds = (use_lds ? fp::hist_lds_bytes(nb) : 0u) + (hp.edges_lds ? fp::edges_lds_bytes(nb) : 0u);
        for (const ms::Group& g : ms::groups(n_active, group)) {                // one group after another: they share the counter rows
            hp.a0 = op.a0 = g.first;
            hp.n_group = g.count;
            SS_HIP(ctx, hipMemsetAsync(hp.rows, 0, (size_t)g.count * stride * sizeof(uint32_t), st));
            for (const ms::Launch& l : ms::launches(R, g.count)) {
                hp.run0 = l.first;
                if (use_lds) launch_hist<true>(mode, hp, l.count * g.count, lds, st);
                else launch_hist<false>(mode, hp, l.count * g.count, lds, st);
            }
            hipLaunchKernelGGL(k_field_hist_out, dim3(g.count), dim3(FS_TPB), 0, st, op);
        }
        SS_HIP(ctx, hipGetLastError());
    }
    SS_HIP(ctx, turn.batch_ev.record(st));          // until here the call reads the turn's sets and tables
    if (dev_out) return SS_OK;                      // ordered on the ctx stream; ss_synchronize (or the stream's owner) waits
    std::vector<unsigned char> h_out(out_bytes);
    SS_HIP(ctx, hipMemcpyAsync(h_out.data(), s->d_fstats_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));
    SS_HIP(ctx, hw::give_rows(counts_out, h_out.data(), nq, nb, sizeof(uint32_t), nullptr));
    if (tails_out) SS_HIP(ctx, hw::give_rows(tails_out, h_out.data() + o_tails, nq, 1, sizeof(ss_hist_tail), nullptr));
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_field_stats(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                       const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                       const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t n_stat_fields, const int32_t* fields, ss_field_stat* stats_out,
                       uint32_t* n_match_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return hw::guarded(s, "ss_field_stats", [&] {
        return field_stats_impl(s, n_q, q_ptr, q_terms, mask_id, cons, ranges, n_stat_fields, fields, stats_out, n_match_out);
    });
}

int32_t ss_field_histogram(ss_scorer* s, int32_t n_q, const uint32_t* q_ptr, const uint32_t* q_terms, const int32_t* mask_id,
                           const uint32_t* req_ptr, const uint32_t* req_terms, const uint32_t* exc_ptr, const uint32_t* exc_terms,
                           const uint32_t* rng_ptr, const ss_doc_range* rng, int32_t field, int64_t origin, uint64_t width, const int64_t* edges,
                           int32_t n_bins, uint32_t* counts_out, ss_hist_tail* tails_out) {
    const QueryConstraints cons{req_ptr, req_terms, exc_ptr, exc_terms};
    const QueryRanges ranges{rng_ptr, rng};
    return hw::guarded(s, "ss_field_histogram", [&] {
        return field_histogram_impl(s, n_q, q_ptr, q_terms, mask_id, cons, ranges, field, origin, width, edges, n_bins, counts_out, tails_out);
    });
}

}  // extern "C"
