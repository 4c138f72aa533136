// links.hip — ss_graph_set_link_key, ss_graph_top_links, ss_graph_hit_links: the best parents or children of a page.
// The last stage of the result pipeline: per result row the m best DISTINCT neighbours of the hit's node and the row's edge count,
// read from the arrays the graph already keeps — children from the out-edge CSR (original ids), parents from the sweep's in-edge
// lists (internal ids, bit 31 = k_flag_row_ends' mark, mapped back through old_id).  Nothing here writes those arrays and no second
// copy of the edges is made.
//
//   k_links_count   a thread per requested row: the row's edge range and how many work items it becomes (0 for an empty, unknown or
//                   unwritten row, 1 up to "links.wave_max" edges, ceil(len / "links.chunk_edges") above); writes degree_out, and
//                   n_out = 0 of the rows that end here
//   k_links_scan    one workgroup: the exclusive prefix of those counts — the work list in run-length form: item w belongs to the
//                   row r with off[r] <= w < off[r + 1] and is its chunk w - off[r]
//   k_links_select  a fixed grid of one-wave workgroups walks the items: the item's edges are staged ONCE in the LDS as (ordered key,
//                   id), then up to m rounds of a wave-wide maximum over the entries strictly below the previous winner.  Equal ids
//                   have equal entries, so "strictly below" is also what makes the winners distinct.  An unsplit row's winners go
//                   to the caller's row; a chunk's go to its slot of the partial block, padded with NONE.
//   k_links_merge   a wave per split row: the chunks' winner lists are descending and duplicate-free, so the row's winners are an
//                   m-step merge of them; 64 lists at a time (a list per lane, the head in registers) against the running result
//                   in the LDS.  Every list whose head equals the winner advances: a node that won in two chunks — a duplicate
//                   edge straddling a cut — is taken once.
// The order is total (key, then id), the selection exact and free of atomics: a row does not depend on which workgroup ran first.
#include "graph.hpp"
#include "links_plan.hpp"

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = 1024;
constexpr uint32_t NONE = 0xFFFFFFFFu;                    // no node: ids stay below 0xFFFFFFF0 (ss_graph_create)
constexpr uint32_t HIT_WORDS = sizeof(ss_hit) / 4;

struct LinkArgs {
    const uint32_t* ids;            // node id of requested row r: ids[r * id_stride]  (id_stride = HIT_WORDS reads ss_hit.doc)
    uint32_t id_stride;
    const int32_t* n_hits;          // hits form: [n_q], row r = (q, j) = (r / k, r % k) is requested iff j < clamp(n_hits[q], 0, k); else NULL
    uint32_t k;
    uint64_t n_rows;
    uint32_t m;
    int32_t dir;
    uint64_t n_nodes;
    const uint64_t* out_ptr;
    const uint32_t* out_dst;
    const uint32_t* new_id;
    const uint32_t* old_id;
    const uint32_t* in_ptr;
    const uint32_t* in_src;
    const double* key;              // NULL: order by id
    uint32_t wave_max, chunk;
    uint64_t* row_base;             // [n_rows]
    uint64_t* row_len;              // [n_rows]
    uint64_t* req_off;              // [n_rows + 1]
    uint32_t* partial;              // [items][m]
    uint32_t* links_out;
    int32_t* n_out;
    uint32_t* degree_out;           // nullable
};

// key descending as float64 VALUES (-0 = +0), NaN below everything: a larger ordered key comes earlier
__device__ __forceinline__ uint64_t ordered_key(double f) {
    if (f != f) return 0ull;
    if (f == 0.0) return 0x8000000000000000ull;           // both zeros: the key of +0
    const uint64_t b = (uint64_t)__double_as_longlong(f);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);  // (~b = 0 only for a NaN's bits)
}
// entries are (ordered key, ~id), compared as one 96-bit number; (0, 0) is below every entry (~id = 0 would be id NONE)
__device__ __forceinline__ bool below(uint64_t ak, uint32_t an, uint64_t bk, uint32_t bn) { return ak < bk || (ak == bk && an < bn); }

__device__ __forceinline__ void wave_max_entry(uint64_t& k, uint32_t& n) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_xor(k, off, 64);
        const uint32_t on = __shfl_xor(n, off, 64);
        if (below(k, n, ok, on)) { k = ok; n = on; }
    }
}

__global__ __launch_bounds__(TPB) void k_links_max_outdeg(const uint64_t* __restrict__ out_ptr, uint64_t n, unsigned long long* __restrict__ d_max) {
    uint64_t best = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * TPB + threadIdx.x; v < n; v += (uint64_t)gridDim.x * TPB) {
        const uint64_t d = out_ptr[v + 1] - out_ptr[v];
        best = d > best ? d : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(d_max, (unsigned long long)best);
}

__global__ __launch_bounds__(TPB) void k_links_count(LinkArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= a.n_rows) return;
    bool wanted = true;
    if (a.n_hits) {
        const uint64_t q = r / a.k;
        const uint32_t j = (uint32_t)(r - q * a.k);
        const int32_t nh = a.n_hits[q];
        wanted = nh > 0 && j < (uint32_t)(nh > (int32_t)a.k ? (int32_t)a.k : nh);
    }
    uint64_t base = 0, len = 0, items = 0;
    if (wanted) {
        const uint32_t v = a.ids[r * a.id_stride];
        if ((uint64_t)v < a.n_nodes) {                    // an id outside the graph has no edges: nothing of the graph is read for it
            if (a.dir == SS_LINKS_CHILDREN) {
                base = a.out_ptr[v];
                len = a.out_ptr[v + 1] - base;
            } else {
                const uint32_t row = a.new_id[v];         // (0, 1) graph: the internal id is the local row
                base = a.in_ptr[row];
                len = a.in_ptr[row + 1] - base;
            }
        }
        if (a.degree_out) a.degree_out[r] = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
        if (len == 0) a.n_out[r] = 0;
        else items = len <= a.wave_max ? 1 : (len + a.chunk - 1) / a.chunk;
    }
    a.row_base[r] = base;
    a.row_len[r] = len;
    a.req_off[r] = items;
}

// off[0 .. n) counts -> their exclusive prefix, off[n] = the total.  One workgroup; thread t owns a run of ceil(n / SCAN_TPB) rows.
__global__ __launch_bounds__(SCAN_TPB) void k_links_scan(uint64_t* __restrict__ off, uint64_t n) {
    __shared__ uint64_t s_sum[SCAN_TPB];
    const uint32_t t = threadIdx.x;
    const uint64_t seg = (n + SCAN_TPB - 1) / SCAN_TPB;
    const uint64_t b = t * seg < n ? t * seg : n, e = b + seg < n ? b + seg : n;
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; i++) sum += off[i];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_TPB; d <<= 1) {
        const uint64_t add = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    uint64_t run = s_sum[t] - sum;
    for (uint64_t i = b; i < e; i++) {
        const uint64_t c = off[i];
        off[i] = run;
        run += c;
    }
    if (t == SCAN_TPB - 1) off[n] = s_sum[t];
}

// dynamic LDS: lds_entries * (8 + 4) bytes
__global__ __launch_bounds__(64) void k_links_select(LinkArgs a, uint32_t lds_entries) {
    extern __shared__ __attribute__((aligned(16))) uint64_t ls_lds[];
    uint64_t* const s_key = ls_lds;
    uint32_t* const s_id = reinterpret_cast<uint32_t*>(ls_lds + lds_entries);
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.req_off[a.n_rows];
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        uint64_t lo = 0, hi = a.n_rows;                   // off[lo] <= w < off[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (a.req_off[mid] <= w) lo = mid; else hi = mid;
        }
        const uint64_t r = lo, c = w - a.req_off[r];
        const uint64_t len = a.row_len[r];
        const bool split = len > a.wave_max;
        const uint64_t first = split ? c * a.chunk : 0;
        uint32_t l = 0;
        if (first < len) {                                // (always: the plan made ceil(len / chunk) items)
            const uint64_t left = len - first;
            const uint64_t cap = split ? a.chunk : a.wave_max;
            l = (uint32_t)(left < cap ? left : cap);
        }
        if (l > lds_entries) l = lds_entries;             // (never: lds_entries = max(wave_max, chunk))
        const uint64_t e0 = a.row_base[r] + first;
        for (uint32_t j = lane; j < l; j += 64) {
            uint32_t u;
            if (a.dir == SS_LINKS_CHILDREN) u = a.out_dst[e0 + j];
            else u = a.old_id[a.in_src[e0 + j] & 0x7FFFFFFFu];
            s_id[j] = u;
            s_key[j] = a.key ? ordered_key(a.key[u]) : 1ull;
        }
        __syncthreads();                                  // (one wave: orders the LDS writes above before the reads below)
        uint32_t* const dst = split ? a.partial + w * a.m : a.links_out + r * a.m;
        uint64_t pk = ~0ull;                              // no entry reaches it (its key part would be a NaN's bits)
        uint32_t pn = ~0u, cnt = 0;
        for (uint32_t round = 0; round < a.m; round++) {
            uint64_t bk = 0;
            uint32_t bn = 0;
            for (uint32_t j = lane; j < l; j += 64) {
                const uint64_t ek = s_key[j];
                const uint32_t en = ~s_id[j];
                if (below(ek, en, pk, pn) && below(bk, bn, ek, en)) { bk = ek; bn = en; }
            }
            wave_max_entry(bk, bn);
            if (bk == 0 && bn == 0) break;                // nothing left below the previous winner
            if (lane == 0) dst[round] = ~bn;
            pk = bk;
            pn = bn;
            cnt++;
        }
        if (split) {
            for (uint32_t j = cnt + lane; j < a.m; j += 64) dst[j] = NONE;
        } else if (lane == 0) {
            a.n_out[r] = (int32_t)cnt;
        }
        __syncthreads();                                  // the next item's staging overwrites what this one's rounds read
    }
}

__global__ __launch_bounds__(64) void k_links_merge(LinkArgs a) {
    __shared__ uint64_t s_key[2][SS_MAX_LINKS];
    __shared__ uint32_t s_nid[2][SS_MAX_LINKS];
    const uint64_t r = blockIdx.x;
    const uint64_t len = a.row_len[r];
    if (len <= a.wave_max) return;                        // not a split row (the whole wave leaves)
    const uint32_t lane = threadIdx.x;
    const uint64_t n_lists = (len + a.chunk - 1) / a.chunk, w0 = a.req_off[r];
    uint32_t cur = 0, n_cur = 0;                          // the running result: s_*[cur][0 .. n_cur), descending
    for (uint64_t g0 = 0; g0 < n_lists; g0 += 64) {
        const bool have = g0 + lane < n_lists;
        const uint32_t* const lst = a.partial + (w0 + g0 + (have ? lane : 0)) * a.m;
        uint32_t at = 0, hn = 0;
        uint64_t hk = 0;
        auto load_head = [&]() {
            hk = 0;
            hn = 0;
            if (have && at < a.m) {
                const uint32_t id = lst[at];
                if (id != NONE) {
                    hn = ~id;
                    hk = a.key ? ordered_key(a.key[id]) : 1ull;
                }
            }
        };
        load_head();
        uint32_t pa = 0, n_new = 0;
        for (uint32_t round = 0; round < a.m; round++) {
            uint64_t wk = hk;
            uint32_t wn = hn;
            wave_max_entry(wk, wn);
            uint64_t ak = 0;
            uint32_t an = 0;
            if (pa < n_cur) { ak = s_key[cur][pa]; an = s_nid[cur][pa]; }
            if (below(wk, wn, ak, an)) { wk = ak; wn = an; }
            if (wk == 0 && wn == 0) break;
            if (lane == 0) { s_key[cur ^ 1][n_new] = wk; s_nid[cur ^ 1][n_new] = wn; }
            n_new++;
            if (ak == wk && an == wn) pa++;
            if (hk == wk && hn == wn) { at++; load_head(); }
        }
        __syncthreads();                                  // (one wave: lane 0's writes before everybody's reads)
        cur ^= 1;
        n_cur = n_new;
    }
    if (lane < n_cur) a.links_out[r * a.m + lane] = ~s_nid[cur][lane];
    if (lane == 0) a.n_out[r] = (int32_t)n_cur;
}

template <typename T>
inline hipError_t ensure(ss::DevBuf<T>& b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    return b.alloc(n + n / 2 + 16);
}

// The largest out-degree is not on the host after ss_graph_create (max_indeg is): the first call for children asks the device and
// waits once; the value is kept until ss_graph_apply_delta.
int32_t max_outdeg(ss_graph* g, uint64_t* out) {
    ss_ctx* ctx = g->ctx;
    ss_graph::Links& L = g->links;
    if (!L.max_outdeg_known) {
        hipStream_t st = ctx->stream;
        SS_HIP(ctx, ensure(L.d_max, 1));
        SS_HIP(ctx, hipMemsetAsync(L.d_max.p, 0, sizeof(uint64_t), st));
        const unsigned grid = std::min<unsigned>(ss::div_up(g->n, TPB), (unsigned)ctx->cu_count * 8u);
        hipLaunchKernelGGL(k_links_max_outdeg, dim3(grid), dim3(TPB), 0, st, (const uint64_t*)g->out_ptr.p, g->n,
                           reinterpret_cast<unsigned long long*>(L.d_max.p));
        SS_HIP(ctx, hipGetLastError());
        uint64_t v = 0;
        SS_HIP(ctx, ss::fetch(ctx, st, &v, L.d_max.p, sizeof(uint64_t)));
        L.max_outdeg = v;
        L.max_outdeg_known = true;
    }
    *out = L.max_outdeg;
    return SS_OK;
}

// Both entry points after their own checks.  ids / id_stride / n_hits / k as in LinkArgs (n_hits NULL: the node-list form).
int32_t links_run(ss_graph* g, const char* fn, int32_t dir, uint64_t n_rows, const uint32_t* ids, uint32_t id_stride, uint64_t n_q, int32_t k,
                  const int32_t* n_hits, int32_t m, uint32_t* links_out, int32_t* n_out, uint32_t* degree_out) {
    ss_ctx* ctx = g->ctx;
    ss_graph::Links& L = g->links;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool dev_i = ss::on_device(ids), dev_h = !n_hits || ss::on_device(n_hits);
    const bool dev_l = ss::on_device(links_out), dev_n = ss::on_device(n_out), dev_d = !degree_out || ss::on_device(degree_out);
    std::vector<int32_t> h_nh;                            // hits form: the counts as the kernel takes them (staged path only)
    if (n_hits && !dev_h) {
        h_nh.assign(n_hits, n_hits + n_q);
        for (uint64_t q = 0; q < n_q; q++)
            if (h_nh[q] < 0 || h_nh[q] > k) return ctx->fail(SS_ERR_INVALID, "%s: n_hits[%llu] = %d outside 0 .. k = %d", fn, (unsigned long long)q, h_nh[q], k);
    }
    uint64_t max_deg = g->max_indeg;
    if (dir == SS_LINKS_CHILDREN) SS_TRY(max_outdeg(g, &max_deg));
    const ss::links::Bounds B = ss::links::bounds(n_rows, (uint32_t)m, max_deg, ctx->opt("links.wave_max", ss::links::WAVE_MAX_DEFAULT),
                                                   ctx->opt("links.chunk_edges", ss::links::CHUNK_DEFAULT));
    if (B.too_large)
        return ctx->fail(SS_ERR_OOM, "%s: %llu rows of up to %llu chunks of %d winners: the partial winners cannot be held", fn,
                         (unsigned long long)n_rows, (unsigned long long)B.items_per_row, m);
    // ---- blocks: all of them before anything is enqueued
    {
        hipError_t e = ensure(L.row_base, n_rows);
        if (e == hipSuccess) e = ensure(L.row_len, n_rows);
        if (e == hipSuccess) e = ensure(L.req_off, n_rows + 1);
        if (e == hipSuccess) e = ensure(L.partial, (size_t)(B.items * (uint64_t)m));
        if (e == hipSuccess && !dev_i) e = ensure(L.d_ids, n_rows);
        if (e == hipSuccess && n_hits && !dev_h) e = ensure(L.d_nhits, n_q);
        if (e == hipSuccess && !dev_l) e = ensure(L.d_links, n_rows * (size_t)m);
        if (e == hipSuccess && !dev_n) e = ensure(L.d_n, n_rows);
        if (e == hipSuccess && degree_out && !dev_d) e = ensure(L.d_deg, n_rows);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "%s: %llu rows x %llu chunks x %d winners: %s", fn,
                             (unsigned long long)n_rows, (unsigned long long)B.items_per_row, m, hipGetErrorString(e));
        }
    }
    // ---- inputs in host memory go up (a host row of hits as its doc ids alone)
    std::vector<uint32_t> h_ids;
    if (!dev_i) {
        const uint32_t* src = ids;
        if (id_stride != 1) {
            h_ids.resize(n_rows);
            for (uint64_t r = 0; r < n_rows; r++) h_ids[r] = ids[r * id_stride];
            src = h_ids.data();
        }
        SS_HIP(ctx, hipMemcpyAsync(L.d_ids.p, src, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (n_hits && !dev_h) SS_HIP(ctx, hipMemcpyAsync(L.d_nhits.p, h_nh.data(), n_q * sizeof(int32_t), hipMemcpyHostToDevice, st));
    LinkArgs a{};
    a.ids = dev_i ? ids : L.d_ids.p;
    a.id_stride = dev_i ? id_stride : 1u;
    a.n_hits = !n_hits ? nullptr : dev_h ? n_hits : L.d_nhits.p;
    a.k = (uint32_t)k;
    a.n_rows = n_rows;
    a.m = (uint32_t)m;
    a.dir = dir;
    a.n_nodes = g->n;
    a.out_ptr = g->out_ptr.p; a.out_dst = g->out_dst.p;
    a.new_id = g->new_id.p; a.old_id = g->old_id.p; a.in_ptr = g->in_ptr.p; a.in_src = g->in_src.p;
    a.key = L.has_key ? L.key.p : nullptr;
    a.wave_max = B.wave_max; a.chunk = B.chunk;
    a.row_base = L.row_base.p; a.row_len = L.row_len.p; a.req_off = L.req_off.p; a.partial = L.partial.p;
    a.links_out = dev_l ? links_out : L.d_links.p;
    a.n_out = dev_n ? n_out : L.d_n.p;
    a.degree_out = !degree_out ? nullptr : dev_d ? degree_out : L.d_deg.p;
    // ---- the pipeline: plan on the device, select over a fixed grid, merge the split rows
    hipLaunchKernelGGL(k_links_count, dim3(ss::div_up(n_rows, TPB)), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_links_scan, dim3(1), dim3(SCAN_TPB), 0, st, a.req_off, n_rows);
    const unsigned grid = (unsigned)std::min<uint64_t>(B.items, (uint64_t)ctx->cu_count * 16u);
    hipLaunchKernelGGL(k_links_select, dim3(grid), dim3(64), (size_t)B.lds_entries * ss::links::LDS_ENTRY_BYTES, st, a, B.lds_entries);
    if (max_deg > B.wave_max) hipLaunchKernelGGL(k_links_merge, dim3((unsigned)n_rows), dim3(64), 0, st, a);
    SS_HIP(ctx, hipGetLastError());
    if (dev_i && dev_h && dev_l && dev_n && dev_d) return SS_OK;   // ordered on the ctx stream; nothing is waited for
    // ---- staged: wait; host outputs get exactly the entries the kernels wrote
    std::vector<int32_t> h_n;
    std::vector<uint32_t> h_links, h_deg;
    if (!dev_l || !dev_n) {
        h_n.resize(n_rows);
        SS_HIP(ctx, hipMemcpyAsync(h_n.data(), a.n_out, n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (!dev_l) {
        h_links.resize(n_rows * (size_t)m);
        SS_HIP(ctx, hipMemcpyAsync(h_links.data(), L.d_links.p, h_links.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (degree_out && !dev_d) {
        h_deg.resize(n_rows);
        SS_HIP(ctx, hipMemcpyAsync(h_deg.data(), L.d_deg.p, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (n_hits && dev_h && (!dev_l || !dev_n || !dev_d)) {
        h_nh.resize(n_q);
        SS_HIP(ctx, hipMemcpyAsync(h_nh.data(), n_hits, n_q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    SS_HIP(ctx, hipStreamSynchronize(st));
    if (dev_l && dev_n && dev_d) return SS_OK;
    for (uint64_t r = 0; r < n_rows; r++) {
        if (n_hits) {
            const uint64_t q = r / (uint64_t)k;
            const int32_t nh = std::min(std::max(h_nh[q], 0), k);
            if ((int64_t)(r - q * (uint64_t)k) >= nh) continue;
        }
        if (!dev_n) n_out[r] = h_n[r];
        if (!dev_l && h_n[r] > 0) std::memcpy(links_out + r * (size_t)m, h_links.data() + r * (size_t)m, (size_t)h_n[r] * sizeof(uint32_t));
        if (degree_out && !dev_d) degree_out[r] = h_deg[r];
    }
    return SS_OK;
}

// the checks both calls share; `rows` = n or n_q * k
int32_t links_checks(ss_graph* g, const char* fn, int32_t dir, int32_t m, uint64_t rows) {
    ss_ctx* ctx = g->ctx;
    if (dir != SS_LINKS_PARENTS && dir != SS_LINKS_CHILDREN) return ctx->fail(SS_ERR_INVALID, "%s: dir = %d, must be SS_LINKS_PARENTS or SS_LINKS_CHILDREN", fn, dir);
    if (m < 1) return ctx->fail(SS_ERR_INVALID, "%s: m = %d, must be >= 1", fn, m);
    if (m > SS_MAX_LINKS) return ctx->fail(SS_ERR_UNSUPPORTED, "%s: m = %d exceeds SS_MAX_LINKS = %d", fn, m, SS_MAX_LINKS);
    if (rows > ((1ull << 31) - 1) / (uint64_t)m)
        return ctx->fail(SS_ERR_UNSUPPORTED, "%s: %llu rows of %d links, must be below 2^31 entries", fn, (unsigned long long)rows, m);
    if (g->rank != 0 || g->world != 1)
        return ctx->fail(SS_ERR_UNSUPPORTED, "%s: needs a (0, 1) graph, this is shard %d of %d (a shard holds only its own rows' in-edges)", fn, g->rank, g->world);
    return SS_OK;
}

}  // namespace

extern "C" {

int32_t ss_graph_set_link_key(ss_graph* g, const double* key) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ss_graph::Links& L = g->links;
    if (!key) {                                           // (the block stays: a call enqueued earlier may still read it)
        L.has_key = false;
        return SS_OK;
    }
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!L.key.p || L.key.n != g->n) SS_HIP(ctx, L.key.alloc(g->n));
    // ordered on the ctx stream behind the link calls that read the previous key, in front of those that follow
    SS_HIP(ctx, hipMemcpyAsync(L.key.p, key, g->n * sizeof(double), hipMemcpyDefault, st));
    if (!ss::on_device(key)) SS_HIP(ctx, hipStreamSynchronize(st));   // the caller's host array has been read when the call returns
    L.has_key = true;
    return SS_OK;
}

int32_t ss_graph_top_links(ss_graph* g, int32_t dir, uint64_t n, const uint32_t* nodes, int32_t m, uint32_t* links_out, int32_t* n_out,
                           uint32_t* degree_out) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    try {
        if (n && (!nodes || !links_out || !n_out)) return ctx->fail(SS_ERR_INVALID, "ss_graph_top_links: NULL argument");
        SS_TRY(links_checks(g, "ss_graph_top_links", dir, m, n));
        if (n == 0) return SS_OK;
        return links_run(g, "ss_graph_top_links", dir, n, nodes, 1u, 0, 1, nullptr, m, links_out, n_out, degree_out);
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "ss_graph_top_links: host allocation failed");
    }
}

int32_t ss_graph_hit_links(ss_graph* g, int32_t dir, int32_t n_q, int32_t k, const ss_hit* hits, const int32_t* n_hits, int32_t m,
                           uint32_t* links_out, int32_t* n_out, uint32_t* degree_out) {
    if (!g) return SS_ERR_INVALID;
    ss_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    try {
        if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "ss_graph_hit_links: n_q = %d", n_q);
        if (k < 1) return ctx->fail(SS_ERR_INVALID, "ss_graph_hit_links: k = %d, must be >= 1", k);
        if (n_q && (!hits || !n_hits || !links_out || !n_out)) return ctx->fail(SS_ERR_INVALID, "ss_graph_hit_links: NULL argument");
        if (k > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_graph_hit_links: k = %d exceeds SS_MAX_TOPK = %d", k, SS_MAX_TOPK);
        SS_TRY(links_checks(g, "ss_graph_hit_links", dir, m, (uint64_t)n_q * (uint64_t)k));
        if (n_q == 0) return SS_OK;
        static_assert(sizeof(ss_hit) == 40 && HIT_WORDS == 10, "ss_hit.doc is word 0 of 10");
        return links_run(g, "ss_graph_hit_links", dir, (uint64_t)n_q * (uint64_t)k, reinterpret_cast<const uint32_t*>(hits), HIT_WORDS,
                         (uint64_t)n_q, k, n_hits, m, links_out, n_out, degree_out);
    } catch (const std::bad_alloc&) {
        return ctx->fail(SS_ERR_OOM, "ss_graph_hit_links: host allocation failed");
    }
}

}  // extern "C"
