// field.hip — ss_scorer_set_doc_fields, ss_doc_field_masks, ss_sort_hits_by_field and ss_hit_fields: a few signed 64-bit values per doc,
// allow-lists from range clauses over them, a result window sorted by one of them and their read-out per row.  The
// range clauses of ss_score_topk_filtered go through launch_field_masks from score_call.hip.
//
//   k_field_masks          One workgroup of 8 waves owns FM_DOCS = 8192 docs (256 words) of one GROUP of up to FM_GROUP = 64 sets.  A wave
//                          first loads the values of its 1024 docs — 16 steps of 64 docs, one coalesced 8-byte load per step and field
//                          the group's clauses read — and keeps them in registers: a column is read once per group, not once per set.
//                          Then it walks the group's sets.  The clauses are wave-uniform (LDS -> scalar registers); a step's test is a
//                          wave ballot, ANDed over the set's clauses in scalar registers; lane l < 32 keeps word l of the wave's 32
//                          words (step l / 2, half l & 1), ANDs the base word into it once per set — the registered allow-list, or
//                          the word that stands in the output (behind k_constraint_masks) — and stores it: every word of every set is
//                          written exactly once with vector stores.  No atomics, no order dependence, no temporaries.
//   k_sort_hits_by_field   One workgroup per query, as k_collapse_hits: (class, key, window index) triples sorted in LDS over the next
//                          power of two >= the window's length; class 0 = doc inside the table, 1 = outside, 2 = padding; the key is
//                          the value with its sign bit flipped (complemented for descending).  The window index makes the order total,
//                          so the bitonic network gives the stable result.  The page's rows are copied five lanes to a row.
//   k_hit_fields           a gather: one thread per (row, field).
// ss_sort_hits_by_field / ss_hit_fields: the window in, the paging checks and the outputs' way back are hit_window.hpp's.
#include "hit_window.hpp"

#include <algorithm>

namespace {

namespace hw = ss::hitwin;

constexpr int FM_TPB = 512;                               // threads: 8 waves
constexpr int FM_STEPS = 16;                              // steps of 64 docs a wave holds in registers (2 VGPRs per step and field)
constexpr int FM_WAVE_DOCS = FM_STEPS * 64;               // 1024 docs = 32 words per wave
constexpr int FM_DOCS = (FM_TPB / 64) * FM_WAVE_DOCS;     // docs of a workgroup: 8192
constexpr int FM_WORDS = FM_DOCS / 32;
constexpr int FM_GROUP = 64;                              // sets that share one read of the columns: column bytes per set = set bytes
constexpr uint32_t FM_MAX_BLOCKS = 1u << 20;              // workgroups of one launch
constexpr size_t FM_KEEP_BYTES = (size_t)64 << 20;        // ss_doc_field_masks: a larger device block of a HOST output is freed when the call returns
static_assert(FM_DOCS <= 32768 && FM_WAVE_DOCS / 32 == 32, "a wave's words are one per lane of its lower half");
static_assert(SS_MAX_DOC_FIELDS == 4 && SS_MAX_RANGE_CLAUSES == 4, "k_field_masks holds four columns and stages four clauses per set");

// m[s] &= the lanes whose value of step s lies in [lo, hi]
__device__ __forceinline__ void and_clause(uint64_t (&m)[FM_STEPS], const int64_t (&v)[FM_STEPS], int64_t lo, int64_t hi) {
#pragma unroll
    for (int s = 0; s < FM_STEPS; s++) m[s] &= __ballot(v[s] >= lo && v[s] <= hi);
}

__device__ __forceinline__ int64_t uniform64(int64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}

__global__ __launch_bounds__(FM_TPB) void k_field_masks(FieldParams p, uint32_t group0, uint32_t n_blocks) {
    __shared__ FieldSet s_set[FM_GROUP];
    __shared__ ss_doc_range s_cl[FM_GROUP * SS_MAX_RANGE_CLAUSES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t grp = group0 + blockIdx.x / n_blocks, blk = blockIdx.x % n_blocks;
    const uint32_t s0 = grp * FM_GROUP;                                              // < n_sets: the launcher's grid
    const uint32_t ns = p.n_sets - s0 < (uint32_t)FM_GROUP ? p.n_sets - s0 : (uint32_t)FM_GROUP;
    if (tid < ns) s_set[tid] = p.sets[s0 + tid];
    __syncthreads();
    if (tid < ns * SS_MAX_RANGE_CLAUSES) {
        const FieldSet fs = s_set[tid >> 2];
        if ((tid & 3u) < fs.n_cl) s_cl[tid] = p.clauses[fs.c0 + (tid & 3u)];
    }
    __syncthreads();
    const uint32_t gf = p.group_fields[grp];
    const uint64_t d0 = (uint64_t)blk * FM_DOCS + (uint64_t)wave * FM_WAVE_DOCS + lane;   // this lane's doc of step 0
    // ---- the wave's docs: which exist, and their values in the columns the group reads
    uint64_t live[FM_STEPS];
    int64_t v0[FM_STEPS], v1[FM_STEPS], v2[FM_STEPS], v3[FM_STEPS];
#pragma unroll
    for (int s = 0; s < FM_STEPS; s++) {
        const uint64_t d = d0 + (uint64_t)s * 64;
        const bool in = d < p.n_docs;
        live[s] = __ballot(in);
        v0[s] = in && (gf & 1u) ? p.values[d] : 0;
        v1[s] = in && (gf & 2u) ? p.values[p.n_docs + d] : 0;
        v2[s] = in && (gf & 4u) ? p.values[2 * p.n_docs + d] : 0;
        v3[s] = in && (gf & 8u) ? p.values[3 * p.n_docs + d] : 0;
    }
    const uint64_t w = (uint64_t)blk * FM_WORDS + (uint64_t)wave * (FM_WAVE_DOCS / 32) + lane;   // lanes 0 .. 31: the word this lane owns
    const bool owner = lane < 32u && w < p.stride;
    // ---- the group's sets
    for (uint32_t i = 0; i < ns; i++) {
        const FieldSet fs = s_set[i];
        const uint32_t n_cl = __builtin_amdgcn_readfirstlane(fs.n_cl);
        uint64_t m[FM_STEPS];
#pragma unroll
        for (int s = 0; s < FM_STEPS; s++) m[s] = live[s];
        for (uint32_t c = 0; c < n_cl; c++) {
            const ss_doc_range cl = s_cl[i * SS_MAX_RANGE_CLAUSES + c];
            const int64_t lo = uniform64(cl.lo), hi = uniform64(cl.hi);
            switch (__builtin_amdgcn_readfirstlane(cl.field)) {                      // (0 .. n_fields-1: checked by the host)
                case 0: and_clause(m, v0, lo, hi); break;
                case 1: and_clause(m, v1, lo, hi); break;
                case 2: and_clause(m, v2, lo, hi); break;
                default: and_clause(m, v3, lo, hi); break;
            }
        }
        uint32_t mine = 0;
#pragma unroll
        for (int s = 0; s < FM_STEPS; s++) {
            const uint32_t half = (lane & 1u) ? (uint32_t)(m[s] >> 32) : (uint32_t)m[s];
            if ((lane >> 1) == (uint32_t)s) mine = half;
        }
        if (owner) {
            uint32_t* const out = p.out + (uint64_t)fs.out_set * p.stride + w;
            uint32_t base = ~0u;                                                     // (the mask AND: once per set, outside the clause loop)
            if (fs.base1 == FS_IN_PLACE) base = *out;
            else if (fs.base1) base = w < p.reg_words ? p.reg_masks[(uint64_t)(fs.base1 - 1u) * p.reg_words + w] : 0u;
            *out = mine & base;
        }
    }
}

// ---- sort a window by a field ------------------------------------------------------------------------------------------------
constexpr uint32_t SF_CLASS_SHIFT = 16;                   // tag = class << 16 | window index (< SS_MAX_TOPK = 2^10)
constexpr uint32_t SF_OUTSIDE = 1, SF_DEAD = 2;

struct SortFieldParams {
    const int64_t* column;                                // [n_docs] the field's values
    uint64_t n_docs;
    const ss_hit* hits;                                   // [n_q][k_in]
    const int32_t* n_hits;                                // [n_q]
    ss_hit* hits_out;                                     // [n_q][k]
    int32_t* n_hits_out;                                  // [n_q]
    int64_t* values_out;                                  // [n_q][k], nullable
    uint32_t k_in, first, k, descending;
};

// (class, key, window index) of a behind that of b
__device__ __forceinline__ bool sf_after(uint64_t ka, uint32_t ta, uint64_t kb, uint32_t tb) {
    const uint32_t ca = ta >> SF_CLASS_SHIFT, cb = tb >> SF_CLASS_SHIFT;
    return ca != cb ? ca > cb : ka != kb ? ka > kb : ta > tb;
}

template <int BLOCK, int PER>
__global__ __launch_bounds__(BLOCK) void k_sort_hits_by_field(SortFieldParams p) {
    constexpr uint32_t CAP = PER * BLOCK;
    __shared__ uint64_t s_key[CAP];
    __shared__ uint32_t s_tag[CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = hw::window_len(p.n_hits[q], p.k_in);   // <= k_in <= CAP: checked by the launcher
    const ss_hit* const rows = p.hits + (size_t)q * p.k_in;
    const uint32_t np = hw::pow2_at_least(n);
    const uint64_t flip = p.descending ? ~0ull : 0ull;
    for (uint32_t j = tid; j < np; j += BLOCK) {
        uint64_t key = 0;
        uint32_t tag = SF_DEAD << SF_CLASS_SHIFT | j;
        if (j < n) {
            const uint32_t d = rows[j].doc;
            tag = SF_OUTSIDE << SF_CLASS_SHIFT | j;
            if ((uint64_t)d < p.n_docs) {
                key = ((uint64_t)p.column[d] ^ (1ull << 63)) ^ flip;
                tag = j;
            }
        }
        s_key[j] = key;
        s_tag[j] = tag;
    }
    __syncthreads();
    hw::bitonic_sort<BLOCK>(np, [&](uint32_t i, uint32_t o, bool up) {
        const uint64_t ka = s_key[i], kb = s_key[o];
        const uint32_t ta = s_tag[i], tb = s_tag[o];
        if (sf_after(ka, ta, kb, tb) == up) {
            s_key[i] = kb; s_tag[i] = tb;
            s_key[o] = ka; s_tag[o] = ta;
        }
    });
    // ---- the page: sorted positions [first, first + n_out), all below n
    const uint32_t n_out = hw::page_len(n, p.first, p.k);
    hw::copy_page<BLOCK>(rows, p.hits_out + (size_t)q * p.k, n_out, [&](uint32_t r) { return s_tag[p.first + r] & ((1u << SF_CLASS_SHIFT) - 1u); });
    if (p.values_out)
        for (uint32_t r = tid; r < n_out; r += BLOCK) {
            const uint32_t tag = s_tag[p.first + r];
            p.values_out[(size_t)q * p.k + r] = tag >> SF_CLASS_SHIFT ? SS_NO_FIELD_VALUE : (int64_t)((s_key[p.first + r] ^ flip) ^ (1ull << 63));
        }
    if (tid == 0) p.n_hits_out[q] = (int32_t)n_out;
}

constexpr int SF_SMALL = 64, SF_SMALL_PER = 2, SF_LARGE = 256, SF_LARGE_PER = 4;
static_assert(SF_LARGE * SF_LARGE_PER >= SS_MAX_TOPK, "k_sort_hits_by_field holds a whole window in LDS");

struct HitFieldParams {
    const int64_t* values;                                // [n_fields][n_docs]
    uint64_t n_docs;
    const ss_hit* hits;
    const int32_t* n_hits;
    int64_t* out;                                         // [n_q][k_in][n_fields]
    uint32_t k_in, n_fields;
    uint64_t total;                                       // n_q * k_in * n_fields
};

__global__ __launch_bounds__(256) void k_hit_fields(HitFieldParams p) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= p.total) return;
    const uint64_t row = x / p.n_fields;
    const uint32_t f = (uint32_t)(x - row * p.n_fields);
    const uint64_t q = row / p.k_in;
    const uint32_t j = (uint32_t)(row - q * p.k_in);
    if (j >= hw::window_len(p.n_hits[q], p.k_in)) return;
    const uint32_t d = p.hits[row].doc;
    p.out[x] = (uint64_t)d < p.n_docs ? p.values[(uint64_t)f * p.n_docs + d] : SS_NO_FIELD_VALUE;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
int32_t field_masks_impl(ss_scorer* s, int32_t n_sets, const uint32_t* rng_ptr, const ss_doc_range* rng, const int32_t* mask_id,
                         uint32_t* words_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and words_out is not touched before the last of them has passed
    if (n_sets < 0) return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: n_sets < 0");
    if (n_sets == 0) return SS_OK;
    if (!rng_ptr || !words_out) return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: rng_ptr or words_out is NULL");
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_sets;
    std::vector<uint32_t> ptr(ns + 1);
    SS_TRY(fetch_ptr_array(ctx, "ss_doc_field_masks", "rng", rng_ptr, ns, ptr.data()));
    if (ptr[0] != 0) return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: rng_ptr[0] is %u, not 0", ptr[0]);
    const size_t n_cl = ptr[ns];
    if (n_cl && !rng) return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: rng is NULL");
    for (size_t i = 0; i < ns; i++)
        if (ptr[i + 1] - ptr[i] > SS_MAX_RANGE_CLAUSES)
            return ctx->fail(SS_ERR_UNSUPPORTED, "ss_doc_field_masks: set %zu has %u clauses (max %d)", i, ptr[i + 1] - ptr[i], SS_MAX_RANGE_CLAUSES);
    if (n_cl && s->n_fields == 0) return ctx->fail(SS_ERR_STATE, "ss_doc_field_masks: no field table registered (ss_scorer_set_doc_fields)");
    std::vector<ss_doc_range> cl(n_cl);
    if (n_cl) SS_HIP(ctx, ss::copy_in(ctx->stream, cl.data(), rng, n_cl * sizeof(ss_doc_range)));
    for (size_t c = 0; c < n_cl; c++)
        if (cl[c].field < 0 || cl[c].field >= s->n_fields)
            return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: clause %zu names field %d (the scorer has %d fields)", c, cl[c].field, s->n_fields);
    std::vector<int32_t> mid(ns, -1);
    if (mask_id && ns) {
        SS_HIP(ctx, ss::copy_in(ctx->stream, mid.data(), mask_id, ns * sizeof(int32_t)));
        for (size_t i = 0; i < ns; i++)
            if (mid[i] < -1 || mid[i] >= s->n_masks)
                return ctx->fail(SS_ERR_INVALID, "ss_doc_field_masks: set %zu has mask id %d (the scorer has %d masks)", i, mid[i], s->n_masks);
    }
    const uint64_t n_words = (s->n_docs + 31) / 32;
    if (n_words == 0) return SS_OK;                           // (a scorer without docs: the sets have no words)
    hipStream_t st = ctx->stream;
    // ---- the table: sets | clauses | the groups' columns
    const size_t n_groups = (ns + FM_GROUP - 1) / FM_GROUP;
    std::vector<FieldSet> sets(ns);
    std::vector<uint32_t> gf(n_groups, 0u);
    for (size_t i = 0; i < ns; i++) {
        sets[i] = FieldSet{(uint32_t)i, (uint32_t)(mid[i] + 1), ptr[i], ptr[i + 1] - ptr[i]};
        for (uint32_t c = ptr[i]; c < ptr[i + 1]; c++) gf[i / FM_GROUP] |= 1u << cl[c].field;
    }
    const size_t o_cl = align16(ns * sizeof(FieldSet)), o_gf = align16(o_cl + n_cl * sizeof(ss_doc_range));
    const size_t tab_bytes = o_gf + n_groups * sizeof(uint32_t);
    std::vector<unsigned char> tab(tab_bytes, 0);
    std::memcpy(tab.data(), sets.data(), ns * sizeof(FieldSet));
    if (n_cl) std::memcpy(tab.data() + o_cl, cl.data(), n_cl * sizeof(ss_doc_range));
    std::memcpy(tab.data() + o_gf, gf.data(), n_groups * sizeof(uint32_t));
    SS_HIP(ctx, ensure(s->d_fld_tab, tab_bytes));
    const bool dev_out = ss::on_device(words_out);
    const size_t total = ns * (size_t)n_words;
    if (!dev_out) {
        const hipError_t e = s->d_fld_words.p && s->d_fld_words.n >= total ? hipSuccess : s->d_fld_words.alloc(total);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ctx->fail(e == hipErrorOutOfMemory ? SS_ERR_OOM : SS_ERR_HIP, "ss_doc_field_masks: no device memory for %zu sets of %llu bytes",
                             ns, (unsigned long long)(n_words * sizeof(uint32_t)));
        }
    }
    SS_HIP(ctx, hipMemcpyAsync(s->d_fld_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
    FieldParams p{};
    p.values = s->fields.p;
    p.n_docs = s->n_docs;
    p.sets = reinterpret_cast<const FieldSet*>(s->d_fld_tab.p);
    p.clauses = reinterpret_cast<const ss_doc_range*>(s->d_fld_tab.p + o_cl);
    p.group_fields = reinterpret_cast<const uint32_t*>(s->d_fld_tab.p + o_gf);
    p.n_sets = (uint32_t)n_sets;
    p.reg_masks = s->masks.p;
    p.reg_words = s->mask_words;
    p.out = dev_out ? words_out : s->d_fld_words.p;
    p.stride = n_words;
    p.n_words = n_words;
    ss::launch_field_masks(&p, st);
    SS_HIP(ctx, hipGetLastError());
    if (!dev_out) SS_HIP(ctx, hipMemcpyAsync(words_out, s->d_fld_words.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(ctx, hipStreamSynchronize(st));                    // (the table's host copy and the host output: the call waits)
    // the device block of a host output is kept for the next call only while it is small: 1024 sets at 10M docs are 1.28 GB
    if (!dev_out && s->d_fld_words.n * sizeof(uint32_t) > FM_KEEP_BYTES) s->d_fld_words.release();
    return SS_OK;
}

int32_t sort_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t field, int32_t descending,
                  int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, int64_t* values_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // ---- the checks: nothing is enqueued and no output is touched before the last of them has passed
    SS_TRY(hw::check_paging(ctx, "ss_sort_hits_by_field", "k_in", n_q, k_in, k, first));
    SS_TRY(hw::check_page_arrays(ctx, "ss_sort_hits_by_field", n_q, k_in, k, hits, n_hits, hits_out, n_hits_out));
    if (s->n_fields == 0) return ctx->fail(SS_ERR_STATE, "ss_sort_hits_by_field: no field table registered (ss_scorer_set_doc_fields)");
    if (field < 0 || field >= s->n_fields)
        return ctx->fail(SS_ERR_INVALID, "ss_sort_hits_by_field: field %d (the scorer has %d fields)", field, s->n_fields);
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_sort_hits_by_field", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    hw::RowsOut o;
    SS_TRY(hw::rows_out_prepare(s, (size_t)n_q, (size_t)k, hits_out, n_hits_out, nullptr, values_out, sizeof(int64_t), &o));
    SortFieldParams p{};
    p.column = s->fields.p + (size_t)field * (size_t)s->n_docs;
    p.n_docs = s->n_docs;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.hits_out = o.hits;
    p.n_hits_out = o.n_hits;
    p.values_out = static_cast<int64_t*>(o.extra);
    p.k_in = (uint32_t)k_in; p.first = (uint32_t)first; p.k = (uint32_t)k; p.descending = descending != 0;
    if (k_in <= SF_SMALL * SF_SMALL_PER)
        hipLaunchKernelGGL((k_sort_hits_by_field<SF_SMALL, SF_SMALL_PER>), dim3((unsigned)n_q), dim3(SF_SMALL), 0, st, p);
    else
        hipLaunchKernelGGL((k_sort_hits_by_field<SF_LARGE, SF_LARGE_PER>), dim3((unsigned)n_q), dim3(SF_LARGE), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    return hw::rows_out_finish(s, o, w.staged);
}

int32_t hit_fields_impl(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int64_t* values_out) {
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_q < 0) return ctx->fail(SS_ERR_INVALID, "ss_hit_fields: n_q < 0");
    if (k_in < 1) return ctx->fail(SS_ERR_INVALID, "ss_hit_fields: k_in = %d must be >= 1", k_in);
    if (k_in > SS_MAX_TOPK) return ctx->fail(SS_ERR_UNSUPPORTED, "ss_hit_fields: k_in = %d exceeds SS_MAX_TOPK = %d", k_in, SS_MAX_TOPK);
    if (n_q > 0 && (!hits || !n_hits || !values_out)) return ctx->fail(SS_ERR_INVALID, "ss_hit_fields: hits, n_hits or values_out is NULL");
    if (s->n_fields == 0) return ctx->fail(SS_ERR_STATE, "ss_hit_fields: no field table registered (ss_scorer_set_doc_fields)");
    if (n_q == 0) return SS_OK;
    SS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hw::WindowIn w;
    SS_TRY(hw::window_check(ctx, "ss_hit_fields", "k_in", n_q, k_in, hits, n_hits, &w));
    SS_TRY(hw::window_stage(s, &w));
    const size_t nf = (size_t)s->n_fields, total = (size_t)n_q * (size_t)k_in * nf;
    hw::EntriesOut o;
    SS_TRY(hw::entries_out_prepare(s, values_out, total * sizeof(int64_t), &o));
    HitFieldParams p{};
    p.values = s->fields.p;
    p.n_docs = s->n_docs;
    p.hits = w.hits;
    p.n_hits = w.n_hits;
    p.out = static_cast<int64_t*>(o.dev);
    p.k_in = (uint32_t)k_in;
    p.n_fields = (uint32_t)nf;
    p.total = total;
    hipLaunchKernelGGL(k_hit_fields, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
    SS_HIP(ctx, hipGetLastError());
    return hw::entries_out_finish(s, o, w, sizeof(int64_t), nf);
}

}  // namespace

namespace ss {

uint32_t field_mask_docs() { return FM_DOCS; }
uint32_t field_mask_group() { return FM_GROUP; }

void launch_field_masks(const void* params, hipStream_t st) {
    const FieldParams& p = *static_cast<const FieldParams*>(params);
    if (!p.n_sets || !p.stride) return;
    const uint64_t n_blocks = (p.stride + FM_WORDS - 1) / FM_WORDS;                  // < 2^20: n_docs < 2^32
    const uint32_t n_groups = (p.n_sets + FM_GROUP - 1) / FM_GROUP;
    const uint32_t per_launch = (uint32_t)std::max<uint64_t>(1, FM_MAX_BLOCKS / n_blocks);
    for (uint32_t g0 = 0; g0 < n_groups; g0 += per_launch) {
        const uint32_t ng = std::min(per_launch, n_groups - g0);
        hipLaunchKernelGGL(k_field_masks, dim3((unsigned)(ng * n_blocks)), dim3(FM_TPB), 0, st, p, g0, (uint32_t)n_blocks);
    }
}

}  // namespace ss

extern "C" {

int32_t ss_scorer_set_doc_fields(ss_scorer* s, int32_t n_fields, const int64_t* values) {
    if (!s) return SS_ERR_INVALID;
    ss_ctx* ctx = s->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n_fields < 0) return ctx->fail(SS_ERR_INVALID, "ss_scorer_set_doc_fields: n_fields < 0");
    if (n_fields > SS_MAX_DOC_FIELDS)
        return ctx->fail(SS_ERR_UNSUPPORTED, "ss_scorer_set_doc_fields: n_fields %d > SS_MAX_DOC_FIELDS %d", n_fields, SS_MAX_DOC_FIELDS);
    SS_HIP(ctx, hipSetDevice(ctx->device));
    const bool clear = n_fields == 0 || !values;
    ss::DevBuf<int64_t> nb;
    const size_t n = (size_t)n_fields * (size_t)s->n_docs;
    if (!clear) SS_HIP(ctx, nb.alloc(std::max<size_t>(n, 1)));                       // (a failure here leaves the old table in place)
    // the scorer's outstanding batches (pipelined calls, tickets) may read the old table — k_field_masks on a wave stream, the sort and
    // read-out kernels on the context's stream —: drained, as ss_scorer_set_doc_masks does, before the table is replaced
    SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t ws : ctx->wave_stream)
        if (ws) SS_HIP(ctx, hipStreamSynchronize(ws));
    if (clear) {
        s->fields.release();
        s->n_fields = 0;
        return SS_OK;
    }
    if (n) {
        SS_HIP(ctx, hipMemcpyAsync(nb.p, values, n * sizeof(int64_t), hipMemcpyDefault, ctx->stream));
        SS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    s->fields = std::move(nb);
    s->n_fields = n_fields;
    return SS_OK;
}

int32_t ss_doc_field_masks(ss_scorer* s, int32_t n_sets, const uint32_t* rng_ptr, const ss_doc_range* rng, const int32_t* mask_id,
                           uint32_t* words_out) {
    return hw::guarded(s, "ss_doc_field_masks", [&] { return field_masks_impl(s, n_sets, rng_ptr, rng, mask_id, words_out); });
}

int32_t ss_sort_hits_by_field(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int32_t field,
                              int32_t descending, int32_t first, int32_t k, ss_hit* hits_out, int32_t* n_hits_out, int64_t* values_out) {
    return hw::guarded(s, "ss_sort_hits_by_field", [&] { return sort_impl(s, n_q, k_in, hits, n_hits, field, descending, first, k, hits_out, n_hits_out, values_out); });
}

int32_t ss_hit_fields(ss_scorer* s, int32_t n_q, int32_t k_in, const ss_hit* hits, const int32_t* n_hits, int64_t* values_out) {
    return hw::guarded(s, "ss_hit_fields", [&] { return hit_fields_impl(s, n_q, k_in, hits, n_hits, values_out); });
}

}  // extern "C"
