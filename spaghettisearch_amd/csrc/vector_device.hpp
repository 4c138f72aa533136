// vector_device.hpp — the device code vector.hip (K4o) and vector_lists.hip (K4q) share: the 64-bit key of a (score, doc) pair, the exact
// radix select of a workgroup, the cut of a query's LDS candidate list back to its k largest keys, and the merge of a query's partial
// lists into rows.  Moved here from vector.hip unchanged; the kernels stay in their files.
#pragma once
#include "scorer.hpp"
#include "vector_plan.hpp"

namespace ss {
namespace vecdev {

constexpr uint32_t VT_TILE = ss::vec::TILE, VT_WAVES = ss::vec::WAVES;
constexpr int VT_TPB = VT_WAVES * 64;
constexpr int VM_TPB = 256;
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t vec_key(int32_t score, uint32_t doc) {
    return (uint64_t)((uint32_t)score ^ 0x80000000u) << 32 | (uint64_t)(0xFFFFFFFFu - doc);
}

// The k-th largest (k >= 1) of n > = k distinct-or-not 64-bit keys, by all NT threads of the workgroup: 8 passes over the keys, most
// significant digit first; s_hist: 256 counters, s_sel: 2 words.  Every thread returns the same value.  Control flow must be uniform.
template <int NT>
__device__ uint64_t block_select(const uint64_t* keys, uint32_t n, uint32_t k, uint32_t* s_hist, uint32_t* s_sel) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint64_t prefix = 0, mask = 0;
    uint32_t need = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (uint32_t b = tid; b < 256; b += NT) s_hist[b] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += NT) {
            const uint64_t key = keys[i];
            if ((key & mask) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                                           // wave 0: lane l owns bins 255 - 4l .. 252 - 4l
            uint32_t c[4], sum = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) { c[b] = s_hist[255u - 4u * lane - (uint32_t)b]; sum += c[b]; }
            uint32_t incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= (uint32_t)d) incl += o;
            }
            uint32_t run = incl - sum;
            if (run < need && need <= incl) {                                     // exactly one lane
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    if (need <= run + c[b]) { s_sel[0] = 255u - 4u * lane - (uint32_t)b; s_sel[1] = run; break; }
                    run += c[b];
                }
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_sel[0] << shift;
        mask |= (uint64_t)255u << shift;
        need -= s_sel[1];
    }
    return prefix;
}

// Cut query ql's list back to its k largest keys (n > k of them stand in buf); the k-th becomes the threshold.  Uniform.
__device__ inline void vec_compact(uint64_t* buf, uint32_t n, uint32_t k, uint64_t* thr_out, uint32_t* cnt_out, uint32_t* s_hist, uint32_t* s_sel,
                                   uint16_t* s_holes) {
    const uint32_t tid = threadIdx.x;
    const uint64_t thr = block_select<VT_TPB>(buf, n, k, s_hist, s_sel);
    if (tid == 0) { s_sel[2] = 0; s_sel[3] = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < k; i += VT_TPB)                                    // slots of the first k that fall out ...
        if (buf[i] < thr) s_holes[atomicAdd(&s_sel[2], 1u)] = (uint16_t)i;
    __syncthreads();
    for (uint32_t i = k + tid; i < n; i += VT_TPB) {                              // ... take the keys behind them that stay: as many, the keys are distinct
        const uint64_t key = buf[i];
        if (key >= thr) buf[s_holes[atomicAdd(&s_sel[3], 1u)]] = key;
    }
    if (tid == 0) { *thr_out = thr; *cnt_out = k; }
    __syncthreads();
}

// One workgroup of VM_TPB threads, one query: the k-th largest key over the n_slots keys of its partial lists (unused slots 0) by the
// same select, the keys at or above it sorted in LDS (bitonic, <= 1024), rows and count written.  s_key [SS_MAX_TOPK], s_hist [256],
// s_sel [4].
__device__ inline void vec_merge_query(const uint64_t* keys, uint32_t n_slots, uint32_t k, ss_vec_hit* rows_out, int32_t* n_out_ptr,
                                       uint64_t* s_key, uint32_t* s_hist, uint32_t* s_sel) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_sel[2] = 0; s_sel[3] = 0; }
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_slots; i += VM_TPB) mine += keys[i] != 0;
    if (mine) atomicAdd(&s_sel[2], mine);
    __syncthreads();
    const uint32_t valid = s_sel[2];
    const uint32_t n_out = valid < k ? valid : k;
    uint64_t thr = 1;                                                             // every key
    if (valid > k) thr = block_select<VM_TPB>(keys, n_slots, k, s_hist, s_sel);
    for (uint32_t i = tid; i < n_slots; i += VM_TPB) {
        const uint64_t key = keys[i];
        if (key >= thr) s_key[atomicAdd(&s_sel[3], 1u)] = key;                    // n_out of them: the keys are distinct
    }
    uint32_t np = 1;
    while (np < n_out) np <<= 1;
    __syncthreads();
    for (uint32_t i = n_out + tid; i < np; i += VM_TPB) s_key[i] = 0;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= np; k2 <<= 1)
        for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (uint32_t i = tid; i < np; i += VM_TPB) {
                const uint32_t o = i ^ j2;
                if (o > i) {
                    const uint64_t a = s_key[i], b = s_key[o];
                    if ((a < b) == ((i & k2) == 0)) { s_key[i] = b; s_key[o] = a; }   // descending
                }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < n_out; i += VM_TPB) {
        const uint64_t key = s_key[i];
        ss_vec_hit row;
        row.doc = 0xFFFFFFFFu - (uint32_t)key;
        row.score = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
        rows_out[i] = row;
    }
    if (tid == 0) *n_out_ptr = (int32_t)n_out;
}

}  // namespace vecdev
}  // namespace ss
