// rank_model_plan.hpp — the part of ss_rank_model (rank_model.hip) that needs no device: the validation of a model with
// its messages and the model's figures, the 16-byte node the kernels walk, and the cut of the forest into chunks of consecutive whole
// trees that k_forest_eval loads into the LDS.  The constexpr functions are compiled for both sides (the kernel calls chunk_end and the
// link accessors; tests/rank_model_plan_harness.cpp runs everything on the host under ASan + UBSan).  Includes nothing of HIP.
//
// The safety argument of the kernels is check_model's: a split's children have larger indices than the split and lie inside the tree,
// so a walk from node 0 visits strictly ascending indices and ends within the tree's node count, on any feature values.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ss {
namespace rankp {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 2 };              // what a check returns; rank_model.hip maps them to the ABI's codes
constexpr int32_t MAX_FEATURES = 64;                        // SS_MAX_RANK_FEATURES (rank_model.hip asserts the equality)
constexpr int32_t MAX_TREES = 8192;                         // SS_MAX_RANK_TREES (likewise)
constexpr uint64_t MAX_NODES = 1ull << 24;                  // of a whole model: a child index fits 24 bits of a link
// "rank.lds_nodes": nodes of one LDS chunk.  The ceiling is what k_forest_eval declares: 1024 nodes x 16 bytes = 16 KiB beside the
// 32 KiB feature tile (256 rows x 16 columns, or 64 rows x 64 columns, of float64): 48 KiB of the 64 KiB static limit, three
// workgroups per CU.  The default is the ceiling: a larger chunk means fewer barriers, and nothing else changes with it.
constexpr int64_t LDS_NODES_DEFAULT = 1024, LDS_NODES_MAX = 1024;

// a node as the ABI passes it: the layout of ss_tree_node (rank_model.hip asserts size and offsets)
struct Node { int32_t feature; uint32_t left, right, nan_left; double value; };
// ... and as the kernels read it: the value, and feature + 1 (0: a leaf) | nan_left | right | left in one word
struct PNode { double value; uint64_t link; };
constexpr uint64_t pack_link(int32_t feature, uint32_t left, uint32_t right, uint32_t nan_left) {
    return feature < 0 ? 0ull : (uint64_t)left | (uint64_t)right << 24 | (uint64_t)(uint32_t)(feature + 1) << 48 | (uint64_t)nan_left << 55;
}
constexpr bool link_is_leaf(uint64_t link) { return ((link >> 48) & 0x7Full) == 0; }
constexpr uint32_t link_feature(uint64_t link) { return (uint32_t)((link >> 48) & 0x7Full) - 1u; }   // (of a split)
constexpr uint32_t link_left(uint64_t link) { return (uint32_t)(link & 0xFFFFFFull); }
constexpr uint32_t link_right(uint64_t link) { return (uint32_t)((link >> 24) & 0xFFFFFFull); }
constexpr bool link_nan_left(uint64_t link) { return ((link >> 55) & 1ull) != 0; }
static_assert(MAX_FEATURES <= 0x7F - 1 && MAX_NODES <= (1ull << 24), "a link holds feature + 1 in 7 bits and a child in 24");

struct Info {                                               // the layout of ss_rank_model_info (likewise asserted)
    int32_t n_features, n_trees;
    uint32_t n_nodes, max_tree_nodes;                       // nodes of the model, of its largest tree
    uint32_t max_depth, pad;                                // splits on the longest path from a node 0 to a leaf
};

// Everything ss_rank_model_create refuses, in the order of the header's list; fills `info` when the model passes.
inline int check_model(char* msg, size_t cap, const char* entry, int32_t n_features, const double* linear, double base, int32_t n_trees,
                       const uint32_t* tree_ptr, const Node* nodes, Info* info) {
    if (n_features < 1) { std::snprintf(msg, cap, "%s: n_features = %d, must be >= 1", entry, n_features); return INVALID; }
    if (n_trees < 0) { std::snprintf(msg, cap, "%s: n_trees < 0", entry); return INVALID; }
    if (n_features > MAX_FEATURES) { std::snprintf(msg, cap, "%s: n_features %d > SS_MAX_RANK_FEATURES %d", entry, n_features, MAX_FEATURES); return UNSUPPORTED; }
    if (n_trees > MAX_TREES) { std::snprintf(msg, cap, "%s: n_trees %d > SS_MAX_RANK_TREES %d", entry, n_trees, MAX_TREES); return UNSUPPORTED; }
    if (!std::isfinite(base)) { std::snprintf(msg, cap, "%s: base is not finite", entry); return INVALID; }
    if (linear)
        for (int32_t f = 0; f < n_features; f++)
            if (!std::isfinite(linear[f])) { std::snprintf(msg, cap, "%s: linear[%d] is not finite", entry, f); return INVALID; }
    *info = Info{n_features, n_trees, 0u, 0u, 0u, 0u};
    if (n_trees == 0) return OK;
    if (!tree_ptr) { std::snprintf(msg, cap, "%s: tree_ptr is NULL", entry); return INVALID; }
    if (tree_ptr[0] != 0) { std::snprintf(msg, cap, "%s: tree_ptr[0] = %u, must be 0", entry, tree_ptr[0]); return INVALID; }
    for (int32_t t = 0; t < n_trees; t++) {
        if (tree_ptr[t + 1] < tree_ptr[t]) { std::snprintf(msg, cap, "%s: tree_ptr decreases at tree %d", entry, t); return INVALID; }
        if (tree_ptr[t + 1] == tree_ptr[t]) { std::snprintf(msg, cap, "%s: tree %d is empty", entry, t); return INVALID; }
    }
    if ((uint64_t)tree_ptr[n_trees] > MAX_NODES) { std::snprintf(msg, cap, "%s: %u nodes, at most 2^24", entry, tree_ptr[n_trees]); return UNSUPPORTED; }
    if (!nodes) { std::snprintf(msg, cap, "%s: nodes is NULL", entry); return INVALID; }
    std::vector<uint32_t> depth;                            // splits above a node; NONE: not reached from node 0
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    for (int32_t t = 0; t < n_trees; t++) {
        const Node* const tr = nodes + tree_ptr[t];
        const uint32_t size = tree_ptr[t + 1] - tree_ptr[t];
        depth.assign(size, NONE);
        depth[0] = 0;
        for (uint32_t i = 0; i < size; i++) {
            const Node& nd = tr[i];
            if (nd.feature < -1 || nd.feature >= n_features) {
                std::snprintf(msg, cap, "%s: tree %d node %u: feature %d outside [-1, %d)", entry, t, i, nd.feature, n_features);
                return INVALID;
            }
            if (nd.feature < 0) {
                if (!std::isfinite(nd.value)) { std::snprintf(msg, cap, "%s: tree %d node %u: leaf value is not finite", entry, t, i); return INVALID; }
                if (depth[i] != NONE && depth[i] > info->max_depth) info->max_depth = depth[i];
                continue;
            }
            if (nd.left <= i || nd.left >= size || nd.right <= i || nd.right >= size) {
                std::snprintf(msg, cap, "%s: tree %d node %u: children %u / %u, must be in (%u, %u)", entry, t, i, nd.left, nd.right, i, size);
                return INVALID;
            }
            if (nd.nan_left > 1) { std::snprintf(msg, cap, "%s: tree %d node %u: nan_left = %u", entry, t, i, nd.nan_left); return INVALID; }
            if (nd.value != nd.value) { std::snprintf(msg, cap, "%s: tree %d node %u: split value is NaN", entry, t, i); return INVALID; }
            if (depth[i] != NONE) {                         // (children come later: their depth is final when the loop gets there)
                const uint32_t d = depth[i] + 1;
                if (depth[nd.left] == NONE || depth[nd.left] < d) depth[nd.left] = d;
                if (depth[nd.right] == NONE || depth[nd.right] < d) depth[nd.right] = d;
            }
        }
        if (size > info->max_tree_nodes) info->max_tree_nodes = size;
    }
    info->n_nodes = tree_ptr[n_trees];
    return OK;
}

// the nodes of a checked model as the kernels read them
inline void pack_nodes(const Node* nodes, size_t n, PNode* out) {
    for (size_t i = 0; i < n; i++) out[i] = PNode{nodes[i].value, pack_link(nodes[i].feature, nodes[i].left, nodes[i].right, nodes[i].nan_left)};
}

// ---- the chunks: the forest is walked as runs of consecutive whole trees, [t, chunk_end(t)) after each other from t = 0.  A run holds
// at most `cap` nodes and is as long as that allows; a tree with more nodes than `cap` is a run of its own, walked from global memory.
// The trees of a run are walked in order, so the order of a row's additions is the tree order for every cap.
constexpr uint32_t clamp_cap(int64_t v) { return (uint32_t)(v < 1 ? 1 : v > LDS_NODES_MAX ? LDS_NODES_MAX : v); }
constexpr uint32_t chunk_end(const uint32_t* tree_ptr, uint32_t n_trees, uint32_t t, uint32_t cap) {
    uint32_t e = t + 1;
    if (tree_ptr[e] - tree_ptr[t] > cap) return e;
    while (e < n_trees && tree_ptr[e + 1] - tree_ptr[t] <= cap) e++;
    return e;
}
struct Chunk { uint32_t first_tree, n_trees, first_node, n_nodes; bool global; };
// the same cut as a list, for the host: what the kernel does step by step
inline std::vector<Chunk> chunks(const uint32_t* tree_ptr, uint32_t n_trees, uint32_t cap) {
    std::vector<Chunk> out;
    for (uint32_t t = 0; t < n_trees;) {
        const uint32_t e = chunk_end(tree_ptr, n_trees, t, cap);
        const uint32_t nn = tree_ptr[e] - tree_ptr[t];
        out.push_back(Chunk{t, e - t, tree_ptr[t], nn, nn > cap});
        t = e;
    }
    return out;
}

}  // namespace rankp
}  // namespace ss
