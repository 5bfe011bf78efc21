// How a Merkle tree is laid out in its node array - the one place that knows.  Plain C++ with no HIP types (host code only: no device
// translation unit includes it; tests/merkle_shape compiles it with g++).
//
// The node array holds the leaves, then every level, root last.  Level l + 1 has ceil(width_l / arity) nodes: on a tree of arity^depth
// leaves every level divides and the ceiling is the floor; on any other leaf count the last parent of a level that does not divide has
// the children that exist.  n_trees trees of arity^depth leaves each, laid out tree after tree, are the first `depth` levels of one tree
// over all their leaves: the walk stops at a width of n_trees instead of 1.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pmx {

enum class MerkleShapeError { ok, arity, no_leaves, not_power, tree_overflow, no_trees, forest_overflow, pow_overflow };

// the level cursor: `width` nodes, the first of them at node `first`
struct MerkleLevel {
    size_t first, width;
    uint32_t arity;
    size_t parents() const { return width / arity + (width % arity ? 1 : 0); }
    void advance() {
        const size_t up = parents();
        first += width;
        width = up;
    }
};

struct MerkleShape {
    size_t depth = 0, n_nodes = 0;
};

// exact: n_leaves must be a power of the arity.  Refused when n_nodes * 32 does not fit size_t.  Writes *out only on success.
inline MerkleShapeError merkle_shape(size_t n_leaves, uint32_t arity, bool exact, MerkleShape *out) {
    if (arity < 2) return MerkleShapeError::arity;
    if (n_leaves == 0) return MerkleShapeError::no_leaves;
    size_t depth = 0;
    for (MerkleLevel lv{0, n_leaves, arity};; lv.advance(), ++depth) {
        if (lv.width > SIZE_MAX / 32 - lv.first) return MerkleShapeError::tree_overflow;
        if (lv.width == 1) {
            *out = MerkleShape{depth, lv.first + 1};
            return MerkleShapeError::ok;
        }
        if (exact && lv.width % arity) return MerkleShapeError::not_power;
    }
}

// n_trees exact trees.  The bound on the forest's bytes is its entry family's own: the 2-to-1 forest (pair_bound) has always refused
// n_trees > (SIZE_MAX / 128) / leaves_per_tree, the forest of any arity n_trees > (SIZE_MAX / 32) / tree_nodes.
inline MerkleShapeError merkle_forest_shape(size_t n_trees, size_t leaves_per_tree, uint32_t arity, bool pair_bound, size_t *total_leaves,
                                            size_t *total_nodes) {
    MerkleShape tree;
    if (MerkleShapeError e = merkle_shape(leaves_per_tree, arity, true, &tree); e != MerkleShapeError::ok) return e;
    if (n_trees == 0) return MerkleShapeError::no_trees;
    if (n_trees > (pair_bound ? (SIZE_MAX / 128) / leaves_per_tree : (SIZE_MAX / 32) / tree.n_nodes)) return MerkleShapeError::forest_overflow;
    *total_leaves = n_trees * leaves_per_tree;
    *total_nodes = n_trees * tree.n_nodes;
    return MerkleShapeError::ok;
}

// arity^depth, the number of leaves of a tree given by its depth; refused when it does not fit 64 bits
inline MerkleShapeError merkle_leaves_of_depth(uint32_t arity, size_t depth, uint64_t *out) {
    if (arity < 2) return MerkleShapeError::arity;
    uint64_t n = 1;
    for (size_t l = 0; l < depth; ++l) {
        if (n > UINT64_MAX / arity) return MerkleShapeError::pow_overflow;
        n *= arity;
    }
    *out = n;
    return MerkleShapeError::ok;
}

// Leaf updates: the first level l whose parents are no more than the k updates - from there on an update runs whole levels - or the
// depth if there is none.  (arity >= 2, n_leaves >= 1)
inline size_t merkle_update_switch_level(size_t n_leaves, uint32_t arity, size_t k) {
    size_t l = 0;
    for (MerkleLevel lv{0, n_leaves, arity}; lv.width > 1 && k < lv.parents(); lv.advance()) ++l;
    return l;
}

}  // namespace pmx
