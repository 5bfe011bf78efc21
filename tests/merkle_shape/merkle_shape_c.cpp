// pmx_merkle_shape.hpp (the layout of every Merkle tree of the library) behind a C interface, for tests/test_merkle_shape.py.
// Error codes are the enum's values: 0 ok, 1 arity, 2 no leaves, 3 not a power, 4 tree overflow, 5 no trees, 6 forest overflow, 7 power overflow.
#include <cstdint>

#include "pmx_merkle_shape.hpp"

using namespace pmx;

extern "C" {

int ms_shape(size_t n_leaves, uint32_t arity, int exact, size_t *depth, size_t *n_nodes) {
    MerkleShape s;
    const MerkleShapeError e = merkle_shape(n_leaves, arity, exact != 0, &s);
    if (e == MerkleShapeError::ok) *depth = s.depth, *n_nodes = s.n_nodes;
    return (int)e;
}
int ms_forest(size_t n_trees, size_t leaves_per_tree, uint32_t arity, int pair_bound, size_t *total_leaves, size_t *total_nodes) {
    return (int)merkle_forest_shape(n_trees, leaves_per_tree, arity, pair_bound != 0, total_leaves, total_nodes);
}
int ms_leaves_of_depth(uint32_t arity, size_t depth, uint64_t *out) { return (int)merkle_leaves_of_depth(arity, depth, out); }
size_t ms_switch_level(size_t n_leaves, uint32_t arity, size_t k) { return merkle_update_switch_level(n_leaves, arity, k); }
// the cursor walked from the leaves to the root: first[l], width[l] for l = 0 .. (at most cap levels are written); returns the level count
size_t ms_walk(size_t n_leaves, uint32_t arity, size_t *first, size_t *width, size_t cap) {
    size_t l = 0;
    for (MerkleLevel lv{0, n_leaves, arity};; lv.advance(), ++l) {
        if (l < cap) first[l] = lv.first, width[l] = lv.width;
        if (lv.width <= 1) return l + 1;
    }
}

}  // extern "C"
