// The host side of pmx_merkle_ary_update: which nodes of a tree k leaf updates touch, and the rows the device compresses for them.
// Plain C++ with no HIP types (it compiles under -DPMX_HOSTCHECK and in the stand-alone programs of tests/merkle_plan).
//
// The node array is the one pmx_merkle_ary produces: leaves, then every level, root last; level l has n_leaves / arity^l nodes, the first
// of them at first[l] = n_leaves + n_leaves / arity + ... + n_leaves / arity^(l-1) (the level walk of pmx_merkle_shape.hpp).
//
//   S_0      = the distinct updated leaves, sorted;   S_{l+1} = distinct(S_l / arity)      (S_depth = {0}: the root)
//   rows_l   = for every p in S_l (l >= 1), in order, its arity children out of level l - 1 of the host array - at level 1 with the new
//              leaves in place (duplicates are sequential updates: the last one wins)
//   slot(q)  = rank(q / arity in S_{l+1}) * arity + q % arity   for q in S_l, 1 <= l < depth: the element of rows_{l+1} that the digest
//              of q has to replace before level l + 1 is compressed
//
// All rows lie in one array, level 1 first: row r = row_first[l] + rank(p in S_l), and digest r is the new value of node p of level l.
// The device compresses rows_1, scatters the digests to their slots of rows_2, compresses rows_2, ... - sum over l >= 1 of |S_l|
// permutations, each distinct ancestor once - and the host writes leaves and digests into the node array afterwards (merkle_update_apply),
// so a failure before that leaves the array as it was.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pmx_merkle_shape.hpp"

namespace pmx {

struct MerkleUpdatePlan {
    uint32_t arity = 0;
    size_t n_leaves = 0, depth = 0;
    std::vector<size_t> first;                  // [depth + 1]: first node of level l in the node array
    std::vector<std::vector<uint64_t>> level;   // [depth + 1]: S_l
    std::vector<size_t> winner;                 // [|S_0|]: the update that holds the final value of leaf S_0[j] (the last of its index)
    std::vector<size_t> row_first;              // [depth + 2]: first row of level l (l >= 1; entries 0 and 1 are 0), then the number of rows
    std::vector<uint64_t> upload;               // rows [n_rows][arity][4], then slots [n_rows] (slot of a root row: unused, 0)
    size_t n_rows() const { return row_first.empty() ? 0 : row_first.back(); }
    size_t level_rows(size_t l) const { return row_first[l + 1] - row_first[l]; }
    uint64_t *rows() { return upload.data(); }
    uint64_t *slots() { return upload.data() + n_rows() * arity * 4; }
    const uint64_t *slots() const { return upload.data() + n_rows() * arity * 4; }
};

// the position of the first index that names no leaf, k if there is none
inline size_t merkle_update_first_bad(const uint64_t *indices, size_t k, size_t n_leaves) {
    for (size_t i = 0; i < k; ++i)
        if (indices[i] >= n_leaves) return i;
    return k;
}

// n_leaves is a power of arity >= 2 and every index is below n_leaves (the caller's checks).  Reads `nodes`, writes nothing but the plan.
inline void merkle_update_plan(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, const uint64_t *new_leaves,
                               size_t k, MerkleUpdatePlan *plan) {
    MerkleUpdatePlan &P = *plan;
    P = MerkleUpdatePlan();
    P.arity = arity;
    P.n_leaves = n_leaves;
    for (MerkleLevel lv{0, n_leaves, arity};; lv.advance()) {
        P.first.push_back(lv.first);
        if (lv.width == 1) break;
    }
    P.depth = P.first.size() - 1;
    P.level.resize(P.depth + 1);
    P.row_first.assign(P.depth + 2, 0);
    if (k == 0) return;

    // S_0 and the update that wins each of its leaves: a stable sort keeps the updates of one index in call order
    std::vector<size_t> order(k);
    for (size_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return indices[a] < indices[b]; });
    for (size_t j = 0; j < k; ++j) {
        if (j + 1 < k && indices[order[j + 1]] == indices[order[j]]) continue;
        P.level[0].push_back(indices[order[j]]);
        P.winner.push_back(order[j]);
    }
    // S_l / arity is non-decreasing: the distinct values are the runs, and the rank of a parent is the number of runs before it
    std::vector<std::vector<uint64_t>> rank(P.depth);      // rank[l][j]: rank of S_l[j] / arity in S_{l+1}
    for (size_t l = 0; l < P.depth; ++l) {
        rank[l].reserve(P.level[l].size());
        for (uint64_t q : P.level[l]) {
            if (P.level[l + 1].empty() || P.level[l + 1].back() != q / arity) P.level[l + 1].push_back(q / arity);
            rank[l].push_back(P.level[l + 1].size() - 1);
        }
        P.row_first[l + 2] = P.row_first[l + 1] + P.level[l + 1].size();
    }
    const size_t n_rows = P.n_rows(), row_words = (size_t)arity * 4;
    P.upload.assign(n_rows * row_words + n_rows, 0);
    uint64_t *rows = P.rows(), *slots = P.slots();
    for (size_t l = 1; l <= P.depth; ++l) {
        uint64_t *out = rows + P.row_first[l] * row_words;
        for (uint64_t p : P.level[l]) {
            std::memcpy(out, nodes + (P.first[l - 1] + (size_t)p * arity) * 4, row_words * 8);
            out += row_words;
        }
    }
    if (P.depth) {
        for (size_t j = 0; j < P.level[0].size(); ++j)      // the new leaves into rows_1
            std::memcpy(rows + ((size_t)rank[0][j] * arity + (size_t)(P.level[0][j] % arity)) * 4, new_leaves + P.winner[j] * 4, 32);
        for (size_t l = 1; l < P.depth; ++l)
            for (size_t j = 0; j < P.level[l].size(); ++j) slots[P.row_first[l] + j] = rank[l][j] * arity + P.level[l][j] % arity;
    }
}

// digests [n_rows][4] as the device returned them: the new leaves and every digest into the node array
inline void merkle_update_apply(const MerkleUpdatePlan &P, const uint64_t *new_leaves, const uint64_t *digests, uint64_t *nodes) {
    for (size_t j = 0; j < P.level[0].size(); ++j) std::memcpy(nodes + (size_t)P.level[0][j] * 4, new_leaves + P.winner[j] * 4, 32);
    for (size_t l = 1; l <= P.depth; ++l)
        for (size_t j = 0; j < P.level[l].size(); ++j)
            std::memcpy(nodes + (P.first[l] + (size_t)P.level[l][j]) * 4, digests + (P.row_first[l] + j) * 4, 32);
}

}  // namespace pmx
