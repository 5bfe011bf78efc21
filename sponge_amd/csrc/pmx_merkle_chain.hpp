// The host plan of pmx_merkle_update_witnesses: k sequential leaf updates of a fixed-depth tree, walked level by level instead of update
// by update.  Plain C++ with no HIP types (host code only; tests/merkle_chain compiles it with g++ under ASan + UBSan).
//
// Update j changes leaf indices[j]; its running node at level l is q_l = indices[j] / arity^l, and the sibling in slot s of that node is
// node (q_l - digit) + (s < digit ? s : s + 1), digit = q_l mod arity.  What update j sees in that sibling is what the LAST update before
// it left there: pred[l][j][s] = the largest j' < j whose running node at level l is that sibling, or kChainNone - then the sibling is
// still what the caller's old opening says.  The value update j' left in its running node of level l is V_l[j'], so once pred is known
// every level is k independent rows: the device gathers (pmx_tree_moves.hip: chain_rows_kernel) and compresses them in one launch each.
//
// Per level the plan is a map from node index to the last update that wrote it, kept as a flat table: siblings share their parent, so
// the table is last[rank of the parent among the level's distinct parents][digit].  Floor division is monotone, so ONE sort of the
// updates by leaf index orders them by running node at every level, and the ranks of a level's parents fall out of one scan of that
// order: O(k log k) once, O(k arity) per level, no O(k^2) path.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace pmx {

constexpr uint32_t kChainNone = 0xffffffffu;              // no earlier update wrote the sibling
constexpr size_t kChainMaxUpdates = 0xfffffffeu;          // pred is 32 bits wide and kChainNone is no update

// the first update whose index names no leaf position (capacity = arity^depth; 2^64 as 0 with `all` set), k if there is none
inline size_t chain_first_bad(const uint64_t *indices, size_t k, uint64_t capacity, bool all) {
    if (all) return k;
    for (size_t j = 0; j < k; ++j)
        if (indices[j] >= capacity) return j;
    return k;
}

class ChainPlanner {
public:
    // k <= kChainMaxUpdates, arity >= 2 (the caller's checks)
    ChainPlanner(const uint64_t *indices, size_t k, uint32_t arity)
        : k_(k), arity_(arity), q_(indices, indices + k), order_(k), rank_(k), last_() {
        std::iota(order_.begin(), order_.end(), (uint32_t)0);
        std::sort(order_.begin(), order_.end(), [&](uint32_t x, uint32_t y) { return q_[x] < q_[y]; });
    }
    // pred_out [k][arity - 1] of the next level (the first call: level 0); then the running nodes move up one level
    void next_level(uint32_t *pred_out) {
        const size_t sib = arity_ - 1;
        // rank of every update's parent among the level's distinct parents, in the one order that sorts every level
        uint32_t parents = 0;
        uint64_t prev = 0;
        for (size_t i = 0; i < k_; ++i) {
            const uint32_t j = order_[i];
            const uint64_t p = q_[j] / arity_;
            if (i && p != prev) ++parents;
            rank_[j] = parents;
            prev = p;
        }
        if (k_) ++parents;
        last_.assign((size_t)parents * arity_, kChainNone);
        for (size_t j = 0; j < k_; ++j) {
            const uint32_t digit = (uint32_t)(q_[j] % arity_);
            uint32_t *row = last_.data() + (size_t)rank_[j] * arity_;
            for (size_t s = 0; s < sib; ++s) pred_out[j * sib + s] = row[s < digit ? s : s + 1];
            row[digit] = (uint32_t)j;
            q_[j] /= arity_;
        }
    }

private:
    size_t k_;
    uint32_t arity_;
    std::vector<uint64_t> q_;        // the running node of every update at the level next_level plans next
    std::vector<uint32_t> order_;    // the updates sorted by leaf index
    std::vector<uint32_t> rank_;
    std::vector<uint32_t> last_;     // [parents][arity]: the last update whose running node is that child
};

}  // namespace pmx
