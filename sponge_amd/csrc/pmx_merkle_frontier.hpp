// The index arithmetic of the fixed-depth trees (pmx_merkle_fixed*, pmx_merkle_frontier_append): what one append of m leaves to a tree of
// n leaves lays into the device array, level by level.  Plain C++ with no HIP types (host code only; tests/merkle_fixed compiles it with
// g++ under ASan + UBSan).
//
// A tree of arity k and depth D has k^D leaf positions; position i >= n holds the default leaf e[0], an empty subtree of height l the
// digest e[l].  Node j of level l is COMPLETE iff (j + 1) k^l <= n and PARTIAL iff it is not complete and j k^l < n: a level has
// f_l = floor(n / k^l) complete nodes and at most one partial node, node f_l, which exists iff n mod k^l != 0.  The frontier of level
// l < D is the complete nodes k floor(f_l / k) .. f_l - 1, digit l of n in base k of them.
//
// Appending m leaves, with g_l = floor((n + m) / k^l): the children row of level l holds, contiguously from slot 0,
//   kept     the d_l = f_l mod k frontier nodes (node k floor(f_l / k) is slot 0),
//   fresh    the g_l - f_l nodes that become complete (level 0: the new leaves),
//   partial  node g_l if (n + m) mod k^l != 0,
//   pads     copies of e[l] up to the next multiple of k,
// and ONE compression launch over parents = ceil(rows / k) rows writes fresh and partial of level l + 1 behind that level's kept nodes:
// (g_l - k f_{l+1} + partial_l) / k rounded up is (g_{l+1} - f_{l+1}) + partial_{l+1}.  The new frontier of level l is the
// (n + m) / k^l mod k slots from slot k floor(g_l / k) - k floor(f_l / k) on.  Level D is the root alone.
//
// The device array, in elements of 4 words: the caller's frontier [D][k - 1] and the default digests [D + 1] as uploaded (`in_*`), the
// new frontier [D][k - 1] and the root as downloaded (`out_*`), then the rows of the levels.  `place` (before the walk: kept nodes and pads
// into the rows) and `gather` (behind it: the new frontier and the root out of the rows) are lists of (destination, source) element pairs
// for launch_node_place.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pmx {

enum class FrontierError { ok, arity, depth, pow_overflow, too_many, no_leaves, bytes_overflow };
using u128 = unsigned __int128;

// arity^depth, at most 2^64 (which a 64-bit count cannot hold: hence 128 bits)
inline FrontierError frontier_capacity(uint32_t arity, size_t depth, u128 *capacity) {
    if (arity < 2) return FrontierError::arity;
    if (depth == 0 || depth > 64) return FrontierError::depth;
    u128 c = 1;
    for (size_t l = 0; l < depth; ++l) {
        c *= arity;
        if (c > ((u128)1 << 64)) return FrontierError::pow_overflow;
    }
    *capacity = c;
    return FrontierError::ok;
}

struct FrontierLevel {
    uint64_t first = 0;        // the node (index in its level) in slot 0 of the row: k floor(f_l / k)
    uint64_t kept = 0;         // frontier nodes of the tree of n leaves: digit l of n
    uint64_t fresh = 0;        // nodes that become complete
    uint64_t partial = 0;      // 1: the partial node of the tree of n + m leaves follows them
    uint64_t pads = 0;         // copies of e[l] up to the row's end
    uint64_t parents = 0;      // rows of this level's compression launch (level D: 0)
    uint64_t digit = 0;        // frontier nodes of the tree of n + m leaves: digit l of n + m
    uint64_t digit_slot = 0;   // the slot of the first of them
    size_t offset = 0;         // the row's slot 0 in the device array
    uint64_t rows() const { return kept + fresh + partial; }
};

struct FrontierPlan {
    uint32_t arity = 0;
    size_t depth = 0;
    uint64_t n = 0, m = 0;
    std::vector<FrontierLevel> level;      // [depth + 1]
    size_t in_frontier = 0, in_defaults = 0, out_frontier = 0, out_root = 0, elements = 0;
    std::vector<uint64_t> place, gather;   // (destination, source) pairs
    // The root is node 0 of level D.  The walk computes it whenever anything below it is kept, fresh or partial; of an empty tree it is
    // e[D]; a FULL tree that nothing is appended to has no frontier node at all, and its root cannot be told from its frontier.
    bool root_computed = false, root_is_default = false;
    size_t frontier_elements() const { return depth * (size_t)(arity - 1); }
};

// (n, m, arity, depth) as the caller gave them; m is one piece (its rows must fit the device array: m * 32 bytes and a third more)
inline FrontierError frontier_plan(uint64_t n, uint64_t m, uint32_t arity, size_t depth, FrontierPlan *plan) {
    u128 capacity = 0;
    if (FrontierError e = frontier_capacity(arity, depth, &capacity); e != FrontierError::ok) return e;
    if ((u128)n + m > capacity || (u128)n + m > UINT64_MAX) return FrontierError::too_many;      // (2^64 leaves do not fit a count)
    if (m > (SIZE_MAX / 32) / 4) return FrontierError::bytes_overflow;
    FrontierPlan &P = *plan;
    P.arity = arity, P.depth = depth, P.n = n, P.m = m;
    P.level.assign(depth + 1, FrontierLevel());
    P.place.clear(), P.gather.clear();
    const uint64_t k = arity, total = n + m;
    const size_t fe = P.frontier_elements();
    P.in_frontier = 0, P.in_defaults = fe, P.out_frontier = fe + depth + 1, P.out_root = P.out_frontier + fe;
    size_t cursor = P.out_root + 1;
    // f = floor(n / k^l) and g = floor((n + m) / k^l) level by level (floor division nests); below: some digit of n + m under level l is
    // not zero, which is (n + m) mod k^l != 0.  At l = D with k^D = 2^64 both quotients are 0, as the last division leaves them.
    uint64_t f = n, g = total, below = 0;
    for (size_t l = 0; l <= depth; ++l) {
        FrontierLevel &L = P.level[l];
        L.fresh = g - f;
        L.partial = below;
        L.offset = cursor;
        if (l < depth) {
            L.kept = f % k, L.first = f - L.kept;
            L.digit = g % k, L.digit_slot = (g - L.digit) - L.first;
            L.parents = L.rows() / k + (L.rows() % k ? 1 : 0);
            L.pads = L.parents * k - L.rows();
            for (uint64_t j = 0; j < L.kept; ++j) P.place.push_back(L.offset + j), P.place.push_back(P.in_frontier + l * (k - 1) + j);
            for (uint64_t j = 0; j < L.pads; ++j) P.place.push_back(L.offset + L.rows() + j), P.place.push_back(P.in_defaults + l);
            for (uint64_t j = 0; j < L.digit; ++j)
                P.gather.push_back(P.out_frontier + l * (k - 1) + j), P.gather.push_back(L.offset + L.digit_slot + j);
            cursor += (size_t)(L.parents * k);
            if (L.digit) below = 1;
            f /= k, g /= k;
        } else {
            cursor += 1;                          // (level D: the root's slot, written iff rows() == 1)
        }
    }
    P.elements = cursor;
    P.root_computed = P.level[depth].rows() == 1;
    P.root_is_default = total == 0;
    if (P.root_computed) P.gather.push_back(P.out_root), P.gather.push_back(P.level[depth].offset);
    return FrontierError::ok;
}

// The dense form (pmx_merkle_fixed): level l of the tree over n_leaves >= 1 leaves stores max(1, ceil(n_leaves / k^l)) nodes - its complete
// nodes and its partial one -, packed, leaves first and root last.  first [depth + 2]: the first node of level l, then the number of nodes.
inline FrontierError fixed_shape(uint64_t n_leaves, uint32_t arity, size_t depth, std::vector<size_t> *first) {
    u128 capacity = 0;
    if (FrontierError e = frontier_capacity(arity, depth, &capacity); e != FrontierError::ok) return e;
    if (n_leaves == 0) return FrontierError::no_leaves;
    if ((u128)n_leaves > capacity) return FrontierError::too_many;
    first->assign(depth + 2, 0);
    u128 pw = 1, nodes = 0;
    for (size_t l = 0; l <= depth; ++l, pw *= arity) {
        (*first)[l] = (size_t)nodes;
        const u128 width = ((u128)n_leaves + pw - 1) / pw;      // >= 1
        nodes += width;
        if (nodes > SIZE_MAX / 32) return FrontierError::bytes_overflow;
    }
    (*first)[depth + 1] = (size_t)nodes;
    return FrontierError::ok;
}

}  // namespace pmx
