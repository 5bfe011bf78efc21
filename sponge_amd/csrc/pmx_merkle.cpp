// Every pmx_merkle_* entry point of include/poseidon_mi355x.h: the 2-to-1 trees and forests, the trees of any arity (a power of the arity
// leaves) and the trees over any number of leaves (pmx_merkle_ragged*), built on one set of bodies.  A parent is (new; absorb(its
// children); squeeze_native(1))[0], one permutation for arity <= rate (mod.rs:126-135, 219-230, 324-328); the last parent of a level that
// does not divide absorbs the children that exist.  The layout is pmx_merkle_shape.hpp's.  The three families are one thing: at arity 2
// every array of the arity-k entries is byte for byte the one the 2-to-1 entries produce and accept, and at n_leaves = arity^depth every
// launch of a ragged builder is the one pmx_merkle_ary* makes (launch_compress_level on a level that divides is launch_compress_ary,
// which at arity 2 is launch_compress).  What stays per entry is its name in the null-pointer message, its shape check with its own
// texts, and the order of its checks; the family picks between the twin gather kernels (a ragged entry launches the bounded one whatever
// the leaf count).  The *_dev entries only enqueue on the caller's stream: no allocation, no synchronisation.  The trees of a fixed depth
// (pmx_merkle_fixed*, pmx_merkle_frontier_append, at the end of the file) are the same full-row launches over rows that
// pmx_merkle_frontier.hpp lays out: host buffers only.  Their sequential leaf updates (pmx_merkle_update_witnesses, last) are `depth` launches
// of launch_compress_ary over rows a gather kernel chains by pmx_merkle_chain.hpp's plan.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"
#include "pmx_merkle_chain.hpp"
#include "pmx_merkle_frontier.hpp"
#include "pmx_merkle_plan.hpp"
#include "pmx_merkle_shape.hpp"

using namespace pmx;

namespace {

using E = MerkleShapeError;
enum class Family { pairs, pair_forest, ary, ary_forest, ragged };

// the message of a refused shape, in the words of the entry's family
int shape_error(E e, Family f) {
    switch (e) {
    case E::ok: return PMX_OK;
    case E::arity: return set_error(PMX_ERR_ARG, "arity must be at least 2");
    case E::pow_overflow: return set_error(PMX_ERR_ARG, "arity^depth overflows 64 bits");
    case E::tree_overflow:
        if (f != Family::pair_forest) return set_error(PMX_ERR_ARG, "tree byte size overflows size_t");
        [[fallthrough]];
    case E::forest_overflow: return set_error(PMX_ERR_ARG, "forest byte size overflows size_t");
    case E::no_trees:
        if (f == Family::ary_forest) return set_error(PMX_ERR_ARG, "a forest needs n_trees >= 1");
        [[fallthrough]];
    default: break;     // no leaves, not a power (and the 2-to-1 forest without trees)
    }
    if (f == Family::pairs) return set_error(PMX_ERR_ARG, "n_leaves must be a power of two");
    if (f == Family::pair_forest) return set_error(PMX_ERR_ARG, "a forest needs n_trees >= 1 and leaves_per_tree a power of two");
    if (f == Family::ragged) return set_error(PMX_ERR_ARG, "a tree needs at least one leaf");
    return set_error(PMX_ERR_ARG, "n_leaves must be a power of the arity");
}
int tree_shape(size_t n_leaves, uint32_t arity, Family f, MerkleShape *s) { return shape_error(merkle_shape(n_leaves, arity, f != Family::ragged, s), f); }
int forest_shape(size_t n_trees, size_t leaves_per_tree, uint32_t arity, Family f, size_t *total_leaves, size_t *total_nodes) {
    return shape_error(merkle_forest_shape(n_trees, leaves_per_tree, arity, f == Family::pair_forest, total_leaves, total_nodes), f);
}
// The root does not bind n_leaves of a ragged tree, so the caller of a verifier states it, and depth must be its depth.
int ragged_verify_shape(size_t depth, uint32_t arity, size_t n_leaves) {
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    if (s.depth != depth) return set_error(PMX_ERR_ARG, "depth %zu is not the depth %zu of a tree of arity %u over %zu leaves", depth, s.depth, arity, n_leaves);
    return PMX_OK;
}

// one permutation compresses at most `rate` children (absorbing more into a fresh sponge permutes in between: a hash row)
int arity_fits(const pmx_ctx *ctx, uint32_t arity) {
    if (arity == 2 && ctx->dev.rounds.rate < 2) return set_error(PMX_ERR_CONFIG, "2-to-1 compression needs rate >= 2");
    if (arity > ctx->dev.rounds.rate)
        return set_error(PMX_ERR_CONFIG, "arity %u exceeds the rate %u: more children than the rate is a hash row (pmx_hash_batch_dev), not a single compression",
                         arity, ctx->dev.rounds.rate);
    return PMX_OK;
}
int misaligned() { return set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned"); }

// ---- the shared bodies ------------------------------------------------------------------------------------------------------------
// Level by level on the caller's stream, from level `lv` until the width is `stop` (1; n_trees for a forest, whose trees advance
// together: a level of all trees is one contiguous array, and the narrowest launch is n_trees compressions wide).  (Cutting a tree into
// subtrees on concurrent streams was measured SLOWER - 7.0 ms -> 12.5 ms at 8 streams for 2^21 leaves - because the narrow levels are
// latency-bound, not launch-bound.)
int levels_dev(pmx_ctx *ctx, uint64_t *d_nodes, MerkleLevel lv, size_t stop, hipStream_t st) {
    for (; lv.width > stop; lv.advance())
        PMX_HIP(launch_compress_level(ctx->dev, ctx->t, d_nodes + lv.first * 4, d_nodes + (lv.first + lv.width) * 4, lv.arity, lv.width, st));
    return PMX_OK;
}
// every builder behind its shape check
int build_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t total_leaves, uint32_t arity, size_t n_trees, void *stream) {
    if (int rc = arity_fits(ctx, arity)) return rc;
    if (!aligned16(d_nodes)) return misaligned();
    PMX_BIND(ctx);
    return levels_dev(ctx, d_nodes, MerkleLevel{0, total_leaves, arity}, n_trees, (hipStream_t)stream);
}
// Host buffers: upload the leaves, the levels, download all nodes and / or the last n_trees (the roots).
int build_host(pmx_ctx *ctx, const uint64_t *leaves, size_t n_trees, size_t total_leaves, size_t n_nodes, uint32_t arity, uint64_t *nodes,
               uint64_t *roots) {
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    Staging node_array;
    node_array.add(n_nodes, 32);   // the leaves, then every level
    char *d = nullptr;
    if ((rc = call.stage(node_array, &d))) return rc;
    PMX_HIP(hipMemcpyAsync(d, leaves, total_leaves * 32, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = build_dev(ctx, (uint64_t *)d, total_leaves, arity, n_trees, ctx->stream))) return rc;
    if (nodes) PMX_HIP(hipMemcpyAsync(nodes, d, n_nodes * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (roots) PMX_HIP(hipMemcpyAsync(roots, (uint64_t *)d + (n_nodes - n_trees) * 4, n_trees * 32, hipMemcpyDeviceToHost, ctx->stream));
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
}

// Openings on the host: paths_out [k][depth][arity - 1][4], per level the siblings in child order with the running node's own slot left
// out; a sibling at or beyond its level's width does not exist and is four zero words (there is none on a tree of arity^depth leaves).
// Every index is checked before anything is written.
int paths_host(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices, size_t k, uint64_t *paths_out) {
    for (size_t i = 0; i < k; ++i)
        if (indices[i] >= n_leaves) return set_error(PMX_ERR_ARG, "leaf index %llu out of range", (unsigned long long)indices[i]);
    const size_t sib = arity - 1;
    for (size_t i = 0; i < k; ++i) {
        size_t idx = (size_t)indices[i];
        MerkleLevel lv{0, n_leaves, arity};
        for (size_t level = 0; level < depth; ++level, lv.advance(), idx /= arity) {
            const size_t digit = idx % arity, base = idx - digit;
            uint64_t *row = paths_out + (i * depth + level) * sib * 4;
            for (size_t s = 0; s < sib; ++s) {
                const size_t child = base + (s < digit ? s : s + 1);
                if (child < lv.width) std::memcpy(row + s * 4, nodes + (lv.first + child) * 4, 32);
                else std::memset(row + s * 4, 0, 32);
            }
        }
    }
    return PMX_OK;
}
// the same gather on the device: nodes, indices and paths stay where they are (an index >= n_leaves, which the host cannot see, gets
// an all-zero path)
int paths_dev(pmx_ctx *ctx, const uint64_t *d_nodes, size_t n_leaves, uint32_t arity, size_t depth, bool ragged, const uint64_t *d_indices, size_t k,
              uint64_t *d_paths, void *stream) {
    if (int rc = arity_fits(ctx, arity)) return rc;
    if (k == 0 || depth == 0) return PMX_OK;
    const size_t per = depth * (arity - 1);     // elements per path (depth <= 64, arity <= PMX_MAX_WIDTH)
    if (k > (SIZE_MAX / 32) / per || k > kMaxLaunchUnits / per) return set_error(PMX_ERR_ARG, "batch too large");
    if (!aligned16(d_nodes) || !aligned16(d_paths)) return misaligned();
    PMX_BIND(ctx);
    PMX_HIP((ragged ? launch_paths_gather_ragged : launch_paths_gather)(d_nodes, n_leaves, arity, depth, d_indices, d_paths, k, (hipStream_t)stream));
    return PMX_OK;
}

// k authentication paths climb one level per step, everything resident on the device: cur[i] starts as leaves[i]; per level a gather
// kernel lays the arity children of every path's parent out as the rows one tree level has - cur[i] at digit `level` of indices[i], the
// siblings of paths[i][level] around it (an absent sibling is the zero a short parent's rate lane holds) - and the compression launcher
// writes the parents back into cur.  Arity 2 gathers with shifts (launch_path_pairs: paths [k][depth][1][4] is [k][depth][4]), any other
// arity with divisions.  d_work: [k][(arity + 1) * 4] u64 of scratch (cur [k][4], then rows [k][arity][4]).  d_ok[i] = 1 iff cur[i] ==
// root after `depth` levels and indices[i] < limit.  `pairs`: the bounds on k the 2-to-1 entries have always had.
int verify_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths, size_t depth, uint32_t arity, uint64_t limit,
               bool pairs, size_t k, const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work, void *stream) {
    if (int rc = arity_fits(ctx, arity)) return rc;
    if (k == 0) return PMX_OK;
    // (depth <= 64 and arity <= PMX_MAX_WIDTH here: the products below stay small)
    if (k > kMaxLaunchUnits / (pairs ? 1 : arity) || k > (SIZE_MAX / 32) / (arity + 1) || (depth && k > (SIZE_MAX / 32) / (depth * (arity - 1))))
        return set_error(PMX_ERR_ARG, "batch too large");
    if (!aligned16(d_leaves) || !aligned16(d_paths) || !aligned16(d_work) || !aligned16(d_root)) return misaligned();
    PMX_BIND(ctx);
    hipStream_t st = (hipStream_t)stream;
    uint64_t *cur = d_work, *rows = d_work + k * 4;
    PMX_HIP(hipMemcpyAsync(cur, d_leaves, k * 32, hipMemcpyDeviceToDevice, st));
    uint64_t pow = 1;     // arity^level
    for (size_t level = 0; level < depth; ++level, pow *= arity) {
        if (arity == 2) PMX_HIP(launch_path_pairs(cur, d_paths, d_indices, depth, level, rows, k, st));
        else PMX_HIP(launch_path_children(cur, d_paths, d_indices, depth, level, pow, arity, rows, k, st));
        PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, rows, cur, arity, k, st));
    }
    PMX_HIP(launch_path_check(cur, d_root, d_indices, limit, d_ok, k, st));
    return PMX_OK;
}

// k leaves of a resident tree change: only their ancestors are recomputed, level by level.  While the k updates are fewer than the
// parents a level has, the level is  gather (the arity children of every update's parent, out of the node array; the bounded twin
// zero-fills the children a short parent does not have) -> one compression launch of k rows -> scatter (cur[i] to the parent's node:
// index / arity^(l+1) is the ancestor's index, floor division nests); two updates under one parent compute it twice and store the same
// bytes.  From merkle_update_switch_level on, the levels are the builder's own launches: an update never costs more permutations than a
// rebuild.  d_work: [k][(arity + 1) * 4] u64 of scratch (cur [k][4], then rows [k][arity][4]).  Enqueue only, nothing is allocated.
int update_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, bool ragged, const uint64_t *d_indices, const uint64_t *d_new_leaves,
               size_t k, uint64_t *d_work, void *stream) {
    if (!aligned16(d_nodes) || !aligned16(d_new_leaves) || !aligned16(d_work)) return misaligned();
    if ((uintptr_t)d_indices & 7u) return set_error(PMX_ERR_ARG, "d_indices must be 8-byte aligned");
    if (int rc = arity_fits(ctx, arity)) return rc;
    if (k == 0) return PMX_OK;
    if (k > kMaxLaunchUnits / arity || k > (SIZE_MAX / 32) / (arity + 1)) return set_error(PMX_ERR_ARG, "batch too large");
    PMX_BIND(ctx);
    hipStream_t st = (hipStream_t)stream;
    uint64_t *cur = d_work, *rows = d_work + k * 4;
    PMX_HIP(launch_node_scatter(d_new_leaves, d_indices, 1, n_leaves, 0, d_nodes, k, st));
    MerkleLevel lv{0, n_leaves, arity};
    uint64_t pow = arity;                    // arity^(l+1) (below n_leaves * arity: no overflow)
    for (size_t l = merkle_update_switch_level(n_leaves, arity, k); l > 0; --l, pow *= arity, lv.advance()) {
        if (ragged) PMX_HIP(launch_node_children_bounded(d_nodes, d_indices, pow, n_leaves, lv.first, lv.width, arity, rows, k, st));
        else PMX_HIP(launch_node_children(d_nodes, d_indices, pow, n_leaves, lv.first, arity, rows, k, st));
        PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, rows, cur, arity, k, st));
        PMX_HIP(launch_node_scatter(cur, d_indices, pow, n_leaves, lv.first + lv.width, d_nodes, k, st));
    }
    return levels_dev(ctx, d_nodes, lv, 1, st);     // the rest of the tree as whole levels
}

}  // namespace

// Host buffers (pmx_ctx.hpp): one upload of (leaves or rows, paths, root, indices), the rows hashed into the leaves by one strided-hash
// launch (row-major strides), `depth` level steps on the device, one download of ok.
int pmx::verify_host(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *rows, size_t row_len, const uint64_t *indices, const uint64_t *paths,
                     size_t depth, uint32_t arity, uint64_t limit, bool pairs, size_t k, const uint64_t *root, uint8_t *ok_out) {
    if (int rc = arity_fits(ctx, arity)) return rc;
    if (k == 0) return PMX_OK;
    Staging climb, siblings, target, verdict;
    climb.add(k, 32);                                                             // leaves [k][4]
    const size_t o_work = climb.add(k, (size_t)(arity + 1) * 32);                 // work [k][(arity + 1) * 4]
    siblings.add(k, depth * (size_t)(arity - 1) * 32);                            // paths [k][depth][arity - 1][4]
    target.add(1, 32);                                                            // root [4]
    const size_t o_idx = target.add(k, 8);                                        // indices [k]
    verdict.add(verdict.times(rows ? k : 0, row_len), 32);                        // rows [k][row_len][4] (the matrix entry)
    const size_t o_ok = verdict.add(k, 1);                                        // ok [k]
    // (all four before the first block is touched: the error a caller sees does not depend on which block is too large)
    if (climb.overflowed() || siblings.overflowed() || target.overflowed() || verdict.overflowed())
        return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    PMX_HOST_CALL(call, ctx);
    char *d_climb = nullptr, *d_paths = nullptr, *d_target = nullptr, *d_verdict = nullptr;
    int rc = PMX_OK;
    if ((rc = call.stage(climb, &d_climb)) || (rc = call.stage(siblings, &d_paths)) || (rc = call.stage(target, &d_target)) || (rc = call.stage(verdict, &d_verdict))) return rc;
    uint64_t *d_leaves = (uint64_t *)d_climb, *d_work = (uint64_t *)(d_climb + o_work), *d_root = (uint64_t *)d_target, *d_idx = (uint64_t *)(d_target + o_idx);
    hipStream_t st = ctx->stream;
    if (rows) PMX_HIP(hipMemcpyAsync(d_verdict, rows, o_ok, hipMemcpyHostToDevice, st));   // (o_ok: the rows' bytes, a multiple of 32)
    else PMX_HIP(hipMemcpyAsync(d_leaves, leaves, k * 32, hipMemcpyHostToDevice, st));
    if (siblings.bytes()) PMX_HIP(hipMemcpyAsync(d_paths, paths, siblings.bytes(), hipMemcpyHostToDevice, st));
    PMX_HIP(hipMemcpyAsync(d_root, root, 32, hipMemcpyHostToDevice, st));
    PMX_HIP(hipMemcpyAsync(d_idx, indices, k * 8, hipMemcpyHostToDevice, st));
    if (rows) PMX_HIP(launch_hash_strided(ctx->dev, ctx->t, (const uint64_t *)d_verdict, row_len, row_len, 1, d_leaves, 1, k, st));
    if ((rc = verify_dev(ctx, d_leaves, d_idx, (const uint64_t *)d_paths, depth, arity, limit, pairs, k, d_root, (uint8_t *)(d_verdict + o_ok), d_work, st))) return rc;
    PMX_HIP(hipMemcpyAsync(ok_out, d_verdict + o_ok, k, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
}

// ---- 2-to-1 trees and forests: n_leaves a power of two ---------------------------------------------------------------------------
extern "C" int pmx_merkle_2to1_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, void *stream) {
    if (!ctx || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_2to1_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, 2, Family::pairs, &s)) return rc;
    return build_dev(ctx, d_nodes, n_leaves, 2, 1, stream);
}

extern "C" int pmx_merkle_2to1(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint64_t *nodes, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_2to1")
    if (!ctx || !leaves) return set_error(PMX_ERR_ARG, "pmx_merkle_2to1: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, 2, Family::pairs, &s)) return rc;
    return build_host(ctx, leaves, 1, n_leaves, s.n_nodes, 2, nodes, root);   // (tree_shape has refused a node array beyond size_t)
    PMX_ABI_END
}

extern "C" int pmx_merkle_2to1_forest_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_trees, size_t leaves_per_tree, void *stream) {
    if (!ctx || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_2to1_forest_dev: null pointer");
    size_t total = 0, n_nodes = 0;
    if (int rc = forest_shape(n_trees, leaves_per_tree, 2, Family::pair_forest, &total, &n_nodes)) return rc;
    return build_dev(ctx, d_nodes, total, 2, n_trees, stream);
}

extern "C" int pmx_merkle_2to1_forest(pmx_ctx *ctx, const uint64_t *leaves, size_t n_trees, size_t leaves_per_tree, uint64_t *nodes,
                                      uint64_t *roots) {
    PMX_ABI_BEGIN("pmx_merkle_2to1_forest")
    if (!ctx || !leaves) return set_error(PMX_ERR_ARG, "pmx_merkle_2to1_forest: null pointer");
    size_t total = 0, n_nodes = 0;
    if (int rc = forest_shape(n_trees, leaves_per_tree, 2, Family::pair_forest, &total, &n_nodes)) return rc;
    return build_host(ctx, leaves, n_trees, total, n_nodes, 2, nodes, roots);
    PMX_ABI_END
}

extern "C" int pmx_merkle_paths(const uint64_t *nodes, size_t n_leaves, const uint64_t *indices, size_t k, uint64_t *paths_out) {
    if ((!nodes || !indices || !paths_out) && k) return set_error(PMX_ERR_ARG, "pmx_merkle_paths: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, 2, Family::pairs, &s)) return rc;
    return paths_host(nodes, n_leaves, 2, s.depth, indices, k, paths_out);
}

// (the 2-to-1 verifiers test the rate before the depth; 2^depth is the limit of the indices: one with bits at or above `depth` names no leaf)
extern "C" int pmx_merkle_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                           size_t depth, size_t k, const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work, void *stream) {
    if (!ctx || ((!d_leaves || !d_indices || !d_ok || !d_work) && k) || (!d_paths && k && depth) || !d_root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_verify_paths_dev: null pointer");
    if (int rc = arity_fits(ctx, 2)) return rc;
    if (depth >= 64) return set_error(PMX_ERR_ARG, "depth out of range");
    return verify_dev(ctx, d_leaves, d_indices, d_paths, depth, 2, (uint64_t)1 << depth, true, k, d_root, d_ok, d_work, stream);
}

extern "C" int pmx_merkle_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths,
                                       size_t depth, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out) {
    PMX_ABI_BEGIN("pmx_merkle_verify_paths")
    if (!ctx || ((!leaves || !indices || !ok_out) && k) || (!paths && k && depth) || !root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_verify_paths: null pointer");
    if (int rc = arity_fits(ctx, 2)) return rc;
    if (depth >= 64) return set_error(PMX_ERR_ARG, "depth out of range");
    return verify_host(ctx, leaves, nullptr, 0, indices, paths, depth, 2, (uint64_t)1 << depth, true, k, root, ok_out);
    PMX_ABI_END
}

// ---- trees of any arity: n_leaves a power of the arity --------------------------------------------------------------------------------
extern "C" int pmx_merkle_ary_shape(size_t n_leaves, uint32_t arity, size_t *depth, size_t *n_nodes) {
    if (!depth || !n_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_shape: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    *depth = s.depth, *n_nodes = s.n_nodes;
    return PMX_OK;
}

extern "C" int pmx_merkle_ary_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, void *stream) {
    if (!ctx || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    return build_dev(ctx, d_nodes, n_leaves, arity, 1, stream);
}

extern "C" int pmx_merkle_ary(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, uint64_t *nodes, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_ary")
    if (!ctx || !leaves) return set_error(PMX_ERR_ARG, "pmx_merkle_ary: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    if (int rc = arity_fits(ctx, arity)) return rc;
    return build_host(ctx, leaves, 1, n_leaves, s.n_nodes, arity, nodes, root);
    PMX_ABI_END
}

extern "C" int pmx_merkle_ary_forest_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_trees, size_t leaves_per_tree, uint32_t arity, void *stream) {
    if (!ctx || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_forest_dev: null pointer");
    size_t total = 0, n_nodes = 0;
    if (int rc = forest_shape(n_trees, leaves_per_tree, arity, Family::ary_forest, &total, &n_nodes)) return rc;
    return build_dev(ctx, d_nodes, total, arity, n_trees, stream);
}

extern "C" int pmx_merkle_ary_forest(pmx_ctx *ctx, const uint64_t *leaves, size_t n_trees, size_t leaves_per_tree, uint32_t arity,
                                     uint64_t *nodes, uint64_t *roots) {
    PMX_ABI_BEGIN("pmx_merkle_ary_forest")
    if (!ctx || !leaves) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_forest: null pointer");
    size_t total = 0, n_nodes = 0;
    if (int rc = forest_shape(n_trees, leaves_per_tree, arity, Family::ary_forest, &total, &n_nodes)) return rc;
    if (int rc = arity_fits(ctx, arity)) return rc;
    return build_host(ctx, leaves, n_trees, total, n_nodes, arity, nodes, roots);
    PMX_ABI_END
}

extern "C" int pmx_merkle_ary_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, size_t k,
                                    uint64_t *paths_out) {
    if ((!nodes || !indices || !paths_out) && k) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_paths: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    return paths_host(nodes, n_leaves, arity, s.depth, indices, k, paths_out);
}

extern "C" int pmx_merkle_ary_paths_dev(pmx_ctx *ctx, const uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                        size_t k, uint64_t *d_paths, void *stream) {
    if (!ctx || ((!d_nodes || !d_indices || !d_paths) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_paths_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    return paths_dev(ctx, d_nodes, n_leaves, arity, s.depth, false, d_indices, k, d_paths, stream);
}

extern "C" int pmx_merkle_ary_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                               size_t depth, uint32_t arity, size_t k, const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work,
                                               void *stream) {
    if (!ctx || ((!d_leaves || !d_indices || !d_ok || !d_work) && k) || (!d_paths && k && depth) || !d_root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_ary_verify_paths_dev: null pointer");
    uint64_t n_leaves = 0;
    if (int rc = shape_error(merkle_leaves_of_depth(arity, depth, &n_leaves), Family::ary)) return rc;
    return verify_dev(ctx, d_leaves, d_indices, d_paths, depth, arity, n_leaves, false, k, d_root, d_ok, d_work, stream);
}

extern "C" int pmx_merkle_ary_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths, size_t depth,
                                           uint32_t arity, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out) {
    PMX_ABI_BEGIN("pmx_merkle_ary_verify_paths")
    if (!ctx || ((!leaves || !indices || !ok_out) && k) || (!paths && k && depth) || !root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_ary_verify_paths: null pointer");
    uint64_t n_leaves = 0;
    if (int rc = shape_error(merkle_leaves_of_depth(arity, depth, &n_leaves), Family::ary)) return rc;
    return verify_host(ctx, leaves, nullptr, 0, indices, paths, depth, arity, n_leaves, false, k, root, ok_out);
    PMX_ABI_END
}

extern "C" int pmx_merkle_ary_update_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                         const uint64_t *d_new_leaves, size_t k, uint64_t *d_work, void *stream) {
    if (!ctx || ((!d_nodes || !d_indices || !d_new_leaves || !d_work) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_update_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    return update_dev(ctx, d_nodes, n_leaves, arity, false, d_indices, d_new_leaves, k, d_work, stream);
}

// Host buffers.  The node array stays on the host: the plan (pmx_merkle_plan.hpp) packs the children rows of every distinct ancestor, one
// upload takes them to the device with the slots their digests go to, each level is one compression launch and one scatter, one download
// brings all digests back, and only then is `nodes` written.
extern "C" int pmx_merkle_ary_update(pmx_ctx *ctx, uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices,
                                     const uint64_t *new_leaves, size_t k, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_ary_update")
    if (!ctx || !nodes || ((!indices || !new_leaves) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_ary_update: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ary, &s)) return rc;
    const size_t bad = merkle_update_first_bad(indices, k, n_leaves);     // (before anything is written)
    if (bad < k) return set_error(PMX_ERR_ARG, "leaf index %llu out of range", (unsigned long long)indices[bad]);
    if (int rc = arity_fits(ctx, arity)) return rc;
    MerkleUpdatePlan plan;
    merkle_update_plan(nodes, n_leaves, arity, indices, new_leaves, k, &plan);
    const size_t n_rows = plan.n_rows();
    std::vector<uint64_t> digests(n_rows * 4);
    if (n_rows) {
        PMX_HOST_CALL(call, ctx);
        int rc = PMX_OK;
        Staging children, parents;   // (`children` is plan.upload, byte for byte)
        children.add(n_rows, (size_t)arity * 32);                 // rows [n_rows][arity][4]
        const size_t o_slots = children.add(n_rows, 8);           // slots [n_rows]
        parents.add(n_rows, 32);                                  // digests [n_rows][4]
        char *d0 = nullptr, *d1 = nullptr;
        if ((rc = call.stage(children, &d0)) || (rc = call.stage(parents, &d1))) return rc;
        uint64_t *d_rows = (uint64_t *)d0, *d_slots = (uint64_t *)(d0 + o_slots), *d_dig = (uint64_t *)d1;
        PMX_HIP(hipMemcpyAsync(d0, plan.upload.data(), children.bytes(), hipMemcpyHostToDevice, ctx->stream));
        for (size_t l = 1; l <= s.depth; ++l) {
            const size_t r = plan.row_first[l], count = plan.level_rows(l);
            PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, d_rows + r * arity * 4, d_dig + r * 4, arity, count, ctx->stream));
            if (l < s.depth)
                PMX_HIP(launch_node_scatter(d_dig + r * 4, d_slots + r, 1, plan.level_rows(l + 1) * arity, plan.row_first[l + 1] * arity, d_rows,
                                            count, ctx->stream));
        }
        PMX_HIP(hipMemcpyAsync(digests.data(), d1, n_rows * 32, hipMemcpyDeviceToHost, ctx->stream));
        PMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    merkle_update_apply(plan, new_leaves, digests.data(), nodes);
    if (root) std::memcpy(root, nodes + (s.n_nodes - 1) * 4, 32);
    return PMX_OK;
    PMX_ABI_END
}

// ---- trees over any number of leaves ----------------------------------------------------------------------------------------------
extern "C" int pmx_merkle_ragged_shape(size_t n_leaves, uint32_t arity, size_t *depth, size_t *n_nodes) {
    if (!depth || !n_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_shape: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    *depth = s.depth, *n_nodes = s.n_nodes;
    return PMX_OK;
}

extern "C" int pmx_merkle_ragged_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, void *stream) {
    if (!ctx || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    return build_dev(ctx, d_nodes, n_leaves, arity, 1, stream);
}

extern "C" int pmx_merkle_ragged(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, uint64_t *nodes, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_ragged")
    if (!ctx || !leaves) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    if (int rc = arity_fits(ctx, arity)) return rc;
    return build_host(ctx, leaves, 1, n_leaves, s.n_nodes, arity, nodes, root);
    PMX_ABI_END
}

extern "C" int pmx_merkle_ragged_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, size_t k,
                                       uint64_t *paths_out) {
    if ((!nodes || !indices || !paths_out) && k) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_paths: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    return paths_host(nodes, n_leaves, arity, s.depth, indices, k, paths_out);
}

extern "C" int pmx_merkle_ragged_paths_dev(pmx_ctx *ctx, const uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                           size_t k, uint64_t *d_paths, void *stream) {
    if (!ctx || ((!d_nodes || !d_indices || !d_paths) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_paths_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    return paths_dev(ctx, d_nodes, n_leaves, arity, s.depth, true, d_indices, k, d_paths, stream);
}

extern "C" int pmx_merkle_ragged_verify_paths_dev(pmx_ctx *ctx, const uint64_t *d_leaves, const uint64_t *d_indices, const uint64_t *d_paths,
                                                  size_t depth, uint32_t arity, size_t n_leaves, size_t k, const uint64_t *d_root,
                                                  uint8_t *d_ok, uint64_t *d_work, void *stream) {
    if (!ctx || ((!d_leaves || !d_indices || !d_ok || !d_work) && k) || (!d_paths && k && depth) || !d_root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_verify_paths_dev: null pointer");
    if (int rc = ragged_verify_shape(depth, arity, n_leaves)) return rc;
    return verify_dev(ctx, d_leaves, d_indices, d_paths, depth, arity, (uint64_t)n_leaves, false, k, d_root, d_ok, d_work, stream);
}

extern "C" int pmx_merkle_ragged_verify_paths(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *indices, const uint64_t *paths, size_t depth,
                                              uint32_t arity, size_t n_leaves, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out) {
    PMX_ABI_BEGIN("pmx_merkle_ragged_verify_paths")
    if (!ctx || ((!leaves || !indices || !ok_out) && k) || (!paths && k && depth) || !root)
        return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_verify_paths: null pointer");
    if (int rc = ragged_verify_shape(depth, arity, n_leaves)) return rc;
    return verify_host(ctx, leaves, nullptr, 0, indices, paths, depth, arity, (uint64_t)n_leaves, false, k, root, ok_out);
    PMX_ABI_END
}

extern "C" int pmx_merkle_ragged_update_dev(pmx_ctx *ctx, uint64_t *d_nodes, size_t n_leaves, uint32_t arity, const uint64_t *d_indices,
                                            const uint64_t *d_new_leaves, size_t k, uint64_t *d_work, void *stream) {
    if (!ctx || ((!d_nodes || !d_indices || !d_new_leaves || !d_work) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_ragged_update_dev: null pointer");
    MerkleShape s;
    if (int rc = tree_shape(n_leaves, arity, Family::ragged, &s)) return rc;
    return update_dev(ctx, d_nodes, n_leaves, arity, true, d_indices, d_new_leaves, k, d_work, stream);
}

// ---- trees of a fixed depth: empty positions are default leaves, leaves are appended in place -----------------------------------------
namespace {

int frontier_error(FrontierError e) {
    switch (e) {
    case FrontierError::ok: return PMX_OK;
    case FrontierError::arity: return set_error(PMX_ERR_ARG, "arity must be at least 2");
    case FrontierError::depth: return set_error(PMX_ERR_ARG, "depth must be 1 .. 64");
    case FrontierError::pow_overflow: return set_error(PMX_ERR_ARG, "arity^depth overflows 64 bits");
    case FrontierError::too_many: return set_error(PMX_ERR_ARG, "more leaves than the arity^depth positions of the tree");
    case FrontierError::no_leaves: return set_error(PMX_ERR_ARG, "a tree needs at least one leaf");
    default: return set_error(PMX_ERR_ARG, "tree byte size overflows size_t");
    }
}

// One piece of the walk (pmx_merkle_frontier.hpp), a host-buffer call of its own - its host temporaries are declared in front of its
// scope, so they outlive its drain, and its two blocks grow with the piece: one upload of frontier and default
// digests, one of the two lists, one of the leaves; the kept nodes and the pads of ALL levels in one launch; one full-row compression
// launch per level that has rows, on the engine pmx_ctx_engine_info names for its parents; the new frontier and the root gathered in one
// launch and brought back in one download.  `frontier` ([D][k - 1][4], host) is read in its kept slots and replaced, unused slots zero;
// `root` [4] receives the root when the plan knows it.  nodes / first: the dense form keeps what the piece computed - the fresh and the
// partial node of every level above the leaves go to their places in the caller's array, one download per level.
int fixed_piece(pmx_ctx *ctx, const FrontierPlan &P, const uint64_t *defaults, uint64_t *frontier, const uint64_t *leaves, uint64_t *root,
                uint64_t *nodes, const size_t *first) {
    const size_t D = P.depth, fe = P.frontier_elements(), n_place = P.place.size() / 2, n_gather = P.gather.size() / 2;
    std::vector<uint64_t> in((fe + D + 1) * 4), out((fe + 1) * 4), lists(P.place);
    std::memcpy(in.data(), frontier, fe * 32);
    std::memcpy(in.data() + fe * 4, defaults, (D + 1) * 32);
    lists.insert(lists.end(), P.gather.begin(), P.gather.end());
    PMX_HOST_CALL(call, ctx);
    Staging rows, pairs;
    rows.add(P.elements, 32);           // frontier and defaults in | frontier and root out | the rows of the levels (FrontierPlan)
    pairs.add(lists.size() + 2, 8);     // the place list | the gather list
    char *d0 = nullptr, *d1 = nullptr;
    int rc = PMX_OK;
    if ((rc = call.stage(rows, &d0)) || (rc = call.stage(pairs, &d1))) return rc;
    uint64_t *d = (uint64_t *)d0, *d_lists = (uint64_t *)d1;
    PMX_HIP(hipMemcpyAsync(d + P.in_frontier * 4, in.data(), in.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!lists.empty()) PMX_HIP(hipMemcpyAsync(d_lists, lists.data(), lists.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (P.m) PMX_HIP(hipMemcpyAsync(d + (P.level[0].offset + P.level[0].kept) * 4, leaves, (size_t)P.m * 32, hipMemcpyHostToDevice, ctx->stream));
    if (n_place) PMX_HIP(launch_node_place(d, d_lists, n_place, ctx->stream));
    for (size_t l = 0; l < D; ++l) {
        const FrontierLevel &L = P.level[l], &U = P.level[l + 1];
        if (L.parents)
            PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, d + L.offset * 4, d + (U.offset + U.kept) * 4, P.arity, (size_t)L.parents, ctx->stream));
    }
    if (n_gather) PMX_HIP(launch_node_place(d, d_lists + n_place * 2, n_gather, ctx->stream));
    PMX_HIP(hipMemcpyAsync(out.data(), d + P.out_frontier * 4, out.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (nodes)
        for (size_t l = 1; l <= D; ++l) {
            const FrontierLevel &L = P.level[l];
            if (const size_t count = (size_t)(L.fresh + L.partial))
                PMX_HIP(hipMemcpyAsync(nodes + (first[l] + (size_t)(L.first + L.kept)) * 4, d + (L.offset + L.kept) * 4, count * 32,
                                       hipMemcpyDeviceToHost, ctx->stream));
        }
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    if (nodes && P.m) std::memcpy(nodes + (size_t)P.n * 4, leaves, (size_t)P.m * 32);
    std::memset(frontier, 0, fe * 32);
    for (size_t l = 0; l < D; ++l)
        std::memcpy(frontier + l * (P.arity - 1) * 4, out.data() + l * (P.arity - 1) * 4, (size_t)P.level[l].digit * 32);
    if (P.root_computed) std::memcpy(root, out.data() + fe * 4, 32);
    else if (P.root_is_default) std::memcpy(root, defaults + D * 4, 32);
    return PMX_OK;
}

// m leaves behind the n the frontier stands for, in pieces of merkle_fixed_piece() leaves (appends compose exactly: pieces change no byte);
// m = 0 is one piece that recomputes the partial nodes and the root.  frontier / root: host temporaries, as for fixed_piece.
int fixed_walk(pmx_ctx *ctx, uint32_t arity, size_t depth, const uint64_t *defaults, uint64_t n, const uint64_t *leaves, uint64_t m,
               uint64_t *frontier, uint64_t *root, uint64_t *nodes, const size_t *first) {
    const uint64_t piece = merkle_fixed_piece();
    uint64_t done = 0;
    do {
        const uint64_t take = m - done < piece ? m - done : piece;
        FrontierPlan plan;
        if (int rc = frontier_error(frontier_plan(n + done, take, arity, depth, &plan))) return rc;
        if (int rc = fixed_piece(ctx, plan, defaults, frontier, leaves + (size_t)done * 4, root, nodes, first)) return rc;
        done += take;
    } while (done < m);
    return PMX_OK;
}

}  // namespace

extern "C" int pmx_merkle_fixed_defaults(pmx_ctx *ctx, const uint64_t default_leaf[PMX_LIMBS], uint32_t arity, size_t depth, uint64_t *defaults_out) {
    PMX_ABI_BEGIN("pmx_merkle_fixed_defaults")
    if (!ctx || !default_leaf || !defaults_out) return set_error(PMX_ERR_ARG, "pmx_merkle_fixed_defaults: null pointer");
    u128 capacity = 0;
    if (int rc = frontier_error(frontier_capacity(arity, depth, &capacity))) return rc;
    if (int rc = arity_fits(ctx, arity)) return rc;
    std::vector<uint64_t> list, e((depth + 1) * 4);     // (in front of the scope: copied from and into until its drain)
    for (size_t l = 0; l < depth; ++l)
        for (uint32_t j = 0; j < arity; ++j) list.push_back(depth + 1 + l * arity + j), list.push_back(l);
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    Staging digests, copies;
    digests.add(depth + 1, 32);                  // e [depth + 1][4]
    digests.add(depth, (size_t)arity * 32);      // rows [depth][arity][4], element depth + 1 on
    copies.add(list.size(), 8);                  // the list that copies e[l] into the arity slots of row l
    char *d0 = nullptr, *d1 = nullptr;
    if ((rc = call.stage(digests, &d0)) || (rc = call.stage(copies, &d1))) return rc;
    uint64_t *d = (uint64_t *)d0, *d_list = (uint64_t *)d1;
    PMX_HIP(hipMemcpyAsync(d, default_leaf, 32, hipMemcpyHostToDevice, ctx->stream));
    PMX_HIP(hipMemcpyAsync(d_list, list.data(), list.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    for (size_t l = 0; l < depth; ++l) {      // e[l + 1] depends on e[l]: `depth` launches of one unit each
        PMX_HIP(launch_node_place(d, d_list + l * arity * 2, arity, ctx->stream));
        PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, d + (depth + 1 + l * arity) * 4, d + (l + 1) * 4, arity, 1, ctx->stream));
    }
    PMX_HIP(hipMemcpyAsync(e.data(), d, e.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(defaults_out, e.data(), e.size() * 8);
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_merkle_frontier_append(pmx_ctx *ctx, uint32_t arity, size_t depth, const uint64_t *defaults, const uint64_t *frontier_in,
                                          size_t n_leaves, const uint64_t *new_leaves, size_t m, uint64_t *frontier_out, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_frontier_append")
    if (!ctx || !defaults || !frontier_out || (!frontier_in && n_leaves) || (!new_leaves && m))
        return set_error(PMX_ERR_ARG, "pmx_merkle_frontier_append: null pointer");
    u128 capacity = 0;
    if (int rc = frontier_error(frontier_capacity(arity, depth, &capacity))) return rc;
    if ((u128)n_leaves + m > capacity || (u128)n_leaves + m > UINT64_MAX) return frontier_error(FrontierError::too_many);
    if (m > (SIZE_MAX / 32) / 4) return frontier_error(FrontierError::bytes_overflow);
    if (root && m == 0 && (u128)n_leaves == capacity)
        return set_error(PMX_ERR_ARG, "the frontier of a full tree holds no node: its root cannot be recomputed (root must be NULL)");
    if (int rc = arity_fits(ctx, arity)) return rc;
    std::vector<uint64_t> frontier(depth * (size_t)(arity - 1) * 4, 0);
    uint64_t top[4] = {0, 0, 0, 0};
    if (frontier_in) std::memcpy(frontier.data(), frontier_in, frontier.size() * 8);
    if (int rc = fixed_walk(ctx, arity, depth, defaults, n_leaves, new_leaves, m, frontier.data(), top, nullptr, nullptr)) return rc;
    std::memcpy(frontier_out, frontier.data(), frontier.size() * 8);
    if (root) std::memcpy(root, top, 32);
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_merkle_fixed_shape(size_t n_leaves, uint32_t arity, size_t depth, size_t *n_nodes) {
    PMX_ABI_BEGIN("pmx_merkle_fixed_shape")
    if (!n_nodes) return set_error(PMX_ERR_ARG, "pmx_merkle_fixed_shape: null pointer");
    std::vector<size_t> first;
    if (int rc = frontier_error(fixed_shape(n_leaves, arity, depth, &first))) return rc;
    *n_nodes = first[depth + 1];
    return PMX_OK;
    PMX_ABI_END
}

// The dense form: the walk from the empty frontier, every computed node kept.  `nodes` is written piece by piece.
extern "C" int pmx_merkle_fixed(pmx_ctx *ctx, const uint64_t *leaves, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *defaults,
                                uint64_t *nodes, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_fixed")
    if (!ctx || !leaves || !defaults) return set_error(PMX_ERR_ARG, "pmx_merkle_fixed: null pointer");
    std::vector<size_t> first;
    if (int rc = frontier_error(fixed_shape(n_leaves, arity, depth, &first))) return rc;
    if (int rc = arity_fits(ctx, arity)) return rc;
    std::vector<uint64_t> frontier(depth * (size_t)(arity - 1) * 4, 0);
    uint64_t top[4] = {0, 0, 0, 0};
    if (int rc = fixed_walk(ctx, arity, depth, defaults, 0, leaves, n_leaves, frontier.data(), top, nodes, first.data())) return rc;
    if (root) std::memcpy(root, top, 32);
    return PMX_OK;
    PMX_ABI_END
}

// Openings of the dense form, on the host: the layout of pmx_merkle_ary_paths; a sibling at or beyond its level's stored width is an
// empty subtree, e[level].  Every index is checked before anything is written.
extern "C" int pmx_merkle_fixed_paths(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *defaults,
                                      const uint64_t *indices, size_t k_paths, uint64_t *paths_out) {
    PMX_ABI_BEGIN("pmx_merkle_fixed_paths")
    if (!nodes || !defaults || ((!indices || !paths_out) && k_paths)) return set_error(PMX_ERR_ARG, "pmx_merkle_fixed_paths: null pointer");
    std::vector<size_t> first;
    if (int rc = frontier_error(fixed_shape(n_leaves, arity, depth, &first))) return rc;
    if (k_paths > (SIZE_MAX / 32) / (depth * (size_t)(arity - 1))) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    for (size_t i = 0; i < k_paths; ++i)
        if (indices[i] >= n_leaves) return set_error(PMX_ERR_ARG, "leaf index %llu out of range", (unsigned long long)indices[i]);
    const size_t sib = arity - 1;
    for (size_t i = 0; i < k_paths; ++i) {
        size_t idx = (size_t)indices[i];
        for (size_t level = 0; level < depth; ++level, idx /= arity) {
            const size_t digit = idx % arity, base = idx - digit, width = first[level + 1] - first[level];
            uint64_t *row = paths_out + (i * depth + level) * sib * 4;
            for (size_t s = 0; s < sib; ++s) {
                const size_t child = base + (s < digit ? s : s + 1);
                std::memcpy(row + s * 4, child < width ? nodes + (first[level] + child) * 4 : defaults + level * 4, 32);
            }
        }
    }
    return PMX_OK;
    PMX_ABI_END
}

// ---- sequential leaf updates of a fixed-depth tree, with witnesses ---------------------------------------------------------------------
// k updates walked level by level (pmx_merkle_chain.hpp): V_0 = new_leaves; per level the planner says which earlier update every sibling
// comes from, one gather launch builds the k rows (and the level's slab of the witnesses) out of V_l and the level's slab of the old
// openings, one compression launch of k rows gives V_{l+1}; V_depth is the roots.  Device memory is one block of O(k * arity) elements
// whatever the depth: V twice, the rows, the indices, and two each of path slab, pred slab and witness slab.  A level's slab goes up and
// comes down as ONE 2-D copy, (arity - 1) * 32 bytes wide and k high, with the pitch of a whole opening on the host side.
// Streams: `stream` copies, `stream2` computes.  The slab of level l + 1 goes up behind the gather of level l - 1 (which read its buffer),
// so it travels while level l compresses; the witness slab of level l comes down on `stream` behind its gather, in front of the next
// upload - the gather of level l + 2, which writes that buffer again, waits for an upload recorded behind it.  The host plans a
// level right before it enqueues it, so the plan of level l + 1 can run under the device's level l - as far as the runtime lets it: pred
// is pageable host memory, [depth][k][arity - 1] for the whole call (only the DEVICE side is O(k * arity) whatever the depth), and a
// pageable upload may hold the host until the copy stream reaches it.
extern "C" int pmx_merkle_update_witnesses(pmx_ctx *ctx, uint32_t arity, size_t depth, const uint64_t *indices, const uint64_t *new_leaves,
                                           const uint64_t *paths, size_t k, uint64_t *witness_out, uint64_t *roots_out, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_merkle_update_witnesses")
    if (!ctx || ((!indices || !new_leaves || !paths) && k)) return set_error(PMX_ERR_ARG, "pmx_merkle_update_witnesses: null pointer");
    u128 capacity = 0;
    if (int rc = frontier_error(frontier_capacity(arity, depth, &capacity))) return rc;
    if (k == 0) {
        if (root) return set_error(PMX_ERR_ARG, "no update leaves no root to return: root must be NULL when k = 0");
        return PMX_OK;
    }
    if (k > kChainMaxUpdates) return set_error(PMX_ERR_ARG, "batch too large: at most %zu updates in one call", kChainMaxUpdates);
    const size_t sib = arity - 1;
    Staging opening, block;
    opening.add(opening.times(opening.times(k, depth), sib), 32);        // paths / witness_out [k][depth][arity - 1][4] (host)
    const size_t o_v = block.add(block.times(k, 2), 32);                 // V [2][k][4]: the running nodes of a level and of the next
    const size_t o_rows = block.add(k, (size_t)arity * 32);              // rows [k][arity][4]
    const size_t o_idx = block.add(k, 8);                                // indices [k]
    const size_t o_slab = block.add(block.times(k, 2), sib * 32);        // [2] path slabs [k][arity - 1][4]
    const size_t o_pred = block.add(block.times(k, 2), sib * 4);         // [2] pred slabs [k][arity - 1]
    const size_t o_wit = block.add(block.times(witness_out ? k : 0, 2), sib * 32);   // [2] witness slabs [k][arity - 1][4]
    if (opening.overflowed() || block.overflowed()) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    const bool all = capacity > (u128)UINT64_MAX;
    const size_t bad = chain_first_bad(indices, k, (uint64_t)capacity, all);     // (before anything is launched or written)
    if (bad < k) return set_error(PMX_ERR_ARG, "leaf index %llu out of range", (unsigned long long)indices[bad]);
    if (int rc = arity_fits(ctx, arity)) return rc;
    ChainPlanner planner(indices, k, arity);
    std::vector<uint32_t> pred(depth * k * sib);     // (in front of the scope: copied from until its drain)
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    char *d = nullptr;
    if ((rc = call.stage(block, &d))) return rc;
    (void)call.pin(paths, opening.bytes(), false);
    if (witness_out) (void)call.pin(witness_out, opening.bytes(), false);
    uint64_t *d_v[2] = {(uint64_t *)(d + o_v), (uint64_t *)(d + o_v) + k * 4}, *d_rows = (uint64_t *)(d + o_rows), *d_idx = (uint64_t *)(d + o_idx);
    const size_t slab_bytes = k * sib * 32, width = sib * 32, pitch = depth * width;
    hipStream_t copy = ctx->stream, run = ctx->stream2;
    PMX_HIP(hipMemcpyAsync(d_v[0], new_leaves, k * 32, hipMemcpyHostToDevice, copy));
    PMX_HIP(hipMemcpyAsync(d_idx, indices, k * 8, hipMemcpyHostToDevice, copy));
    uint64_t pow = 1;     // arity^l (l < depth: below arity^depth <= 2^64)
    for (size_t l = 0; l < depth; ++l) {
        const int slot = (int)(l % pmx_ctx::kPipeChunks);
        uint32_t *h_pred = pred.data() + l * k * sib;
        planner.next_level(h_pred);
        uint64_t *d_slab = (uint64_t *)(d + o_slab + (l & 1) * slab_bytes), *d_wit = witness_out ? (uint64_t *)(d + o_wit + (l & 1) * slab_bytes) : nullptr;
        uint32_t *d_pred = (uint32_t *)(d + o_pred + (l & 1) * (k * sib * 4));
        // (the gather of level l - 2 read these buffers: its event is two slots back, recorded before this point)
        if (l >= 2) PMX_HIP(hipStreamWaitEvent(copy, ctx->pipe_done[(l - 2) % pmx_ctx::kPipeChunks], 0));
        PMX_HIP(hipMemcpy2DAsync(d_slab, width, (const char *)paths + l * width, pitch, width, k, hipMemcpyHostToDevice, copy));
        PMX_HIP(hipMemcpyAsync(d_pred, h_pred, k * sib * 4, hipMemcpyHostToDevice, copy));
        PMX_HIP(hipEventRecord(ctx->pipe_up[slot], copy));
        PMX_HIP(hipStreamWaitEvent(run, ctx->pipe_up[slot], 0));
        PMX_HIP(launch_chain_rows(d_v[l & 1], d_slab, d_pred, d_idx, pow, arity, d_rows, d_wit, k, run));
        PMX_HIP(hipEventRecord(ctx->pipe_done[slot], run));
        PMX_HIP(launch_compress_ary(ctx->dev, ctx->t, d_rows, d_v[(l + 1) & 1], arity, k, run));
        if (witness_out) {
            PMX_HIP(hipStreamWaitEvent(copy, ctx->pipe_done[slot], 0));
            PMX_HIP(hipMemcpy2DAsync((char *)witness_out + l * width, pitch, d_wit, width, width, k, hipMemcpyDeviceToHost, copy));
        }
        if (l + 1 < depth) pow *= arity;
    }
    const uint64_t *d_roots = d_v[depth & 1];
    if (roots_out) PMX_HIP(hipMemcpyAsync(roots_out, d_roots, k * 32, hipMemcpyDeviceToHost, run));
    if (root) PMX_HIP(hipMemcpyAsync(root, d_roots + (k - 1) * 4, 32, hipMemcpyDeviceToHost, run));
    PMX_HIP(hipStreamSynchronize(run));
    PMX_HIP(hipStreamSynchronize(copy));
    return PMX_OK;
    PMX_ABI_END
}
