// Launcher entry points of pmx_device.hip, pmx_convert.hip and pmx_tree_moves.hip (host-callable; they only enqueue on `st`).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/poseidon_mi355x.h"
#include "pmx_internal.hpp"

namespace pmx {

using EngineInfo = ::pmx_engine_info;
// pmx_ctx_engine_info: the engine `op` over n units would be launched on, decided by the launchers' own conditions
hipError_t describe_launch(const DevConfig &c, uint32_t t, int op, size_t n, size_t len, EngineInfo *o);

hipError_t launch_permute(const DevConfig &c, uint32_t t, uint64_t *states, size_t n, hipStream_t st);
hipError_t launch_hash(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len,
                       size_t n, hipStream_t st);
// the same rows addressed through two strides in elements (pmx_matrix_*, pmx_matrix_shape.hpp): element k of row i at
// in + (i * row_stride + k * elem_stride) * 4; out [n][out_len][4] packed as above.  Nothing but those n * in_len elements is read.
hipError_t launch_hash_strided(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, size_t row_stride, size_t elem_stride,
                               uint64_t *out, size_t out_len, size_t n, hipStream_t st);
// out[i] = 2-to-1 compression of in[2i], in[2i+1]   (rate >= 2)
hipError_t launch_compress(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, size_t n, hipStream_t st);
// out[i] = arity-to-1 compression of in[arity i .. arity i + arity)   (2 <= arity <= rate; arity 2 is launch_compress)
hipError_t launch_compress_ary(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n, hipStream_t st);
// one tree level of n_children nodes, any number >= 1 (pmx_merkle_ragged*): out[p] = the compression of in[arity p .. min(arity (p + 1),
// n_children)) for the ceil(n_children / arity) parents, in one launch; nothing at or beyond in[n_children] is read.  A level that divides
// by the arity is launch_compress_ary.
hipError_t launch_compress_level(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n_children,
                                 hipStream_t st);
// one chunk of a proof-of-work search (pmx_sponge_grind): the nonces first .. first + n - 1 tried against the one base state at `base`
// ([t][4], device) with the nonce absorbed at state[capacity + index], index < rate; best[0] (device, UINT64_MAX before the first chunk)
// is lowered to the smallest nonce whose digest has `bits` low zero bits and best[1] (0 before) is set to 1 with it.  No per-candidate memory.
hipError_t launch_grind(const DevConfig &c, uint32_t t, const uint64_t *base, uint32_t index, uint32_t bits, uint64_t first, size_t n,
                        uint64_t *best, hipStream_t st);
// Device scratch for the pass lists of the drivers that run as passes (pmx_engine_launch.hpp: sponge_passes): `get` hands out at least
// `bytes` bytes that stay valid for everything enqueued on `st` by this call, `done` is called once behind the call's last launch
// (pmx_sponge.cpp: a pool of blocks owned by the context, each released by an event recorded there).  Engines that need no lists
// call neither.
struct PassScratch {
    void *owner = nullptr;
    hipError_t (*get)(void *owner, hipStream_t st, size_t bytes, uint32_t **out) = nullptr;
    void (*done)(void *owner, hipStream_t st, uint32_t *block) = nullptr;
};
// One block of a PassScratch for the length of a scope: `take` is the `get`, and the scope's end - whichever way out, behind everything
// the scope enqueued on `st` - is the `done` of a block that was taken.  A block that is not given back is never handed out again.
class PassLease {
public:
    PassLease(const PassScratch &from, hipStream_t st) : from_(from), st_(st) {}
    ~PassLease() {
        if (block && err == hipSuccess && from_.done) from_.done(from_.owner, st_, block);
    }
    PassLease(const PassLease &) = delete;
    PassLease &operator=(const PassLease &) = delete;
    hipError_t take(size_t bytes) { return err = from_.get(from_.owner, st_, bytes, &block); }

    uint32_t *block = nullptr;      // what `take` got; null before it and after one that failed
    hipError_t err = hipSuccess;    // of the take

private:
    const PassScratch &from_;
    hipStream_t st_;
};
hipError_t launch_absorb(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                         const uint64_t *in, size_t in_len, size_t n, hipStream_t st, const PassScratch &scratch);
hipError_t launch_squeeze(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                          uint64_t *out, size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch);
// Variable-length rows (pmx_sponge_plan.hpp: varlen_row_len): row i is in[offsets[i] .. offsets[i + 1]) clamped to max_len elements,
// offsets [n + 1] device-resident.  absorb: an empty row leaves its sponge untouched (mod.rs:234-236).  hash: per row new; absorb(row);
// squeeze_native(out_len) into out [n][out_len][4]; the n fresh states are a block of `scratch` (get / done once, around the call).
hipError_t launch_absorb_varlen(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                                const uint64_t *offsets, size_t max_len, size_t n, hipStream_t st, const PassScratch &scratch);
hipError_t launch_hash_varlen(const DevConfig &c, uint32_t t, const uint64_t *in, const uint64_t *offsets, size_t max_len, uint64_t *out,
                              size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch);

// squeeze_bytes (bits = false) / squeeze_bits (mod.rs:256-286) of n sponges into out [n][len], one byte per output unit (pmx_convert.hip):
// launch_squeeze of ceil(len / unit) native elements into a block of `scratch`, then the conversion kernel from it into `out`; states and
// mode words end as after that native squeeze.  `out` needs no alignment.  Scratch is bounded by kCutScratchBytes: a larger call runs in
// slices over sponges through one block.
constexpr size_t kCutScratchBytes = PMX_SQUEEZE_SCRATCH_BYTES;
hipError_t launch_squeeze_cut(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, uint8_t *out, size_t len,
                              bool bits, size_t n, hipStream_t st, const PassScratch &scratch);

// What ONE engine instantiation serves (pmx_engine_launch.hpp: engine_ops<Engine>() fills it; pmx_device.hip: select_engine picks the table of a call): every
// member has the signature of its launch_* above whatever the engine - one that runs absorb / squeeze as per-lane kernels does not touch
// the PassScratch, one that runs them as passes takes its lists from it.  Both the launchers and describe_launch go through the table
// select_engine returns, so what pmx_ctx_engine_info reports is what a launch runs.
// Adding an operation: its kernel, a member here, a one-line Launch<Engine> method that hands the kernel and its arguments to
// Launch<Engine>::enqueue (the one launch body: LDS attribute, geometry, error), its line in engine_ops, a launch_* one-liner.
struct EngineOps {
    hipError_t (*permute)(const DevConfig &c, uint32_t t, uint64_t *states, size_t n, hipStream_t st);
    hipError_t (*hash)(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len, size_t n,
                       hipStream_t st);
    hipError_t (*hash_strided)(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, size_t row_stride, size_t elem_stride,
                               uint64_t *out, size_t out_len, size_t n, hipStream_t st);
    hipError_t (*compress)(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, size_t n, hipStream_t st);
    hipError_t (*compress_ary)(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n, hipStream_t st);
    // (the level with a short last row: n = ceil(n_children / arity) parents, children bounded by n_children)
    hipError_t (*compress_ary_bounded)(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n_children,
                                       size_t n, hipStream_t st);
    hipError_t (*grind)(const DevConfig &c, uint32_t t, const uint64_t *base, uint32_t index, uint32_t bits, uint64_t first, size_t n,
                        uint64_t *best, hipStream_t st);
    hipError_t (*absorb)(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                         size_t in_len, size_t n, hipStream_t st, const PassScratch &scratch);
    hipError_t (*absorb_varlen)(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                                const uint64_t *offsets, size_t max_len, size_t n, hipStream_t st, const PassScratch &scratch);
    hipError_t (*squeeze)(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, uint64_t *out,
                          size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch);
    size_t (*lds_bytes)(const DevConfig &c, uint32_t t);   // dynamic LDS one workgroup asks for
    // fills EngineInfo for `op` (PMX_OP_*) at `len` elements per sponge: the engine's own fields, then waves, LDS and launches of the op
    void (*describe)(const DevConfig &c, uint32_t t, int op, size_t len, EngineInfo *o);
};

// Authentication paths, one level per step (pmx_merkle_verify_paths_dev): pairs[i] = (cur[i], sibling) or (sibling, cur[i])
// by bit `level` of indices[i], sibling = paths[i][level]; then ok[i] = (cur[i] == root) && indices[i] < limit (2^depth).
hipError_t launch_path_pairs(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level,
                             uint64_t *pairs, size_t k, hipStream_t st);
hipError_t launch_path_check(const uint64_t *cur, const uint64_t *root, const uint64_t *indices, uint64_t limit, uint8_t *ok,
                             size_t k, hipStream_t st);
// The same for any arity (pmx_merkle_ary_verify_paths_dev; paths [k][depth][arity - 1][4]): rows[i] = the arity children of path i's
// parent at `level`, cur[i] at digit (indices[i] / pow) % arity with pow = arity^level; the check above with limit = arity^depth.
hipError_t launch_path_children(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level, uint64_t pow,
                                uint32_t arity, uint64_t *rows, size_t k, hipStream_t st);
// The opening on the device (pmx_merkle_ary_paths_dev): paths[i] = the siblings of leaf indices[i] and of its ancestors out of `nodes`
// (zeros for an index >= n_leaves).  depth >= 1, k >= 1.
hipError_t launch_paths_gather(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices, uint64_t *paths,
                               size_t k, hipStream_t st);
// Leaf updates (pmx_merkle_ary_update*): dst[base + indices[i] / pow] = src[i] for indices[i] < limit (elements of 4 words; pow >= 1), and
// rows[i] = the arity children nodes[first + p * arity ...] of parent p = indices[i] / pow (p = 0 for an index >= n_leaves).  k >= 1.
hipError_t launch_node_scatter(const uint64_t *src, const uint64_t *indices, uint64_t pow, uint64_t limit, uint64_t base, uint64_t *dst,
                               size_t k, hipStream_t st);
hipError_t launch_node_children(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first, uint32_t arity,
                                uint64_t *rows, size_t k, hipStream_t st);
// Trees over any number of leaves (pmx_merkle_ragged*): the two gathers with the level's width carried along - a child at or beyond it is
// four zero words, and nothing at or beyond the level's end is read.  `width`: the nodes of the level whose first node is `first`.
hipError_t launch_paths_gather_ragged(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices,
                                      uint64_t *paths, size_t k, hipStream_t st);
hipError_t launch_node_children_bounded(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first,
                                        uint64_t width, uint32_t arity, uint64_t *rows, size_t k, hipStream_t st);
// Opened rows of a matrix on the device (pmx_matrix_open_dev): rows[i][j] = element (indices[i], j) of the strided view - the 4 words at
// matrix + (indices[i] * row_stride + j * elem_stride) * 4 - for j < row_len, rows [k][row_len][4] with each row contiguous; an all-zero
// row for an index >= n_rows, and nothing outside the view is read.  k * row_len <= kMaxLaunchUnits, k >= 1.
hipError_t launch_matrix_rows(const uint64_t *matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                              const uint64_t *indices, uint64_t *rows, size_t k, hipStream_t st);
// Fixed-depth trees (pmx_merkle_fixed*, pmx_merkle_frontier_append): elems[list[2 i]] = elems[list[2 i + 1]] for i < k, elements of 4 words
// of one device array, the pairs built by the host (pmx_merkle_frontier.hpp); no destination is a source of the same launch.  k >= 1.
hipError_t launch_node_place(uint64_t *elems, const uint64_t *list, size_t k, hipStream_t st);
// Sequential leaf updates (pmx_merkle_update_witnesses), one level: rows[j] = the arity children of update j's parent, cur[j] at digit
// (indices[j] / pow) % arity and in sibling slot s cur[pred[j][s]] if pred[j][s] < j, else slab[j][s] (slab, wit: [k][arity - 1][4]; pred:
// [k][arity - 1], pmx_merkle_chain.hpp); the siblings also go to wit[j][s] unless wit is null.  pow = arity^level >= 1, k >= 1.
hipError_t launch_chain_rows(const uint64_t *cur, const uint64_t *slab, const uint32_t *pred, const uint64_t *indices, uint64_t pow,
                             uint32_t arity, uint64_t *rows, uint64_t *wit, size_t k, hipStream_t st);

}  // namespace pmx
