// The data movement of the Merkle entries (pmx_merkle.cpp) around the compression launches: authentication paths, node scatter / gather,
// the placement lists of the fixed-depth trees, the chained rows of their sequential leaf updates - and the opened rows of a matrix
// on the device (pmx_matrix.cpp).  The kernels move 16-byte pieces of
// ABI elements and know nothing of a field or an engine, so - like pmx_convert.hip - this translation unit is compiled once.
// Declarations: pmx_launch.hpp.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pmx_launch.hpp"

namespace pmx {

// ---- authentication paths (pmx_merkle_verify_paths_dev) --------------------------------------------------------------
// Pure data movement: four lanes per path, one 16-byte quarter of the 64-byte pair each.
__global__ void __launch_bounds__(256) path_pairs_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ paths,
                                                         const uint64_t *__restrict__ indices, size_t depth, size_t level,
                                                         uint4 *__restrict__ pairs, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 2;
    if (i >= k) return;
    const uint32_t quarter = gid & 3, half = quarter & 1;
    const bool right = (indices[i] >> level) & 1;          // the running node is the right child at this level
    const bool from_cur = (quarter >> 1) == (right ? 1u : 0u);
    pairs[gid] = from_cur ? cur[i * 2 + half] : paths[(i * depth + level) * 2 + half];
}

// the same for a tree of any arity (pmx_merkle_ary_verify_paths_dev): 2 arity lanes per path, one 16-byte quarter of a child each.
// Row i of `rows` is the arity children of path i's parent at `level`: the running node at digit (index / arity^level) % arity, the
// arity - 1 siblings of paths[i][level] in child order around it.  pow = arity^level (the caller's; >= 1).  The digit is below the
// arity whatever the index holds, so an index that names no leaf still reads inside the arrays.
__global__ void __launch_bounds__(256) path_children_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ paths,
                                                            const uint64_t *__restrict__ indices, size_t depth, size_t level, uint64_t pow,
                                                            uint32_t arity, uint4 *__restrict__ rows, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint32_t quarter = (uint32_t)(gid - i * per), child = quarter >> 1, half = quarter & 1;
    const uint32_t digit = (uint32_t)((indices[i] / pow) % arity);
    const uint32_t sibling = child < digit ? child : child - 1;   // the running node's own slot is left out of the path
    rows[gid] = child == digit ? cur[i * 2 + half] : paths[((i * depth + level) * (arity - 1) + sibling) * 2 + half];
}

// The opening itself on the device (pmx_merkle_ary_paths_dev): from the node array (leaves, then every level, root last) to paths
// [k][depth][arity - 1][4], one 16-byte quarter per lane.  Device-resident indices are not validated by the host: an index that names
// no leaf gets an all-zero path, and nothing outside the node array is read.
__global__ void __launch_bounds__(256) paths_gather_kernel(const uint4 *__restrict__ nodes, uint64_t n_leaves, uint32_t arity, size_t depth,
                                                           const uint64_t *__restrict__ indices, uint4 *__restrict__ paths, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per_level = 2 * (size_t)(arity - 1), per = depth * per_level, i = gid / per;
    if (i >= k) return;
    const size_t rest = gid - i * per, level = rest / per_level;
    const uint32_t quarter = (uint32_t)(rest - level * per_level), sibling = quarter >> 1, half = quarter & 1;
    uint64_t idx = indices[i], first = 0, width = n_leaves;   // the running node's index in its level, the level's first node, its width
    if (idx >= n_leaves) {
        paths[gid] = make_uint4(0, 0, 0, 0);
        return;
    }
    for (size_t l = 0; l < level; ++l) {
        first += width;
        width /= arity;
        idx /= arity;
    }
    const uint32_t digit = (uint32_t)(idx % arity);
    const uint32_t child = sibling < digit ? sibling : sibling + 1;
    paths[gid] = nodes[(first + (idx - digit) + child) * 2 + half];
}

// ok[i] = the running node equals the root and indices[i] < limit, the number of leaves a tree of this depth has (2^depth, arity^depth)
__global__ void __launch_bounds__(256) path_check_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ root,
                                                         const uint64_t *__restrict__ indices, uint64_t limit,
                                                         uint8_t *__restrict__ ok, size_t k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const uint4 a = cur[i * 2], b = cur[i * 2 + 1], ra = root[0], rb = root[1];
    const bool same = a.x == ra.x && a.y == ra.y && a.z == ra.z && a.w == ra.w && b.x == rb.x && b.y == rb.y && b.z == rb.z && b.w == rb.w;
    ok[i] = (same && indices[i] < limit) ? 1 : 0;
}

// ---- leaf updates of a resident tree (pmx_merkle_ary_update_dev, pmx_merkle_ary_update) -------------------------------------------
// Pure data movement around launch_compress_ary, like the path kernels above.  The scatter: two lanes per element, one 16-byte half each,
// dst[base + indices[i] / pow] = src[i] if indices[i] < limit.  The leaves go in with pow = 1, base = 0; the parents of level l + 1 with
// pow = arity^(l+1), base = the level's first node (limit = n_leaves both times: index / pow is then below the level's width); the host
// entry's digests go to explicit slots of its packed rows (pow = 1, limit = the slots the level has).  An index at or above the limit
// stores nothing.  Two lanes that store to one element store what their sources hold: equal sources, equal bytes.  pow >= 1.
__global__ void __launch_bounds__(256) node_scatter_kernel(const uint4 *__restrict__ src, const uint64_t *__restrict__ indices, uint64_t pow,
                                                           uint64_t limit, uint64_t base, uint4 *__restrict__ dst, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 1;
    if (i >= k) return;
    const uint64_t idx = indices[i];
    if (idx >= limit) return;
    dst[(base + idx / pow) * 2 + (gid & 1)] = src[gid];
}

// The gather: 2 arity lanes per update, one 16-byte half of a child each.  Row i of `rows` is the arity children of update i's parent
// p = indices[i] / pow (pow = arity^(l+1)) out of level l, whose first node is `first`: nodes[first + p * arity ...].  An index that names no
// leaf (>= n_leaves) gathers the row of parent 0 - in range like every other, and its parent is never stored (the scatter above).
__global__ void __launch_bounds__(256) node_children_kernel(const uint4 *__restrict__ nodes, const uint64_t *__restrict__ indices, uint64_t pow,
                                                            uint64_t n_leaves, uint64_t first, uint32_t arity, uint4 *__restrict__ rows,
                                                            size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint64_t idx = indices[i], p = idx < n_leaves ? idx / pow : 0;
    rows[gid] = nodes[(first + p * arity) * 2 + (gid - i * per)];
}

// ---- trees over any number of leaves (pmx_merkle_ragged*) -------------------------------------------------------------------------------
// Level l + 1 has ceil(M_l / arity) nodes, so a level's width and first row are carried down the levels, not divided out.  Bounded twins of
// paths_gather_kernel and node_children_kernel: a child at or beyond its level's width does not exist - it is four zero words in the
// opening and in the gathered row (the zero a short parent's rate lane holds), and nothing at or beyond the level's end is read.
__global__ void __launch_bounds__(256) paths_gather_ragged_kernel(const uint4 *__restrict__ nodes, uint64_t n_leaves, uint32_t arity, size_t depth,
                                                                  const uint64_t *__restrict__ indices, uint4 *__restrict__ paths, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per_level = 2 * (size_t)(arity - 1), per = depth * per_level, i = gid / per;
    if (i >= k) return;
    const size_t rest = gid - i * per, level = rest / per_level;
    const uint32_t quarter = (uint32_t)(rest - level * per_level), sibling = quarter >> 1, half = quarter & 1;
    uint64_t idx = indices[i], first = 0, width = n_leaves;   // the running node's index in its level, the level's first node, its width
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < n_leaves) {
        for (size_t l = 0; l < level; ++l) {
            first += width;
            width = width / arity + (width % arity ? 1 : 0);
            idx /= arity;
        }
        const uint32_t digit = (uint32_t)(idx % arity);
        const uint64_t child = (idx - digit) + (sibling < digit ? sibling : sibling + 1);   // in its level
        if (child < width) v = nodes[(first + child) * 2 + half];
    }
    paths[gid] = v;
}

// `width`: the nodes level l has (its first node is `first`); parent p = indices[i] / pow has the children p * arity .. below width
__global__ void __launch_bounds__(256) node_children_bounded_kernel(const uint4 *__restrict__ nodes, const uint64_t *__restrict__ indices,
                                                                    uint64_t pow, uint64_t n_leaves, uint64_t first, uint64_t width,
                                                                    uint32_t arity, uint4 *__restrict__ rows, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint32_t quarter = (uint32_t)(gid - i * per), half = quarter & 1;
    const uint64_t idx = indices[i], p = idx < n_leaves ? idx / pow : 0, child = p * arity + (quarter >> 1);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (child < width) v = nodes[(first + child) * 2 + half];
    rows[gid] = v;
}

// ---- opened rows of a matrix on the device (pmx_matrix_open_dev) -------------------------------------------------------------------------
// The row gather: 2 row_len lanes per opened row, one 16-byte half of an element each, consecutive along the row, so the stores into
// rows [k][row_len][4] coalesce; the loads are as far apart as the view's element stride puts them.  Element (i, j) of the view is at
// element index i * row_stride + j * elem_stride (pmx_matrix_shape.hpp: below the view's extent < 2^59 for i < n_rows, j < row_len - the
// 64-bit products do not wrap).  Device-resident indices are not validated by the host: an index that names no row gets an all-zero
// row, and nothing outside the view is read.
__global__ void __launch_bounds__(256) matrix_rows_kernel(const uint4 *__restrict__ matrix, uint64_t n_rows, uint64_t row_len, uint64_t row_stride,
                                                          uint64_t elem_stride, const uint64_t *__restrict__ indices, uint4 *__restrict__ rows,
                                                          size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)row_len, i = gid / per;
    if (i >= k) return;
    const size_t rest = gid - i * per, j = rest >> 1, half = rest & 1;
    const uint64_t idx = indices[i];
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < n_rows) v = matrix[(idx * row_stride + j * elem_stride) * 2 + half];
    rows[gid] = v;
}

// THE launch of a data-movement kernel, whichever: one lane per 16-byte piece it writes (path_check_kernel: per path), 256 lanes a
// workgroup, no LDS.  The elements of the callers' uint64_t arrays reach the kernels as their 16-byte halves (u4).
static const uint4 *u4(const uint64_t *p) { return reinterpret_cast<const uint4 *>(p); }
static uint4 *u4(uint64_t *p) { return reinterpret_cast<uint4 *>(p); }
template <class K, class... A>
static hipError_t plain(K kernel, size_t lanes, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, args...);
    return hipGetLastError();
}

hipError_t launch_paths_gather_ragged(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices,
                                      uint64_t *paths, size_t k, hipStream_t st) {
    return plain(paths_gather_ragged_kernel, k * depth * 2 * (arity - 1), st, u4(nodes), n_leaves, arity, depth, indices, u4(paths), k);
}
hipError_t launch_node_children_bounded(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first,
                                        uint64_t width, uint32_t arity, uint64_t *rows, size_t k, hipStream_t st) {
    return plain(node_children_bounded_kernel, k * 2 * arity, st, u4(nodes), indices, pow, n_leaves, first, width, arity, u4(rows), k);
}

hipError_t launch_matrix_rows(const uint64_t *matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                              const uint64_t *indices, uint64_t *rows, size_t k, hipStream_t st) {
    return plain(matrix_rows_kernel, k * row_len * 2, st, u4(matrix), (uint64_t)n_rows, (uint64_t)row_len, (uint64_t)row_stride,
                 (uint64_t)elem_stride, indices, u4(rows), k);
}

hipError_t launch_node_scatter(const uint64_t *src, const uint64_t *indices, uint64_t pow, uint64_t limit, uint64_t base, uint64_t *dst,
                               size_t k, hipStream_t st) {
    return plain(node_scatter_kernel, k * 2, st, u4(src), indices, pow, limit, base, u4(dst), k);
}
hipError_t launch_node_children(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first, uint32_t arity,
                                uint64_t *rows, size_t k, hipStream_t st) {
    return plain(node_children_kernel, k * 2 * arity, st, u4(nodes), indices, pow, n_leaves, first, arity, u4(rows), k);
}

// ---- fixed-depth trees (pmx_merkle_fixed*, pmx_merkle_frontier_append) ----------------------------------------------------------------
// Pure data movement around the compression launches, driven by a list the host built (pmx_merkle_frontier.hpp): entry i is the pair
// (list[2 i], list[2 i + 1]) = (destination element, source element) of `elems`, two lanes per entry, one 16-byte half each.  It lays the
// uploaded frontier nodes and the default digests into the levels' rows before the walk and collects the new frontier and the root behind
// it.  Sources and destinations of one launch never overlap (the host's lists read what was uploaded or computed and write elsewhere),
// but they lie in one array: no __restrict__ on it.
__global__ void __launch_bounds__(256) node_place_kernel(uint4 *elems, const uint64_t *__restrict__ list, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 1;
    if (i >= k) return;
    elems[list[2 * i] * 2 + (gid & 1)] = elems[list[2 * i + 1] * 2 + (gid & 1)];
}
hipError_t launch_node_place(uint64_t *elems, const uint64_t *list, size_t k, hipStream_t st) {
    return plain(node_place_kernel, k * 2, st, u4(elems), list, k);
}

// ---- sequential leaf updates of a fixed-depth tree (pmx_merkle_update_witnesses) ------------------------------------------------------
// One level of k chained updates, pure data movement in front of the level's compression launch: 2 arity lanes per update, one 16-byte
// half of a child each.  Row j of `rows` is the arity children of update j's parent at this level as update j sees them: its own running
// node cur[j] at digit (indices[j] / pow) % arity (pow = arity^level), and in sibling slot s the running node cur[pred[j][s]] of the last
// earlier update that wrote that sibling, or - no such update - slab[j][s], the sibling of the caller's old opening (pmx_merkle_chain.hpp
// computes pred).  The same lane stores a sibling's piece into wit[j][s] (unless wit is null): the level's slab of the witness.
// A predecessor is an EARLIER update: whatever pred holds, a value that is not below j (kChainNone among them) reads the slab, so nothing
// outside cur [k][4] and slab [k][arity - 1][4] is read.
__global__ void __launch_bounds__(256) chain_rows_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ slab,
                                                         const uint32_t *__restrict__ pred, const uint64_t *__restrict__ indices, uint64_t pow,
                                                         uint32_t arity, uint4 *__restrict__ rows, uint4 *__restrict__ wit, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, j = gid / per;
    if (j >= k) return;
    const uint32_t quarter = (uint32_t)(gid - j * per), child = quarter >> 1, half = quarter & 1;
    const uint32_t digit = (uint32_t)((indices[j] / pow) % arity);
    if (child == digit) {
        rows[gid] = cur[j * 2 + half];
        return;
    }
    const size_t slot = j * (arity - 1) + (child < digit ? child : child - 1);
    const size_t p = pred[slot];
    const uint4 v = p < j ? cur[p * 2 + half] : slab[slot * 2 + half];
    rows[gid] = v;
    if (wit) wit[slot * 2 + half] = v;
}
hipError_t launch_chain_rows(const uint64_t *cur, const uint64_t *slab, const uint32_t *pred, const uint64_t *indices, uint64_t pow,
                             uint32_t arity, uint64_t *rows, uint64_t *wit, size_t k, hipStream_t st) {
    return plain(chain_rows_kernel, k * 2 * arity, st, u4(cur), u4(slab), pred, indices, pow, arity, u4(rows), u4(wit), k);
}

hipError_t launch_path_pairs(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level,
                             uint64_t *pairs, size_t k, hipStream_t st) {
    return plain(path_pairs_kernel, k * 4, st, u4(cur), u4(paths), indices, depth, level, u4(pairs), k);
}
hipError_t launch_path_children(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level, uint64_t pow,
                                uint32_t arity, uint64_t *rows, size_t k, hipStream_t st) {
    return plain(path_children_kernel, k * 2 * arity, st, u4(cur), u4(paths), indices, depth, level, pow, arity, u4(rows), k);
}
hipError_t launch_paths_gather(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices, uint64_t *paths,
                               size_t k, hipStream_t st) {
    return plain(paths_gather_kernel, k * depth * 2 * (arity - 1), st, u4(nodes), n_leaves, arity, depth, indices, u4(paths), k);
}
hipError_t launch_path_check(const uint64_t *cur, const uint64_t *root, const uint64_t *indices, uint64_t limit, uint8_t *ok,
                             size_t k, hipStream_t st) {
    return plain(path_check_kernel, k, st, u4(cur), u4(root), indices, limit, ok, k);
}

}  // namespace pmx
