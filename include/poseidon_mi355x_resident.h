/*
 * poseidon_mi355x_resident.h -- the device-resident forms of families whose entries in poseidon_mi355x.h take host buffers.  Exported by
 * libposeidon_mi355x.so (and by the test library) next to the main header's functions; the ABI version is the main header's, this header
 * carries none of its own.  Not in the Rust binding yet.
 *
 * Everything the main header says about its *_dev entry points holds here and is not restated: status codes and pmx_last_error, the
 * threading rules, "Graph capture", "Alignment of device pointers" (element arrays 16 bytes, d_indices 8 bytes, d_ok any address), the
 * context's device bound for the call and restored, `stream` (NULL = default stream) belonging to the context's device.  Every
 * stream-taking entry below only enqueues on the caller's stream, allocates nothing, synchronises nothing, and MAY BE CAPTURED into a
 * graph.
 */
#ifndef POSEIDON_MI355X_RESIDENT_H
#define POSEIDON_MI355X_RESIDENT_H

#include "poseidon_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- matrix commitments on a matrix that lives on the device -------------------------------------------
 * The family of pmx_matrix_leaves / _commit / _rows / _verify_rows (poseidon_mi355x.h: what a leaf, the node array, an opening and a
 * verdict are) without the link: the matrix, the node array, the query indices, the opened rows, their paths and the verdicts all stay
 * on the device, so a transcript can absorb, commit, absorb the root, squeeze its queries, open and verify without a host round trip.
 *
 * The matrix is a STRIDED VIEW of device memory: element (i, j), i < n_rows, j < row_len, is the 4 limbs at
 *   d_matrix + (i * row_stride + j * elem_stride) * 4,     strides counted in elements.
 * Column-major with leading dimension ld >= n_rows is (row_stride, elem_stride) = (1, ld) - what an NTT leaves behind -, packed
 * row-major is (row_len, 1), pitched row-major (pitch, 1), and a block of a larger matrix is a view like any other.  Nothing is
 * transposed or copied; only the n_rows * row_len elements of the view are read.  Views whose elements overlap are legal (the matrix is
 * only read).  Outputs (d_leaves, d_nodes, d_rows, d_paths, d_ok, d_work) must not overlap the view or each other: the result of a call
 * where they do is unspecified, and it is not checked.
 *
 * pmx_matrix_view_extent: host only, no context.  *extent_elems = 1 + (n_rows - 1) * row_stride + (row_len - 1) * elem_stride, the
 *   elements from d_matrix that the view spans (extent * 32 bytes must be readable device memory).  PMX_ERR_ARG for n_rows = 0,
 *   row_len = 0, a zero stride, or an extent whose byte size overflows size_t.  Every entry below refuses what this one refuses.
 * pmx_matrix_leaves_dev: d_leaves [n_rows][4] = the row digests, byte for byte pmx_matrix_leaves on the same matrix
 *   (pmx_hash_batch(in_len = row_len, out_len = 1) on its row-major copy).  ONE strided hash launch over the n_rows rows, on the engine
 *   pmx_ctx_engine_info(ctx, PMX_OP_HASH, n_rows, row_len) names.
 * pmx_matrix_commit_dev: d_nodes [n_nodes][4], n_nodes from pmx_merkle_ragged_shape(n_rows, arity): the digests land in its first
 *   n_rows rows and the walk of pmx_merkle_ragged_dev follows on the same stream; the root is the last row.  Byte for byte the `nodes`
 *   of pmx_matrix_commit.  At n_rows = 1 the leaf is the root and only the hash launch runs.
 * pmx_matrix_open_dev: d_rows [k][row_len][4] = the rows d_indices names, each row contiguous whatever the view - the layout
 *   pmx_matrix_rows gives and pmx_matrix_verify_rows[_dev] takes.  With d_nodes (the node array of pmx_matrix_commit_dev for the same
 *   n_rows and arity) d_paths [k][depth][arity - 1][4] receives exactly what pmx_merkle_ragged_paths_dev gives on it; with d_nodes = NULL
 *   d_paths must be NULL too, arity is not read, and only the rows are gathered.  Device-resident indices are not validated: an index
 *   >= n_rows gets an all-zero row and an all-zero path, and nothing outside the view or the node array is read.  At most two launches:
 *   the path gather, then the row gather (one lane per 16-byte half of an element, consecutive along the row).
 * pmx_matrix_verify_rows_dev: d_ok[i] = 1 iff the digest of d_rows[i] climbs d_paths[i] to *d_root AND d_indices[i] < n_rows, else 0:
 *   one strided hash launch of the k rows into the head of d_work, then the climb of pmx_merkle_ragged_verify_paths_dev.  d_work is
 *   [k][(arity + 2) * 4] u64 of scratch: the k digests, then that climb's [k][(arity + 1) * 4].  depth must be the depth of
 *   (n_rows, arity).  d_root [4] is device memory.
 * k = 0: PMX_OK, nothing launched (the arrays indexed by k may then be NULL, as for the host entries; so may d_paths at depth 0).
 * Errors, nothing launched or written on any: PMX_ERR_ARG for null pointers, a view pmx_matrix_view_extent refuses, n_rows, k * row_len or
 *   k * arity beyond the launch grid ("batch too large"), arity < 2, a depth that is not the tree's, d_paths without d_nodes or d_nodes
 *   without d_paths, an element array that is not 16-byte aligned ("device pointers must be 16-byte aligned") or d_indices that is not
 *   8-byte aligned; PMX_ERR_CONFIG for arity > rate. */
int pmx_matrix_view_extent(size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride, size_t *extent_elems);
int pmx_matrix_leaves_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                          uint64_t *d_leaves, void *stream);
int pmx_matrix_commit_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                          uint32_t arity, uint64_t *d_nodes, void *stream);
int pmx_matrix_open_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                        const uint64_t *d_nodes /* may be NULL */, uint32_t arity, const uint64_t *d_indices, size_t k, uint64_t *d_rows,
                        uint64_t *d_paths /* NULL iff d_nodes is NULL */, void *stream);
int pmx_matrix_verify_rows_dev(pmx_ctx *ctx, const uint64_t *d_rows, size_t row_len, const uint64_t *d_indices, const uint64_t *d_paths,
                               size_t depth, uint32_t arity, size_t n_rows, size_t k, const uint64_t *d_root, uint8_t *d_ok,
                               uint64_t *d_work, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* POSEIDON_MI355X_RESIDENT_H */
