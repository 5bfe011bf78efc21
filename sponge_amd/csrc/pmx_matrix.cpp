// C ABI of libposeidon_mi355x.so: the matrix commitment - row digests, the tree over them, opened rows and their verification - on a
// matrix in host memory (include/poseidon_mi355x.h) and, at the end of the file, on one that lives on the device
// (include/poseidon_mi355x_resident.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/poseidon_mi355x.h"
#include "../../include/poseidon_mi355x_resident.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"
#include "pmx_matrix_shape.hpp"

using namespace pmx;

// ---- matrix commitments -----------------------------------------------------------------------------
// A trace / LDE matrix to its row digests and the tree over them (include/poseidon_mi355x.h has the contract): leaf_i = (new; absorb(row i);
// squeeze_native(1))[0] (mod.rs:219-254, 321-341), the hash row of pmx_hash_batch at out_len = 1, read where the matrix lies.  The
// index arithmetic is pmx_matrix_shape.hpp's.  The matrix goes up in slabs of rows (PMX_MATRIX_SLAB_BYTES of them, 65536 rows at least:
// profiles/matrix_commit/README.md has the sweep) through two slab buffers (staging blocks of their own):
// `stream` uploads slab s + 1 while `stream2` hashes slab s (hash_strided_kernel, the slab's own strides) straight into rows [a, b) of
// the node array; an upload into a buffer waits for the hash that read it last.  The tree walk and the one download follow
// on `stream2`.  A column-major slab is ONE 2-D copy into a packed column-major buffer of leading dimension b - a.
namespace {

uint64_t matrix_slab_rows_of(size_t n_rows, size_t row_len) {
    const uint64_t hook = matrix_slab_rows_hook();
    if (hook) return hook < n_rows ? hook : n_rows;
    return matrix_slab_rows(n_rows, row_len, PMX_MATRIX_SLAB_BYTES);
}

// the checks every entry shares, none of which reads a context
int matrix_shape_args(size_t n_rows, size_t row_len, uint32_t layout, const char *who, uint64_t *bytes) {
    if (n_rows == 0) return set_error(PMX_ERR_ARG, "%s: a matrix needs at least one row", who);
    if (row_len == 0) return set_error(PMX_ERR_ARG, "%s: a row needs at least one element", who);
    if (!matrix_layout_ok(layout)) return set_error(PMX_ERR_ARG, "%s: layout %u is neither PMX_MATRIX_ROW_MAJOR nor PMX_MATRIX_COL_MAJOR", who, layout);
    if (!matrix_bytes(n_rows, row_len, bytes) || *bytes > SIZE_MAX) return set_error(PMX_ERR_ARG, "%s: matrix byte size overflows size_t", who);
    if (n_rows > kMaxLaunchUnits) return set_error(PMX_ERR_ARG, "batch too large");
    return PMX_OK;
}
int matrix_arity_fits(const pmx_ctx *ctx, uint32_t arity) {
    if (arity > ctx->dev.rounds.rate) return set_error(PMX_ERR_CONFIG, "arity %u exceeds the rate %u", arity, ctx->dev.rounds.rate);
    return PMX_OK;
}

// rows [0, n_rows) of `matrix` (host) hashed into d_leaves [n_rows][4]; everything ends enqueued on ctx->stream2.  `src` is
// page-locked or small (see matrix_host).
int matrix_leaves_enqueue(HostCall &call, const char *src, size_t n_rows, size_t row_len, uint32_t layout, uint64_t *d_leaves) {
    pmx_ctx *ctx = call.ctx;
    int rc = PMX_OK;
    const uint64_t slab_rows = matrix_slab_rows_of(n_rows, row_len), slabs = matrix_slabs(n_rows, slab_rows);
    Staging slab_layout;
    slab_layout.add(slab_layout.times((size_t)slab_rows, row_len), 32);   // one slab of rows; a second block of it when there are several
    char *d_slab[2] = {nullptr, nullptr};
    if ((rc = call.stage(slab_layout, &d_slab[0]))) return rc;
    if (slabs > 1 && (rc = call.stage(slab_layout, &d_slab[1]))) return rc;
    for (uint64_t s = 0; s < slabs; ++s) {
        const MatrixSlab slab = matrix_slab_at(n_rows, slab_rows, s);
        const MatrixCopy cp = matrix_slab_copy(layout, n_rows, row_len, slab);
        const MatrixStrides strides = matrix_strides(layout, row_len, slab.b - slab.a);
        const int slot = (int)(s % pmx_ctx::kPipeChunks);
        void *d = d_slab[s & 1];
        // (the hash of slab s - 2 read this buffer: its event is two slots back, recorded before this point)
        if (s >= 2) PMX_HIP(hipStreamWaitEvent(ctx->stream, ctx->pipe_done[(s - 2) % pmx_ctx::kPipeChunks], 0));
        if (cp.height == 1) PMX_HIP(hipMemcpyAsync(d, src + cp.src_offset, cp.width, hipMemcpyHostToDevice, ctx->stream));
        else PMX_HIP(hipMemcpy2DAsync(d, cp.dst_pitch, src + cp.src_offset, cp.src_pitch, cp.width, cp.height, hipMemcpyHostToDevice, ctx->stream));
        PMX_HIP(hipEventRecord(ctx->pipe_up[slot], ctx->stream));
        PMX_HIP(hipStreamWaitEvent(ctx->stream2, ctx->pipe_up[slot], 0));
        PMX_HIP(launch_hash_strided(ctx->dev, ctx->t, (const uint64_t *)d, row_len, strides.row, strides.elem, d_leaves + slab.a * 4, 1,
                                    (size_t)(slab.b - slab.a), ctx->stream2));
        PMX_HIP(hipEventRecord(ctx->pipe_done[slot], ctx->stream2));
    }
    return PMX_OK;
}

// leaves_out, or (tree) the node array and / or the root of the tree of `arity` over the digests; nodes / root may be NULL
int matrix_host(pmx_ctx *ctx, const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, bool tree, uint32_t arity,
                uint64_t *leaves_out, uint64_t *nodes, uint64_t *root, const char *who) {
    uint64_t bytes = 0;
    if (int rc = matrix_shape_args(n_rows, row_len, layout, who, &bytes)) return rc;
    size_t depth = 0, n_nodes = n_rows;
    if (tree) {
        if (int rc = pmx_merkle_ragged_shape(n_rows, arity, &depth, &n_nodes)) return rc;
        if (int rc = matrix_arity_fits(ctx, arity)) return rc;
    }
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    Staging node_array;
    node_array.add(n_nodes, 32);   // the digests, then (tree) every level above them
    char *d0 = nullptr;
    if ((rc = call.stage(node_array, &d0))) return rc;
    uint64_t *d_nodes = (uint64_t *)d0;
    // A page-locked matrix is copied from where it lies; a small pageable one goes through the context's page-locked block, a large one
    // is page-locked for the length of the call, and what lies between takes the runtime's own staging (unasked: its path is the same).
    const char *src = (const char *)matrix;
    if (bytes <= kSmallCallBytes) {
        if (!call.pin(matrix, (size_t)bytes)) {   // (too small to register: the pin only asks)
            char *h = nullptr;
            if ((rc = call.pinned_block(&h))) return rc;
            std::memcpy(h, matrix, (size_t)bytes);
            src = h;
        }
    } else {
        (void)call.pin(matrix, (size_t)bytes, false);
    }
    if ((rc = matrix_leaves_enqueue(call, src, n_rows, row_len, layout, d_nodes))) return rc;
    hipStream_t st = ctx->stream2;
    if (!tree) {
        PMX_HIP(hipMemcpyAsync(leaves_out, d_nodes, n_rows * 32, hipMemcpyDeviceToHost, st));
    } else {
        if ((rc = pmx_merkle_ragged_dev(ctx, d_nodes, n_rows, arity, st))) return rc;
        if (nodes) PMX_HIP(hipMemcpyAsync(nodes, d_nodes, n_nodes * 32, hipMemcpyDeviceToHost, st));
        if (root) PMX_HIP(hipMemcpyAsync(root, d_nodes + (n_nodes - 1) * 4, 32, hipMemcpyDeviceToHost, st));
    }
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
}

}  // namespace

extern "C" int pmx_matrix_leaves(pmx_ctx *ctx, const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, uint64_t *leaves_out) {
    PMX_ABI_BEGIN("pmx_matrix_leaves")
    if (!ctx || !matrix || !leaves_out) return set_error(PMX_ERR_ARG, "pmx_matrix_leaves: null pointer");
    return matrix_host(ctx, matrix, n_rows, row_len, layout, false, 0, leaves_out, nullptr, nullptr, "pmx_matrix_leaves");
    PMX_ABI_END
}

extern "C" int pmx_matrix_commit(pmx_ctx *ctx, const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, uint32_t arity,
                                 uint64_t *nodes, uint64_t *root) {
    PMX_ABI_BEGIN("pmx_matrix_commit")
    if (!ctx || !matrix) return set_error(PMX_ERR_ARG, "pmx_matrix_commit: null pointer");
    return matrix_host(ctx, matrix, n_rows, row_len, layout, true, arity, nullptr, nodes, root, "pmx_matrix_commit");
    PMX_ABI_END
}

// the opened rows, on the host: rows_out [k][row_len][4] row-major whatever the layout
extern "C" int pmx_matrix_rows(const uint64_t *matrix, size_t n_rows, size_t row_len, uint32_t layout, const uint64_t *indices, size_t k,
                               uint64_t *rows_out) {
    if (!matrix || ((!indices || !rows_out) && k)) return set_error(PMX_ERR_ARG, "pmx_matrix_rows: null pointer");
    uint64_t bytes = 0;
    if (int rc = matrix_shape_args(n_rows, row_len, layout, "pmx_matrix_rows", &bytes)) return rc;
    if (k > (SIZE_MAX / 32) / row_len) return set_error(PMX_ERR_ARG, "pmx_matrix_rows: rows byte size overflows size_t");
    for (size_t i = 0; i < k; ++i)
        if (indices[i] >= n_rows) return set_error(PMX_ERR_ARG, "row index %llu out of range", (unsigned long long)indices[i]);
    const MatrixStrides s = matrix_strides(layout, row_len, n_rows);
    for (size_t i = 0; i < k; ++i) {
        const uint64_t *row = matrix + (size_t)indices[i] * s.row * 4;
        uint64_t *out = rows_out + i * row_len * 4;
        if (s.elem == 1) std::memcpy(out, row, row_len * 32);
        else
            for (size_t j = 0; j < row_len; ++j) std::memcpy(out + j * 4, row + j * s.elem * 4, 32);
    }
    return PMX_OK;
}

// k opened rows against the root: the staged verify body of the Merkle entries (pmx_merkle.cpp: verify_host), which hashes the rows
// into the leaves by one strided-hash launch in front of the climb
extern "C" int pmx_matrix_verify_rows(pmx_ctx *ctx, const uint64_t *rows, size_t row_len, const uint64_t *indices, const uint64_t *paths,
                                      size_t depth, uint32_t arity, size_t n_rows, size_t k, const uint64_t root[PMX_LIMBS], uint8_t *ok_out) {
    PMX_ABI_BEGIN("pmx_matrix_verify_rows")
    if (!ctx || ((!rows || !indices || !ok_out) && k) || (!paths && k && depth) || !root)
        return set_error(PMX_ERR_ARG, "pmx_matrix_verify_rows: null pointer");
    if (row_len == 0) return set_error(PMX_ERR_ARG, "pmx_matrix_verify_rows: a row needs at least one element");
    size_t tree_depth = 0, n_nodes = 0;
    if (int rc = pmx_merkle_ragged_shape(n_rows, arity, &tree_depth, &n_nodes)) return rc;
    if (tree_depth != depth)
        return set_error(PMX_ERR_ARG, "depth %zu is not the depth %zu of a tree of arity %u over %zu leaves", depth, tree_depth, arity, n_rows);
    if (int rc = matrix_arity_fits(ctx, arity)) return rc;
    if (k == 0) return PMX_OK;
    if (k > kMaxLaunchUnits / arity) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    return verify_host(ctx, nullptr, rows, row_len, indices, paths, depth, arity, (uint64_t)n_rows, false, k, root, ok_out);
    PMX_ABI_END
}

// ---- the device-resident forms (include/poseidon_mi355x_resident.h) --------------------------------------------------------------------
// The matrix is a strided view of the caller's device memory (pmx_matrix_shape.hpp: matrix_view_extent), read where it lies by the
// kernel the slabs above are hashed with; the tree, the path gather and the climb are the ragged entries' own (pmx_merkle.cpp), called
// through their *_dev entry points on the caller's stream.  Each entry tests everything those would refuse before its first launch, so
// a refused call has launched nothing.  Enqueue only: nothing is allocated, nothing synchronised, and every entry may be captured.
namespace {

int matrix_view_args(size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride, const char *who, uint64_t *extent) {
    if (n_rows == 0) return set_error(PMX_ERR_ARG, "%s: a matrix needs at least one row", who);
    if (row_len == 0) return set_error(PMX_ERR_ARG, "%s: a row needs at least one element", who);
    if (row_stride == 0 || elem_stride == 0) return set_error(PMX_ERR_ARG, "%s: a stride of a view must be at least one element", who);
    if (!matrix_view_extent(n_rows, row_len, row_stride, elem_stride, extent) || *extent > SIZE_MAX / kMatrixElemBytes)
        return set_error(PMX_ERR_ARG, "%s: the view's byte size overflows size_t", who);
    return PMX_OK;
}
// a view some launch reads n_rows rows of
int matrix_view_launch_args(size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride, const char *who) {
    uint64_t extent = 0;
    if (int rc = matrix_view_args(n_rows, row_len, row_stride, elem_stride, who, &extent)) return rc;
    if (n_rows > kMaxLaunchUnits) return set_error(PMX_ERR_ARG, "batch too large");
    return PMX_OK;
}
int matrix_misaligned() { return set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned"); }
int matrix_indices_aligned(const uint64_t *d_indices) {
    if ((uintptr_t)d_indices & 7u) return set_error(PMX_ERR_ARG, "d_indices must be 8-byte aligned");
    return PMX_OK;
}

}  // namespace

extern "C" int pmx_matrix_view_extent(size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride, size_t *extent_elems) {
    if (!extent_elems) return set_error(PMX_ERR_ARG, "pmx_matrix_view_extent: null pointer");
    uint64_t extent = 0;
    if (int rc = matrix_view_args(n_rows, row_len, row_stride, elem_stride, "pmx_matrix_view_extent", &extent)) return rc;
    *extent_elems = (size_t)extent;
    return PMX_OK;
}

extern "C" int pmx_matrix_leaves_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride,
                                     size_t elem_stride, uint64_t *d_leaves, void *stream) {
    if (!ctx || !d_matrix || !d_leaves) return set_error(PMX_ERR_ARG, "pmx_matrix_leaves_dev: null pointer");
    if (int rc = matrix_view_launch_args(n_rows, row_len, row_stride, elem_stride, "pmx_matrix_leaves_dev")) return rc;
    if (!aligned16(d_matrix) || !aligned16(d_leaves)) return matrix_misaligned();
    PMX_BIND(ctx);
    PMX_HIP(launch_hash_strided(ctx->dev, ctx->t, d_matrix, row_len, row_stride, elem_stride, d_leaves, 1, n_rows, (hipStream_t)stream));
    return PMX_OK;
}

extern "C" int pmx_matrix_commit_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride,
                                     size_t elem_stride, uint32_t arity, uint64_t *d_nodes, void *stream) {
    if (!ctx || !d_matrix || !d_nodes) return set_error(PMX_ERR_ARG, "pmx_matrix_commit_dev: null pointer");
    if (int rc = matrix_view_launch_args(n_rows, row_len, row_stride, elem_stride, "pmx_matrix_commit_dev")) return rc;
    size_t depth = 0, n_nodes = 0;
    if (int rc = pmx_merkle_ragged_shape(n_rows, arity, &depth, &n_nodes)) return rc;
    if (int rc = matrix_arity_fits(ctx, arity)) return rc;
    if (!aligned16(d_matrix) || !aligned16(d_nodes)) return matrix_misaligned();
    PMX_BIND(ctx);
    PMX_HIP(launch_hash_strided(ctx->dev, ctx->t, d_matrix, row_len, row_stride, elem_stride, d_nodes, 1, n_rows, (hipStream_t)stream));
    if (depth == 0) return PMX_OK;   // one row: its digest is the root
    return pmx_merkle_ragged_dev(ctx, d_nodes, n_rows, arity, stream);
}

// the paths first (their entry tests its own arguments again), the rows behind them
extern "C" int pmx_matrix_open_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride,
                                   size_t elem_stride, const uint64_t *d_nodes, uint32_t arity, const uint64_t *d_indices, size_t k,
                                   uint64_t *d_rows, uint64_t *d_paths, void *stream) {
    if (!ctx || !d_matrix || ((!d_indices || !d_rows) && k)) return set_error(PMX_ERR_ARG, "pmx_matrix_open_dev: null pointer");
    if (int rc = matrix_view_launch_args(n_rows, row_len, row_stride, elem_stride, "pmx_matrix_open_dev")) return rc;
    if (d_paths && !d_nodes) return set_error(PMX_ERR_ARG, "pmx_matrix_open_dev: d_paths without d_nodes");
    size_t depth = 0, n_nodes = 0;
    if (d_nodes) {
        if (int rc = pmx_merkle_ragged_shape(n_rows, arity, &depth, &n_nodes)) return rc;
        if (int rc = matrix_arity_fits(ctx, arity)) return rc;
        if (!d_paths && k && depth) return set_error(PMX_ERR_ARG, "pmx_matrix_open_dev: d_nodes without d_paths");
    }
    if (k == 0) return PMX_OK;
    // (depth <= 64 and arity <= the rate here: the products stay small)
    const size_t per = depth * (d_nodes ? arity - 1 : 0);     // elements per path
    if (k > kMaxLaunchUnits / row_len || (d_nodes && k > kMaxLaunchUnits / arity) || (per && k > kMaxLaunchUnits / per))
        return set_error(PMX_ERR_ARG, "batch too large");
    if (!aligned16(d_matrix) || !aligned16(d_rows) || !aligned16(d_nodes) || !aligned16(d_paths)) return matrix_misaligned();
    if (int rc = matrix_indices_aligned(d_indices)) return rc;
    PMX_BIND(ctx);
    if (per)
        if (int rc = pmx_merkle_ragged_paths_dev(ctx, d_nodes, n_rows, arity, d_indices, k, d_paths, stream)) return rc;
    PMX_HIP(launch_matrix_rows(d_matrix, n_rows, row_len, row_stride, elem_stride, d_indices, d_rows, k, (hipStream_t)stream));
    return PMX_OK;
}

extern "C" int pmx_matrix_verify_rows_dev(pmx_ctx *ctx, const uint64_t *d_rows, size_t row_len, const uint64_t *d_indices,
                                          const uint64_t *d_paths, size_t depth, uint32_t arity, size_t n_rows, size_t k,
                                          const uint64_t *d_root, uint8_t *d_ok, uint64_t *d_work, void *stream) {
    if (!ctx || ((!d_rows || !d_indices || !d_ok || !d_work) && k) || (!d_paths && k && depth) || !d_root)
        return set_error(PMX_ERR_ARG, "pmx_matrix_verify_rows_dev: null pointer");
    if (row_len == 0) return set_error(PMX_ERR_ARG, "pmx_matrix_verify_rows_dev: a row needs at least one element");
    size_t tree_depth = 0, n_nodes = 0;
    if (int rc = pmx_merkle_ragged_shape(n_rows, arity, &tree_depth, &n_nodes)) return rc;
    if (tree_depth != depth)
        return set_error(PMX_ERR_ARG, "depth %zu is not the depth %zu of a tree of arity %u over %zu leaves", depth, tree_depth, arity, n_rows);
    if (int rc = matrix_arity_fits(ctx, arity)) return rc;
    if (k == 0) return PMX_OK;
    // (the bounds of the climb, pmx_merkle.cpp: verify_dev, and the rows' own)
    if (k > kMaxLaunchUnits / arity || k > (SIZE_MAX / 32) / (arity + 2) || k > (SIZE_MAX / 32) / row_len ||
        (depth && k > (SIZE_MAX / 32) / (depth * (arity - 1))))
        return set_error(PMX_ERR_ARG, "batch too large");
    if (!aligned16(d_rows) || !aligned16(d_paths) || !aligned16(d_root) || !aligned16(d_work)) return matrix_misaligned();
    if (int rc = matrix_indices_aligned(d_indices)) return rc;
    PMX_BIND(ctx);
    PMX_HIP(launch_hash_strided(ctx->dev, ctx->t, d_rows, row_len, row_len, 1, d_work, 1, k, (hipStream_t)stream));
    return pmx_merkle_ragged_verify_paths_dev(ctx, d_work, d_indices, d_paths, depth, arity, n_rows, k, d_root, d_ok, d_work + k * 4, stream);
}
