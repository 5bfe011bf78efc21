// The index arithmetic of the matrix entries (pmx_matrix_*, pmx_matrix.cpp): how a layout addresses its elements, how the rows of a matrix
// are cut into slabs for the upload, the byte sizes, the 2-D copy that lifts a slab of rows out of a column-major matrix, and the span
// of a strided view of a matrix on the device.
// Pure 64-bit arithmetic, host only; compiled into tests/matrix/matrix_host.cpp as well.
//
// A matrix has n_rows rows of row_len elements of 32 bytes.  Row-major: element (i, j) at element index i * row_len + j.  Column-major:
// at j * n_rows + i.  The strided hash kernel (pmx_kernels.hpp: hash_strided_kernel) reads element k of row i at
// i * row_stride + k * elem_stride, so a layout is a pair of strides.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pmx_merkle_shape.hpp"

namespace pmx {

constexpr uint32_t kMatrixRowMajor = 0, kMatrixColMajor = 1;   // PMX_MATRIX_ROW_MAJOR, PMX_MATRIX_COL_MAJOR
constexpr uint64_t kMatrixElemBytes = 32;

inline bool matrix_layout_ok(uint32_t layout) { return layout == kMatrixRowMajor || layout == kMatrixColMajor; }

struct MatrixStrides {
    uint64_t row, elem;   // in elements
};
// `ld`: the leading dimension of a column-major matrix, the rows it holds (n_rows for the caller's matrix, b - a for a slab's own copy);
// a row-major matrix has none
inline MatrixStrides matrix_strides(uint32_t layout, uint64_t row_len, uint64_t ld) {
    return layout == kMatrixColMajor ? MatrixStrides{1, ld} : MatrixStrides{row_len, 1};
}
// element (i, j) of the whole matrix, as an element index
inline uint64_t matrix_element(uint32_t layout, uint64_t n_rows, uint64_t row_len, uint64_t i, uint64_t j) {
    const MatrixStrides s = matrix_strides(layout, row_len, n_rows);
    return i * s.row + j * s.elem;
}

// n_rows * row_len * 32 bytes; false when either dimension is zero or the product does not fit 64 bits.  Writes *bytes only on success.
inline bool matrix_bytes(uint64_t n_rows, uint64_t row_len, uint64_t *bytes) {
    if (n_rows == 0 || row_len == 0) return false;
    if (row_len > (UINT64_MAX / kMatrixElemBytes) / n_rows) return false;
    *bytes = n_rows * row_len * kMatrixElemBytes;
    return true;
}
// A matrix that lives on the device is a strided view (include/poseidon_mi355x_resident.h): element (i, j) at element index
// i * row_stride + j * elem_stride, whatever the strides - (1, ld) column-major, (row_len, 1) or (pitch, 1) row-major, a block of a
// larger matrix.  The elements it spans, 1 + (n_rows - 1) * row_stride + (row_len - 1) * elem_stride: false for an empty dimension, a
// zero stride, or a span whose byte size does not fit 64 bits.  Every element index of the view is then below *extent <= 2^59 - 1, so
// the gather's 64-bit products cannot wrap.  Writes *extent only on success.
inline bool matrix_view_extent(uint64_t n_rows, uint64_t row_len, uint64_t row_stride, uint64_t elem_stride, uint64_t *extent) {
    if (n_rows == 0 || row_len == 0 || row_stride == 0 || elem_stride == 0) return false;
    const uint64_t limit = UINT64_MAX / kMatrixElemBytes;   // the most elements whose bytes fit
    if (n_rows > 1 && row_stride > limit / (n_rows - 1)) return false;
    if (row_len > 1 && elem_stride > limit / (row_len - 1)) return false;
    const uint64_t down = (n_rows - 1) * row_stride, across = (row_len - 1) * elem_stride;   // each <= limit < 2^59
    if (down + across + 1 > limit) return false;
    *extent = down + across + 1;
    return true;
}

// the node array of the tree over the n_rows digests (pmx_merkle_shape.hpp: any leaf count): n_nodes and depth, refused as there
inline MerkleShapeError matrix_tree_shape(uint64_t n_rows, uint32_t arity, MerkleShape *out) { return merkle_shape((size_t)n_rows, arity, false, out); }

// Rows per slab for a budget of `slab_bytes` of device memory, but never fewer than kMatrixMinSlabRows: a launch of fewer rows leaves
// the chip partly empty whatever its bytes (and at t = 3 falls to the quad engine, the latency engine), so a matrix of long rows takes
// slabs of that many rows and more memory than the budget (profiles/matrix_commit/README.md: the sweep).  Whole workgroups of 256 rows,
// at most n_rows.
constexpr uint64_t kMatrixMinSlabRows = 65536;
inline uint64_t matrix_slab_rows(uint64_t n_rows, uint64_t row_len, uint64_t slab_bytes) {
    uint64_t rows = slab_bytes / kMatrixElemBytes / row_len;   // (row_len >= 1)
    if (rows < kMatrixMinSlabRows) rows = kMatrixMinSlabRows;
    rows -= rows % 256;
    return rows < n_rows ? rows : n_rows;
}
// slabs the matrix takes: ceil(n_rows / slab_rows), slab_rows >= 1
inline uint64_t matrix_slabs(uint64_t n_rows, uint64_t slab_rows) { return n_rows / slab_rows + (n_rows % slab_rows != 0); }

struct MatrixSlab {
    uint64_t a, b;   // rows [a, b), a < b <= n_rows
};
// slab s < matrix_slabs(n_rows, slab_rows): ascending, disjoint, together exactly [0, n_rows)
inline MatrixSlab matrix_slab_at(uint64_t n_rows, uint64_t slab_rows, uint64_t s) {
    const uint64_t a = s * slab_rows;   // < n_rows
    return MatrixSlab{a, n_rows - a < slab_rows ? n_rows : a + slab_rows};
}

// The copy that takes rows [a, b) of the caller's matrix into a slab buffer, as the arguments of a 2-D copy: `height` runs of `width`
// bytes, the source runs `src_pitch` apart starting at byte `src_offset` of the matrix, the destination runs `dst_pitch` apart.
//   column-major: one run per column - width (b - a) * 32, height row_len, source pitch n_rows * 32, the slab packed with ld = b - a;
//   row-major: the rows are one contiguous piece - a single run of (b - a) * row_len * 32 bytes.
struct MatrixCopy {
    uint64_t src_offset, src_pitch, dst_pitch, width, height;
};
inline MatrixCopy matrix_slab_copy(uint32_t layout, uint64_t n_rows, uint64_t row_len, MatrixSlab s) {
    const uint64_t rows = s.b - s.a;
    if (layout == kMatrixColMajor) return MatrixCopy{s.a * kMatrixElemBytes, n_rows * kMatrixElemBytes, rows * kMatrixElemBytes, rows * kMatrixElemBytes, row_len};
    const uint64_t run = rows * row_len * kMatrixElemBytes;
    return MatrixCopy{s.a * row_len * kMatrixElemBytes, run, run, run, 1};
}

}  // namespace pmx
