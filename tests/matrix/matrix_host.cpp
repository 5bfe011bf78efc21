// The index arithmetic of the matrix entries (sponge_amd/csrc/pmx_matrix_shape.hpp) as a program of its own, built with
// -fsanitize=address,undefined by tests/test_matrix_host.py and run directly.
//   matrix_host                              the self-check below ("sanitized ok")
//   matrix_host walk <n_rows> <slab_rows>    the slabs, one "a b" line each
//   matrix_host copy <layout> <n_rows> <row_len> <a> <b>    "src_offset src_pitch dst_pitch width height row_stride elem_stride" of that slab
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pmx_matrix_shape.hpp"

using namespace pmx;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static int self_check() {
    // the walk: ascending, disjoint, exactly [0, n) - one slab, slabs of one row, a short last slab, a slab larger than the matrix
    for (uint64_t n : {1ull, 2ull, 63ull, 64ull, 65ull, 1000ull}) {
        for (uint64_t slab_rows : {1ull, 7ull, 64ull, (unsigned long long)n, (unsigned long long)n + 1}) {
            const uint64_t slabs = matrix_slabs(n, slab_rows);
            if (slabs != (n + slab_rows - 1) / slab_rows) return fail("matrix_slabs");
            uint64_t next = 0;
            for (uint64_t s = 0; s < slabs; ++s) {
                const MatrixSlab g = matrix_slab_at(n, slab_rows, s);
                if (g.a != next || g.b <= g.a || g.b > n || g.b - g.a > slab_rows) return fail("slab out of order or out of size");
                if (s + 1 < slabs && g.b - g.a != slab_rows) return fail("a slab before the last is short");
                next = g.b;
            }
            if (next != n) return fail("the slabs do not cover the rows");
        }
    }
    // strides and the 2-D copy: a slab copied as matrix_slab_copy says, then read through the slab's own strides, is the rows it names
    for (uint32_t layout : {kMatrixRowMajor, kMatrixColMajor}) {
        for (uint64_t n : {1ull, 5ull, 65ull}) {
            for (uint64_t len : {1ull, 3ull, 9ull}) {
                std::vector<uint64_t> m(n * len * 4);
                for (uint64_t i = 0; i < n; ++i)
                    for (uint64_t j = 0; j < len; ++j)
                        for (uint64_t w = 0; w < 4; ++w) m[matrix_element(layout, n, len, i, j) * 4 + w] = (i << 32) | (j << 8) | w;
                const MatrixStrides whole = matrix_strides(layout, len, n);
                if (layout == kMatrixRowMajor ? (whole.row != len || whole.elem != 1) : (whole.row != 1 || whole.elem != n)) return fail("strides of a layout");
                uint64_t bytes = 0;
                if (!matrix_bytes(n, len, &bytes) || bytes != m.size() * 8) return fail("matrix_bytes");
                for (uint64_t slab_rows : {1ull, 2ull, 64ull}) {
                    for (uint64_t s = 0; s < matrix_slabs(n, slab_rows); ++s) {
                        const MatrixSlab g = matrix_slab_at(n, slab_rows, s);
                        const uint64_t rows = g.b - g.a;
                        const MatrixCopy c = matrix_slab_copy(layout, n, len, g);
                        if (layout == kMatrixColMajor &&
                            (c.width != rows * 32 || c.height != len || c.src_pitch != n * 32 || c.dst_pitch != rows * 32 || c.src_offset != g.a * 32))
                            return fail("geometry of a column-major slab");
                        if (layout == kMatrixRowMajor && (c.height != 1 || c.width != rows * len * 32 || c.src_offset != g.a * len * 32))
                            return fail("geometry of a row-major slab");
                        if (c.width > c.src_pitch || c.width > c.dst_pitch) return fail("a run longer than its pitch");
                        if (c.src_offset + (c.height - 1) * c.src_pitch + c.width > bytes) return fail("the copy reads beyond the matrix");
                        std::vector<uint64_t> slab(rows * len * 4, ~0ull);   // exactly the slab's bytes: ASan sees a copy that runs over
                        if ((c.height - 1) * c.dst_pitch + c.width != slab.size() * 8) return fail("the copy does not fill the slab exactly");
                        for (uint64_t r = 0; r < c.height; ++r)
                            std::memcpy((char *)slab.data() + r * c.dst_pitch, (const char *)m.data() + c.src_offset + r * c.src_pitch, c.width);
                        const MatrixStrides st = matrix_strides(layout, len, rows);
                        for (uint64_t i = 0; i < rows; ++i)
                            for (uint64_t j = 0; j < len; ++j)
                                for (uint64_t w = 0; w < 4; ++w)
                                    if (slab[(i * st.row + j * st.elem) * 4 + w] != (((g.a + i) << 32) | (j << 8) | w)) return fail("a slab element is not the matrix element");
                    }
                }
            }
        }
    }
    // sizes: refused when a dimension is zero or the bytes do not fit 64 bits; *bytes untouched then
    uint64_t bytes = 77;
    if (matrix_bytes(0, 5, &bytes) || matrix_bytes(5, 0, &bytes) || matrix_bytes((uint64_t)1 << 59, 2, &bytes) || matrix_bytes((uint64_t)1 << 30, (uint64_t)1 << 30, &bytes) ||
        matrix_bytes(UINT64_MAX, 1, &bytes) || matrix_bytes(1, UINT64_MAX, &bytes) || bytes != 77)
        return fail("an overflowing or empty matrix passes");
    if (matrix_bytes((uint64_t)1 << 59, 1, &bytes) || bytes != 77) return fail("2^64 bytes pass");
    if (!matrix_bytes((uint64_t)1 << 58, 1, &bytes) || bytes != (uint64_t)1 << 63) return fail("2^63 bytes are refused");
    if (!matrix_bytes(((uint64_t)1 << 59) - 1, 1, &bytes) || bytes != UINT64_MAX - 31) return fail("the largest matrix is refused");
    if (!matrix_layout_ok(0) || !matrix_layout_ok(1) || matrix_layout_ok(2) || matrix_layout_ok(UINT32_MAX)) return fail("matrix_layout_ok");
    // the node array through pmx_merkle_shape.hpp
    MerkleShape shape;
    if (matrix_tree_shape(1000, 2, &shape) != MerkleShapeError::ok || shape.depth != 10 || shape.n_nodes != 1000 + 500 + 250 + 125 + 63 + 32 + 16 + 8 + 4 + 2 + 1)
        return fail("tree over 1000 rows");
    if (matrix_tree_shape(5, 1, &shape) != MerkleShapeError::arity || matrix_tree_shape(0, 2, &shape) != MerkleShapeError::no_leaves) return fail("tree refusals");
    if (sizeof(size_t) == 8 && matrix_tree_shape((uint64_t)1 << 59, 2, &shape) != MerkleShapeError::tree_overflow) return fail("tree byte size overflow");
    // rows per slab: what the budget holds in whole workgroups, 65536 rows at least, never more than the matrix
    if (matrix_slab_rows(1 << 20, 8, 32 << 20) != 131072 || matrix_slab_rows(1000, 8, 32 << 20) != 1000 || matrix_slab_rows(1 << 20, 64, 32 << 20) != 65536 ||
        matrix_slab_rows(1 << 20, 3, 32 << 20) != 349440 || matrix_slab_rows(1 << 20, 1 << 22, 32 << 20) != 65536 || matrix_slab_rows(70000, 64, 1) != 65536)
        return fail("matrix_slab_rows");
    std::printf("sanitized ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (!std::strcmp(argv[1], "walk") && argc == 4) {
        const uint64_t n = std::strtoull(argv[2], nullptr, 10), slab_rows = std::strtoull(argv[3], nullptr, 10);
        if (n == 0 || slab_rows == 0) return 2;
        for (uint64_t s = 0; s < matrix_slabs(n, slab_rows); ++s) {
            const MatrixSlab g = matrix_slab_at(n, slab_rows, s);
            std::printf("%" PRIu64 " %" PRIu64 "\n", g.a, g.b);
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "copy") && argc == 7) {
        const uint32_t layout = (uint32_t)std::strtoul(argv[2], nullptr, 10);
        const uint64_t n = std::strtoull(argv[3], nullptr, 10), len = std::strtoull(argv[4], nullptr, 10);
        const MatrixSlab g{std::strtoull(argv[5], nullptr, 10), std::strtoull(argv[6], nullptr, 10)};
        if (!matrix_layout_ok(layout) || g.a >= g.b || g.b > n || len == 0) return 2;
        const MatrixCopy c = matrix_slab_copy(layout, n, len, g);
        const MatrixStrides st = matrix_strides(layout, len, g.b - g.a);
        std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c.src_offset, c.src_pitch, c.dst_pitch, c.width, c.height,
                    st.row, st.elem);
        return 0;
    }
    return 2;
}
